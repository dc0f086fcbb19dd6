// pcp_ascii_parse.hip -- PCD ASCII rows parsed on the device ("Device PCD reader"): the x y z intensity floats of a
// window of text, bit for bit what strtof returns for their tokens (csrc/pcp_ascii_parse.hpp), or the index of the first row
// that is outside the grammar.  Opt-in: nothing here runs unless pcp_ascii_parse is called.
//
// The host cuts the window into pieces that end on a '\n' (kParsePiece bytes at most) and moves them through two slots of
// pinned staging and device buffers: the copy of piece k + 1 into pinned memory and its upload overlap the kernels of piece k
// and the download of piece k - 1.  Four launches per piece:
//   k_parse_count   16 bytes per lane, 4 096 per workgroup: the '\n' bytes of every tile of text;
//   k_scan_tile_offsets (pcp_scan.hpp)  ONE workgroup: exclusive prefix of the tile counts, the row count;
//   k_parse_index   the same loads again: the 32-bit offset of every '\n', in order (row r is [end[r - 1] + 1, end[r]));
//   k_parse_rows    a row per lane, 256 rows per workgroup: their contiguous span of text is staged into LDS with 16-byte
//                   loads and walked there; a span above kParseTile bytes (long rows: rare) is walked in global memory by
//                   the same code.  SoA outputs, 4-byte stores per lane; the first bad row by a vector atomic min on one word.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pcp_ascii_parse.hpp"
#include "pcp_internal.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // (only the single-workgroup scan of pcp_scan.hpp is used here)
#include "pcp_scan.hpp"
#pragma clang diagnostic pop

namespace pcp {

static_assert(ascii::kParseMaxRow == PCP_ASCII_PARSE_MAX_ROW, "the row limit of the header");

constexpr int kPaBlock = 256;                         // lanes of every kernel; rows of a tile of k_parse_rows
constexpr int kPaTextTile = kPaBlock * 16;            // bytes of text per workgroup of the count / index kernels
constexpr int32_t kParseTile = 24 * 1024;             // LDS staging of k_parse_rows (256 rows of 60 B are 15 KB)
constexpr int64_t kParsePiece = int64_t(8) << 20;     // bytes per upload piece
constexpr int64_t kParseWindowMax = (int64_t(1) << 31) - 1;

// rows a piece of `bytes` bytes can hold in front of its first bad row: a good row has a token and a '\n' (2 bytes), so
// bytes / 2 + 1 rows of 2 bytes or more do not fit and one of the first bytes / 2 + 1 rows is bad if there are more
static inline int64_t piece_row_cap(int64_t bytes) { return bytes / 2 + 1; }

__device__ __forceinline__ uint32_t newline_mask(const uint4 &v, int64_t base, int64_t bytes) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == 0x0au && base + k < bytes) m |= 1u << k;
  return m;
}

// text: bytes rounded up to 16 and 16 more are allocated, so every lane's load is inside the buffer
__global__ __launch_bounds__(kPaBlock) void k_parse_count(const uint8_t *__restrict__ text, int64_t bytes, int32_t *__restrict__ tile_count) {
  __shared__ int32_t ws[kPaBlock / 64];
  const int64_t tiles = (bytes + kPaTextTile - 1) / kPaTextTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kPaTextTile + 16 * static_cast<int64_t>(threadIdx.x);
    int32_t c = 0;
    if (base < bytes) c = __popc(newline_mask(*reinterpret_cast<const uint4 *>(text + base), base, bytes));
    int32_t total;
    (void)scan_block_exclusive(c, &total, ws);
    if (threadIdx.x == 0) tile_count[tile] = total;
  }
}

// end[i] = offset of the i-th '\n' for i < cap
__global__ __launch_bounds__(kPaBlock) void k_parse_index(const uint8_t *__restrict__ text, int64_t bytes, const int32_t *__restrict__ tile_offset,
                                                          int32_t *__restrict__ end, int64_t cap) {
  __shared__ int32_t ws[kPaBlock / 64];
  const int64_t tiles = (bytes + kPaTextTile - 1) / kPaTextTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kPaTextTile + 16 * static_cast<int64_t>(threadIdx.x);
    uint32_t m = 0;
    if (base < bytes) m = newline_mask(*reinterpret_cast<const uint4 *>(text + base), base, bytes);
    int32_t total;
    int64_t at = static_cast<int64_t>(tile_offset[tile]) + scan_block_exclusive(__popc(m), &total, ws);
    while (m) {
      const int k = __ffs(m) - 1;
      m &= m - 1u;
      if (at < cap) end[at] = static_cast<int32_t>(base + k);
      ++at;
    }
  }
}

struct ParseResult {  // one per slot, downloaded after the kernels of a piece
  unsigned long long newlines;
  uint32_t bad, pad;
};

// Rows [0, min(newlines + tail_row, cap)) of the piece: row r is text[r ? end[r - 1] + 1 : 0, r < newlines ? end[r] : bytes).
// out: four planes of `cap` words (x y z intensity).  res->bad = min over the bad rows (0xffffffff on entry).
__global__ __launch_bounds__(kPaBlock) void k_parse_rows(const uint8_t *__restrict__ text, int32_t bytes, const int32_t *__restrict__ end,
                                                         ParseResult *res, int32_t tail_row, int64_t cap, ascii::RowCols rc,
                                                         uint32_t *__restrict__ out) {
  __shared__ uint4 tile4[kParseTile / 16 + 2];
  const int64_t newlines = static_cast<int64_t>(res->newlines);
  const int64_t rows = min(newlines + (tail_row ? 1 : 0), cap);
  const int64_t tiles = (rows + kPaBlock - 1) / kPaBlock;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kPaBlock, r1 = min(r0 + kPaBlock, rows);  // the workgroup's rows
    const int32_t span_b = r0 ? end[r0 - 1] + 1 : 0;
    const int32_t span_e = r1 - 1 < newlines ? end[r1 - 1] : bytes;
    const int32_t lds_base = span_b & ~15;  // the staged bytes are text[lds_base, span_e), 16-byte words of text
    const bool staged = span_e - lds_base <= kParseTile;
    if (staged) {
      for (int32_t p = lds_base + 16 * static_cast<int32_t>(threadIdx.x); p < span_e; p += 16 * kPaBlock)
        tile4[(p - lds_base) >> 4] = *reinterpret_cast<const uint4 *>(text + p);
    }
    __syncthreads();
    const int64_t r = r0 + threadIdx.x;
    if (r < r1) {
      const int32_t b = r ? end[r - 1] + 1 : 0;
      const int32_t e = r < newlines ? end[r] : bytes;
      uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
      bool ok;
      if (staged)
        ok = ascii::parse_row(reinterpret_cast<const uint8_t *>(tile4), b - lds_base, e - lds_base, rc, &v0, &v1, &v2, &v3);
      else
        ok = ascii::parse_row(text, b, e, rc, &v0, &v1, &v2, &v3);
      if (ok) {
        out[r] = v0;
        out[cap + r] = v1;
        out[2 * cap + r] = v2;
        out[3 * cap + r] = v3;
      } else {
        atomicMin(&res->bad, static_cast<uint32_t>(r));
      }
    }
    __syncthreads();
  }
}

hipError_t preload_ascii_parse() {
  hipFuncAttributes a;
  return hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_parse_rows));
}

void ascii_parse_release(pcp_context *ctx) {
  for (auto &s : ctx->parse_slot) {
    if (s.stage) (void)hipHostFree(s.stage);
    if (s.res_h) (void)hipHostFree(s.res_h);
    s.stage = nullptr;
    s.res_h = nullptr;
    for (hipEvent_t *e : {&s.staged, &s.parsed, &s.drained}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
  }
  for (hipStream_t *st : {&ctx->parse_up, &ctx->parse_down}) {
    if (*st) (void)hipStreamDestroy(*st);
    *st = nullptr;
  }
}

static int parse_slots_ready(pcp_context *ctx, int64_t piece) {
  if (!ctx->parse_up) PCP_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->parse_up, hipStreamNonBlocking));
  if (!ctx->parse_down) PCP_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->parse_down, hipStreamNonBlocking));
  const size_t text_bytes = (static_cast<size_t>(piece) + 15) / 16 * 16 + 16;
  const size_t cap = static_cast<size_t>(piece_row_cap(piece));
  for (auto &s : ctx->parse_slot) {
    if (s.stage_bytes < static_cast<size_t>(piece)) {
      if (s.stage) (void)hipHostFree(s.stage);
      s.stage = nullptr;
      s.stage_bytes = 0;
      PCP_HIP_TRY(ctx, hipHostMalloc(&s.stage, static_cast<size_t>(piece), hipHostMallocDefault));
      s.stage_bytes = static_cast<size_t>(piece);
    }
    if (!s.res_h) PCP_HIP_TRY(ctx, hipHostMalloc(&s.res_h, sizeof(ParseResult), hipHostMallocDefault));
    PCP_HIP_TRY(ctx, s.text.ensure(text_bytes));
    PCP_HIP_TRY(ctx, s.end.ensure(cap));
    PCP_HIP_TRY(ctx, s.tiles.ensure(static_cast<size_t>(div_up(piece, kPaTextTile)) + 1));
    PCP_HIP_TRY(ctx, s.out.ensure(4 * cap));
    PCP_HIP_TRY(ctx, s.res.ensure(sizeof(ParseResult) / sizeof(unsigned long long)));
    for (hipEvent_t *e : {&s.staged, &s.parsed, &s.drained})
      if (!*e) PCP_HIP_TRY(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
    s.staged_live = s.parsed_live = s.drained_live = false;
  }
  return PCP_OK;
}

struct Piece {
  int64_t begin = 0, bytes = 0;  // of the window
  int64_t whole = 0;             // bytes consumed when every row of the piece is taken
  int64_t next = 0;              // where the piece behind it starts (the window's end behind the last piece)
  int32_t tail_row = 0;          // the bytes after the last '\n' are a row (final window, last piece, a non-blank byte)
  int64_t cap = 0;
};

// upload and kernels of one piece, queued; nothing waits on the host except for the slot's staging buffer
static int parse_issue(pcp_context *ctx, AsciiParseSlot &s, const char *text, const Piece &p, const ascii::RowCols &rc) {
  if (s.staged_live) PCP_HIP_TRY(ctx, hipEventSynchronize(s.staged));  // the upload that read the staging buffer last
  std::memcpy(s.stage, text + p.begin, static_cast<size_t>(p.bytes));
  if (s.parsed_live) PCP_HIP_TRY(ctx, hipStreamWaitEvent(ctx->parse_up, s.parsed, 0));  // the kernels that read the text buffer last
  PCP_HIP_TRY(ctx, hipMemcpyAsync(s.text.p, s.stage, static_cast<size_t>(p.bytes), hipMemcpyHostToDevice, ctx->parse_up));
  PCP_HIP_TRY(ctx, hipEventRecord(s.staged, ctx->parse_up));
  s.staged_live = true;
  PCP_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s.staged, 0));
  if (s.drained_live) PCP_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s.drained, 0));  // the download that read the outputs last
  ParseResult *res = reinterpret_cast<ParseResult *>(s.res.p);
  PCP_HIP_TRY(ctx, hipMemsetAsync(res, 0xff, sizeof(ParseResult), ctx->stream));
  {
    LaunchTimer t(ctx, PCP_K_MISC);
    const int64_t tiles = div_up(p.bytes, kPaTextTile);
    const uint32_t grid = static_cast<uint32_t>(std::min<int64_t>(tiles, 1 << 16));
    hipLaunchKernelGGL(k_parse_count, dim3(grid), dim3(kPaBlock), 0, ctx->stream, s.text.p, p.bytes, s.tiles.p);
    hipLaunchKernelGGL(k_scan_tile_offsets, dim3(1), dim3(kScanSingle), 0, ctx->stream, s.tiles.p, tiles, &res->newlines);
    hipLaunchKernelGGL(k_parse_index, dim3(grid), dim3(kPaBlock), 0, ctx->stream, s.text.p, p.bytes, s.tiles.p, s.end.p, p.cap);
    // the row count is known on the device only: a grid for the densest text the cap allows, walked with the grid's stride
    const uint32_t row_grid = static_cast<uint32_t>(std::min<int64_t>(div_up(p.cap, kPaBlock), 4096));
    hipLaunchKernelGGL(k_parse_rows, dim3(row_grid), dim3(kPaBlock), 0, ctx->stream, s.text.p, static_cast<int32_t>(p.bytes), s.end.p, res,
                       p.tail_row, p.cap, rc, s.out.p);
    PCP_HIP_TRY(ctx, hipGetLastError());
  }
  PCP_HIP_TRY(ctx, hipMemcpyAsync(s.res_h, res, sizeof(ParseResult), hipMemcpyDeviceToHost, ctx->stream));
  PCP_HIP_TRY(ctx, hipEventRecord(s.parsed, ctx->stream));
  s.parsed_live = true;
  return PCP_OK;
}

struct ParseTotals {
  int64_t rows = 0, consumed = 0, bad_row = -1;
  bool stop = false;
};

// the results of an issued piece: its rows go to the caller's arrays (queued on the download stream)
static int parse_retire(pcp_context *ctx, AsciiParseSlot &s, const Piece &p, int64_t max_rows, float *const out[4], ParseTotals *t) {
  PCP_HIP_TRY(ctx, hipEventSynchronize(s.parsed));
  const ParseResult res = *static_cast<const ParseResult *>(s.res_h);
  const int64_t rows = static_cast<int64_t>(res.newlines) + p.tail_row;
  const int64_t parsed = std::min(rows, p.cap);
  const int64_t bad = res.bad == 0xffffffffu ? -1 : static_cast<int64_t>(res.bad);
  if (rows > p.cap && bad < 0)
    return set_error(ctx, PCP_ERR_DEVICE, "pcp_ascii_parse: %lld rows in a piece of %lld bytes and none of them bad", static_cast<long long>(rows),
                     static_cast<long long>(p.bytes));
  int64_t take = std::min(parsed, max_rows - t->rows);
  if (bad >= 0 && bad < take) {
    take = bad;
    t->bad_row = t->rows + bad;
    t->stop = true;
  }
  if (take > 0) {
    for (int c = 0; c < 4; ++c)
      PCP_HIP_TRY(ctx, hipMemcpyAsync(out[c] + t->rows, s.out.p + static_cast<size_t>(c) * static_cast<size_t>(p.cap),
                                      static_cast<size_t>(take) * 4, hipMemcpyDeviceToHost, ctx->parse_down));
  }
  if (take == rows) {
    t->consumed = p.begin + p.whole;
  } else {  // the parse ends inside this piece: at the start of row `take`
    int32_t last_end = -1;
    if (take > 0) PCP_HIP_TRY(ctx, hipMemcpyAsync(&last_end, s.end.p + (take - 1), 4, hipMemcpyDeviceToHost, ctx->parse_down));
    PCP_HIP_TRY(ctx, hipStreamSynchronize(ctx->parse_down));
    t->consumed = p.begin + last_end + 1;
    t->stop = true;
  }
  PCP_HIP_TRY(ctx, hipEventRecord(s.drained, ctx->parse_down));
  s.drained_live = true;
  t->rows += take;
  if (t->rows >= max_rows) t->stop = true;
  return PCP_OK;
}

// the next piece of the window from `at`: up to kParsePiece bytes, cut after its last '\n'.  false: no '\n' in a full piece's
// reach (a row above the limit starts at `at`).
static bool next_piece(const char *text, int64_t bytes, int64_t at, int32_t final_window, Piece *p) {
  p->begin = at;
  p->tail_row = 0;
  const int64_t reach = std::min(kParsePiece, bytes - at);
  const bool last = at + reach == bytes;
  int64_t cut = reach;  // one past the last '\n'
  while (cut > 0 && text[at + cut - 1] != '\n') --cut;
  if (!last) {
    if (cut == 0) return false;
    p->bytes = p->whole = cut;
    p->next = at + cut;
  } else {
    p->next = bytes;
    bool tail = false;
    for (int64_t k = cut; k < reach && !tail; ++k) tail = !ascii::is_blank(static_cast<uint8_t>(text[at + k]));
    if (final_window && tail) {
      p->bytes = p->whole = reach;
      p->tail_row = 1;
    } else {
      p->bytes = p->whole = cut;
    }
  }
  p->cap = piece_row_cap(p->bytes);
  return true;
}

static const char *parse_args_problem(const char *text, int64_t bytes, int32_t columns, const int32_t col[4], int64_t max_rows, float *out_x,
                                      float *out_y, float *out_z, float *out_intensity, int64_t *out_rows, int64_t *out_consumed,
                                      int64_t *out_bad_row) {
  if (!out_rows || !out_consumed || !out_bad_row) return "out_rows / out_consumed / out_bad_row is NULL";
  if (bytes < 0) return "negative bytes";
  if (max_rows < 0) return "negative max_rows";
  if (columns < 1 || columns > 64) return "columns outside 1..64";
  if (!col) return "col is NULL";
  for (int c = 0; c < 4; ++c)
    if (col[c] >= columns || col[c] < (c == 3 ? -1 : 0)) return "a col entry outside the row (only the intensity may be -1)";
  if (bytes > 0 && !text) return "text is NULL";
  if (max_rows > 0 && (!out_x || !out_y || !out_z || !out_intensity)) return "an output array is NULL";
  return nullptr;
}

}  // namespace pcp

using namespace pcp;

extern "C" {

int64_t pcp_ascii_parse_limit(int32_t which) {
  switch (which) {
    case PCP_PARSE_LIMIT_ROW: return ascii::kParseMaxRow;
    case PCP_PARSE_LIMIT_TILE: return kParseTile;
    case PCP_PARSE_LIMIT_PIECE: return kParsePiece;
    case PCP_PARSE_LIMIT_TILE_ROWS: return kPaBlock;
    case PCP_PARSE_LIMIT_WINDOW: return kParseWindowMax;
    default: return -1;
  }
}

int pcp_ascii_parse_host(const char *text, int64_t bytes, int32_t columns, const int32_t col[4], int32_t final_window, int64_t max_rows,
                         float *out_x, float *out_y, float *out_z, float *out_intensity, int64_t *out_rows, int64_t *out_consumed,
                         int64_t *out_bad_row) {
  if (const char *why = parse_args_problem(text, bytes, columns, col, max_rows, out_x, out_y, out_z, out_intensity, out_rows, out_consumed,
                                           out_bad_row)) {
    set_global_error("pcp_ascii_parse_host: %s", why);
    return PCP_ERR_INVALID;
  }
  *out_rows = 0;
  *out_consumed = 0;
  *out_bad_row = -1;
  if (bytes > kParseWindowMax) {
    set_global_error("pcp_ascii_parse_host: a window of %lld bytes (the limit is 2^31 - 1)", static_cast<long long>(bytes));
    return PCP_ERR_RANGE;
  }
  const ascii::RowCols rc{columns, {col[0], col[1], col[2], col[3]}};
  ascii::parse_window(text, static_cast<int32_t>(bytes), rc, final_window != 0, max_rows, reinterpret_cast<uint32_t *>(out_x),
                      reinterpret_cast<uint32_t *>(out_y), reinterpret_cast<uint32_t *>(out_z), reinterpret_cast<uint32_t *>(out_intensity),
                      out_rows, out_consumed, out_bad_row);
  return PCP_OK;
}

int pcp_ascii_parse(pcp_context *ctx, const char *text, int64_t bytes, int32_t columns, const int32_t col[4], int32_t final_window,
                    int64_t max_rows, float *out_x, float *out_y, float *out_z, float *out_intensity, int64_t *out_rows,
                    int64_t *out_consumed, int64_t *out_bad_row) {
  if (!ctx) return PCP_ERR_INVALID;
  if (const char *why = parse_args_problem(text, bytes, columns, col, max_rows, out_x, out_y, out_z, out_intensity, out_rows, out_consumed,
                                           out_bad_row))
    return set_error(ctx, PCP_ERR_INVALID, "pcp_ascii_parse: %s", why);
  *out_rows = 0;
  *out_consumed = 0;
  *out_bad_row = -1;
  if (bytes > kParseWindowMax)
    return set_error(ctx, PCP_ERR_RANGE, "pcp_ascii_parse: a window of %lld bytes (the limit is 2^31 - 1)", static_cast<long long>(bytes));
  if (bytes == 0 || max_rows == 0) return PCP_OK;
  PCP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc_ = parse_slots_ready(ctx, std::min(bytes, kParsePiece));
  if (rc_ != PCP_OK) return rc_;
  const ascii::RowCols rc{columns, {col[0], col[1], col[2], col[3]}};
  float *const out[4] = {out_x, out_y, out_z, out_intensity};
  ParseTotals t;
  Piece piece[2];
  bool pending = false, more = true;  // pending: piece[(k - 1) & 1] is issued and not retired; more: text left to cut
  int64_t at = 0;
  int rc2 = PCP_OK;
  for (int k = 0;; ++k) {
    bool issued = false, long_row = false;
    if (more && !t.stop) {
      Piece &p = piece[k & 1];
      if (!next_piece(text, bytes, at, final_window, &p)) {
        long_row = true;
        more = false;
      } else {
        if (p.bytes > 0) {
          rc2 = parse_issue(ctx, ctx->parse_slot[k & 1], text, p, rc);
          if (rc2 != PCP_OK) break;
          issued = true;
        }
        at = p.next;
        more = at < bytes;
      }
    }
    if (pending && !t.stop) {  // (a piece issued behind the one that ended the parse is dropped)
      rc2 = parse_retire(ctx, ctx->parse_slot[(k - 1) & 1], piece[(k - 1) & 1], max_rows, out, &t);
      if (rc2 != PCP_OK) break;
    }
    pending = issued;
    if (long_row && !t.stop) {  // every piece in front is retired: the row that starts at `at` has no '\n' within a piece
      t.bad_row = t.rows;
      t.consumed = at;
      t.stop = true;
    }
    if (!pending) break;
  }
  // nothing of this call is left in flight
  hipError_t e0 = hipStreamSynchronize(ctx->parse_up), e1 = hipStreamSynchronize(ctx->stream), e2 = hipStreamSynchronize(ctx->parse_down);
  if (rc2 != PCP_OK) return rc2;
  PCP_HIP_TRY(ctx, e0);
  PCP_HIP_TRY(ctx, e1);
  PCP_HIP_TRY(ctx, e2);
  *out_rows = t.rows;
  *out_consumed = t.consumed;
  *out_bad_row = t.bad_row;
  return PCP_OK;
}

}  // extern "C"
