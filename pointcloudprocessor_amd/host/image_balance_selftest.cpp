// image_balance_selftest -- csrc/pcp_image_balance.hpp compiled for the CPU (no GPU, no library): the arithmetic the kernels and
// pcp_image_balance_host share, driven the way they drive it (reflected indices, closed-form redistribution, one pass per
// tile), against a brute-force form written differently: a materialised padded copy of V, per-tile loops over it, the serial
// redistribution walk exactly as DESIGN.md's IB5 writes it, and the interpolation spelled out per pixel.
//
//   image_balance_selftest [rounds]     prints "<cases> cases, <n> mismatches"; exit status 0 iff n == 0
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pcp_image_balance.hpp"

namespace ib = pcp::ib;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return static_cast<uint32_t>(g_state >> 16);
}

struct Image {
  int w, h;
  std::vector<uint8_t> bgr;
};

static Image make_image(int w, int h, int kind) {
  Image im{w, h, std::vector<uint8_t>(static_cast<size_t>(w) * h * 3)};
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      uint8_t *p = &im.bgr[(static_cast<size_t>(y) * w + x) * 3];
      switch (kind) {
        case 0: p[0] = rnd() & 255; p[1] = rnd() & 255; p[2] = rnd() & 255; break;           // noise
        case 1: p[0] = static_cast<uint8_t>(x * 255 / (w > 1 ? w - 1 : 1)); p[1] = p[0] / 2; p[2] = p[0] / 3; break;  // ramp
        case 2: p[0] = 40; p[1] = 97; p[2] = 60; break;                                      // constant
        case 3: p[0] = p[1] = p[2] = (rnd() % 10 < 3) ? 255 : 0; break;                      // two levels
        default: {                                                                           // dark with a saturated blob
          const bool in = (x - w / 2) * (x - w / 2) + (y - h / 2) * (y - h / 2) < (w < h ? w : h) * (w < h ? w : h) / 16;
          p[0] = p[1] = p[2] = in ? 255 : static_cast<uint8_t>(rnd() % 30);
        }
      }
    }
  return im;
}

// the header's way: what pcp_image_balance_host does
static void header_form(const Image &im, int tx_n, int ty_n, float clip_limit, const uint8_t *gamma, const int32_t *sdiv,
                        const int32_t *hdiv, std::vector<uint32_t> &hist, std::vector<uint8_t> &lut, std::vector<uint8_t> &out) {
  ib::Grid g;
  if (ib::make_grid(im.w, im.h, tx_n, ty_n, &g) != 0) std::abort();
  const int tiles = tx_n * ty_n, clip = ib::clip_count(clip_limit, g.total);
  hist.assign(static_cast<size_t>(tiles) * 256, 0);
  lut.assign(static_cast<size_t>(tiles) * 256, 0);
  for (int t = 0; t < tiles; ++t) {
    const int ty = t / tx_n, tx = t % tx_n;
    for (int p = 0; p < g.total; ++p) {
      const int row = p / g.tw, col = p % g.tw;
      const uint8_t *px = &im.bgr[(static_cast<size_t>(ib::reflect101(ty * g.th + row, im.h)) * im.w + ib::reflect101(tx * g.tw + col, im.w)) * 3];
      uint8_t v = px[0] > px[1] ? px[0] : px[1];
      v = v > px[2] ? v : px[2];
      ++hist[static_cast<size_t>(t) * 256 + v];
    }
    int32_t clipped = 0;
    for (int i = 0; i < 256; ++i) clipped += ib::excess(static_cast<int32_t>(hist[static_cast<size_t>(t) * 256 + i]), clip);
    int32_t cum = 0;
    for (int i = 0; i < 256; ++i) {
      cum += ib::redistributed(static_cast<int32_t>(hist[static_cast<size_t>(t) * 256 + i]), i, clip, clipped);
      lut[static_cast<size_t>(t) * 256 + i] = static_cast<uint8_t>(ib::lut_entry(cum, g.lut_scale));
    }
  }
  out.resize(im.bgr.size());
  for (int y = 0; y < im.h; ++y) {
    const ib::Weights wy = ib::weights(y, g.inv_th, ty_n);
    for (int x = 0; x < im.w; ++x) {
      const size_t at = (static_cast<size_t>(y) * im.w + x) * 3;
      uint32_t b = im.bgr[at], gg = im.bgr[at + 1], r = im.bgr[at + 2], H, S, V;
      pcp::hsv_forward(sdiv, hdiv, b, gg, r, H, S, V);
      const ib::Weights wx = ib::weights(x, g.inv_tw, tx_n);
      pcp::hsv_backward(H, S, ib::lookup4(lut.data(), tx_n, wx, wy, V), b, gg, r);
      out[at] = gamma[b];
      out[at + 1] = gamma[gg];
      out[at + 2] = gamma[r];
    }
  }
}

// the brute-force way
static void brute_form(const Image &im, int tx_n, int ty_n, float clip_limit, const uint8_t *gamma, const int32_t *sdiv,
                       const int32_t *hdiv, std::vector<uint32_t> &hist, std::vector<uint8_t> &lut, std::vector<uint8_t> &out) {
  int ex = 0, ey = 0;
  if (im.w % tx_n != 0 || im.h % ty_n != 0) {
    ex = tx_n - im.w % tx_n;
    ey = ty_n - im.h % ty_n;
  }
  const int W = im.w + ex, Hh = im.h + ey, tw = W / tx_n, th = Hh / ty_n, total = tw * th;
  std::vector<uint8_t> V(static_cast<size_t>(W) * Hh);  // the padded V plane, materialised
  for (int y = 0; y < Hh; ++y)
    for (int x = 0; x < W; ++x) {
      const int sx = x < im.w ? x : 2 * (im.w - 1) - x, sy = y < im.h ? y : 2 * (im.h - 1) - y;
      const uint8_t *p = &im.bgr[(static_cast<size_t>(sy) * im.w + sx) * 3];
      uint8_t v = p[0];
      if (p[1] > v) v = p[1];
      if (p[2] > v) v = p[2];
      V[static_cast<size_t>(y) * W + x] = v;
    }
  hist.assign(static_cast<size_t>(tx_n) * ty_n * 256, 0);
  lut.assign(static_cast<size_t>(tx_n) * ty_n * 256, 0);
  const float lut_scale = 255.0f / static_cast<float>(total);
  for (int ty = 0; ty < ty_n; ++ty)
    for (int tx = 0; tx < tx_n; ++tx) {
      int h[256] = {};
      for (int y = ty * th; y < (ty + 1) * th; ++y)
        for (int x = tx * tw; x < (tx + 1) * tw; ++x) ++h[V[static_cast<size_t>(y) * W + x]];
      uint32_t *raw = &hist[(static_cast<size_t>(ty) * tx_n + tx) * 256];
      for (int i = 0; i < 256; ++i) raw[i] = static_cast<uint32_t>(h[i]);
      if (clip_limit > 0) {
        int clip = static_cast<int>(static_cast<double>(clip_limit) * total / 256);
        if (clip < 1) clip = 1;
        int clipped = 0;
        for (int i = 0; i < 256; ++i)
          if (h[i] > clip) {
            clipped += h[i] - clip;
            h[i] = clip;
          }
        const int batch = clipped / 256;
        int residual = clipped - batch * 256;
        for (int i = 0; i < 256; ++i) h[i] += batch;
        if (residual != 0) {
          const int step = 256 / residual > 1 ? 256 / residual : 1;
          for (int i = 0; i < 256 && residual > 0; i += step, --residual) ++h[i];
        }
      }
      int sum = 0;
      uint8_t *l = &lut[(static_cast<size_t>(ty) * tx_n + tx) * 256];
      for (int i = 0; i < 256; ++i) {
        sum += h[i];
        const float s = static_cast<float>(sum) * lut_scale;
        const float rr = __builtin_rintf(s);
        l[i] = static_cast<uint8_t>(rr < 0.0f ? 0 : (rr > 255.0f ? 255 : static_cast<int>(rr)));
      }
    }
  out.resize(im.bgr.size());
  const float inv_tw = 1.0f / static_cast<float>(tw), inv_th = 1.0f / static_cast<float>(th);
  for (int y = 0; y < im.h; ++y)
    for (int x = 0; x < im.w; ++x) {
      const float txf = static_cast<float>(x) * inv_tw - 0.5f, tyf = static_cast<float>(y) * inv_th - 0.5f;
      int tx1 = static_cast<int>(__builtin_floorf(txf)), ty1 = static_cast<int>(__builtin_floorf(tyf));
      const float xa = txf - static_cast<float>(tx1), ya = tyf - static_cast<float>(ty1);
      const float xa1 = 1.0f - xa, ya1 = 1.0f - ya;
      int tx2 = tx1 + 1, ty2 = ty1 + 1;
      if (tx1 < 0) tx1 = 0;
      if (ty1 < 0) ty1 = 0;
      if (tx2 > tx_n - 1) tx2 = tx_n - 1;
      if (ty2 > ty_n - 1) ty2 = ty_n - 1;
      const size_t at = (static_cast<size_t>(y) * im.w + x) * 3;
      uint32_t b = im.bgr[at], gg = im.bgr[at + 1], r = im.bgr[at + 2], H, S, v;
      pcp::hsv_forward(sdiv, hdiv, b, gg, r, H, S, v);
      const float l11 = lut[(static_cast<size_t>(ty1) * tx_n + tx1) * 256 + v], l12 = lut[(static_cast<size_t>(ty1) * tx_n + tx2) * 256 + v];
      const float l21 = lut[(static_cast<size_t>(ty2) * tx_n + tx1) * 256 + v], l22 = lut[(static_cast<size_t>(ty2) * tx_n + tx2) * 256 + v];
      const float a = l11 * xa1, bq = l12 * xa, top = a + bq;
      const float c = l21 * xa1, d = l22 * xa, bottom = c + d;
      const float e = top * ya1, f = bottom * ya, res = e + f;
      const float rr = __builtin_rintf(res);
      const uint32_t v2 = rr < 0.0f ? 0u : (rr > 255.0f ? 255u : static_cast<uint32_t>(rr));
      pcp::hsv_backward(H, S, v2, b, gg, r);
      out[at] = gamma[b];
      out[at + 1] = gamma[gg];
      out[at + 2] = gamma[r];
    }
}

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 2;
  int32_t sdiv[256], hdiv[256];
  pcp::hsv_build_tables(sdiv, hdiv);
  static const int shapes[][4] = {{64, 48, 8, 8}, {70, 50, 8, 8}, {64, 50, 8, 8}, {48, 36, 1, 1}, {90, 60, 3, 5}, {128, 128, 16, 16},
                                  {33, 17, 16, 16}, {9, 9, 8, 8}, {200, 150, 2, 2}};
  static const float clips[] = {0.0f, 1.0f, 3.0f, 40.0f};
  static const float gammas[] = {0.8f, 1.0f, 1.1f};
  long cases = 0, bad = 0;
  // the refusals of IB3 and the gamma table's fixed points
  ib::Grid g;
  if (ib::make_grid(8, 9, 8, 8, &g) != 2 || ib::make_grid(4, 4, 8, 8, &g) != 2 || ib::make_grid(64, 48, 17, 8, &g) != 1 ||
      ib::make_grid(64, 48, 8, 0, &g) != 1 || ib::make_grid(64, 50, 8, 8, &g) != 0 || g.tw != 9 || g.th != 7) {
    std::printf("make_grid: wrong refusal or size\n");
    ++bad;
  }
  uint8_t ident[256];
  ib::gamma_table(1.0f, ident);
  for (int i = 0; i < 256; ++i)
    if (ident[i] != i) ++bad;
  for (int round = 0; round < rounds; ++round)
    for (const auto &s : shapes)
      for (int kind = 0; kind < 5; ++kind) {
        const Image im = make_image(s[0], s[1], kind);
        for (float clip : clips) {
          uint8_t gamma[256];
          ib::gamma_table(gammas[cases % 3], gamma);
          std::vector<uint32_t> h1, h2;
          std::vector<uint8_t> l1, l2, o1, o2;
          header_form(im, s[2], s[3], clip, gamma, sdiv, hdiv, h1, l1, o1);
          brute_form(im, s[2], s[3], clip, gamma, sdiv, hdiv, h2, l2, o2);
          ++cases;
          if (h1 != h2 || l1 != l2 || o1 != o2) {
            ++bad;
            std::printf("mismatch: %dx%d tiles %dx%d image %d clip %g: hist %d lut %d pixels %d\n", s[0], s[1], s[2], s[3], kind, clip,
                        h1 != h2, l1 != l2, o1 != o2);
          }
        }
      }
  std::printf("%ld cases, %ld mismatches\n", cases, bad);
  return bad == 0 ? 0 : 1;
}
