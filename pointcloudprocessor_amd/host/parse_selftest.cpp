// parse_selftest -- the PCD ASCII parser of csrc/pcp_ascii_parse.hpp, compiled for the host, over adversarial windows: every
// prefix of a 3-row text, rows of only blanks, a token cut at the window's end, a 5 000-byte row, windows that end in 'e', '-'
// or '.', random bytes and random tokens.  Every window lies at the very end of a mapping whose next page is inaccessible, so a
// read past it is a fault (and a report under -fsanitize=address).  The values are compared with strtof, the row rules (DESIGN.md
// "Device PCD reader", DR1-DR5) with a plain reference written here.  Exit code 0 iff everything agrees.
// usage: parse_selftest [random windows]
#include <sys/mman.h>
#include <unistd.h>

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/pcp_ascii_parse.hpp"

namespace pa = pcp::ascii;

static uint64_t mix(uint64_t v) {
  v += 0x9e3779b97f4a7c15ull;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}

// a window copied to the end of a mapping in front of a PROT_NONE page
struct Guarded {
  char *base = nullptr;
  size_t span = 0, page = 0;
  explicit Guarded(size_t capacity) {
    page = static_cast<size_t>(sysconf(_SC_PAGESIZE));
    span = (capacity + page - 1) / page * page + page;
    base = static_cast<char *>(mmap(nullptr, span, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
    if (base == MAP_FAILED || mprotect(base + span - page, page, PROT_NONE) != 0) {
      std::perror("mmap");
      std::exit(2);
    }
  }
  ~Guarded() { munmap(base, span); }
  const char *place(const std::string &w) const {
    char *p = base + span - page - w.size();
    std::memcpy(p, w.data(), w.size());
    return p;
  }
};

static bool blank(unsigned char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// DR3 by a plain reading of the grammar
static bool ref_token_ok(const std::string &t) {
  size_t i = 0;
  if (i < t.size() && (t[i] == '+' || t[i] == '-')) ++i;
  std::string low;
  for (size_t k = i; k < t.size(); ++k) low += static_cast<char>(std::tolower(static_cast<unsigned char>(t[k])));
  if (low == "nan" || low == "inf" || low == "infinity") return true;
  std::string digits;
  size_t ni = 0, nf = 0;
  while (i < t.size() && std::isdigit(static_cast<unsigned char>(t[i]))) digits += t[i++], ++ni;
  if (i < t.size() && t[i] == '.') {
    ++i;
    while (i < t.size() && std::isdigit(static_cast<unsigned char>(t[i]))) digits += t[i++], ++nf;
  }
  if (ni + nf == 0) return false;
  const size_t first = digits.find_first_not_of('0'), last = digits.find_last_not_of('0');
  if (first != std::string::npos && last - first + 1 > 19) return false;
  if (i == t.size()) return true;
  if (t[i] != 'e' && t[i] != 'E') return false;
  ++i;
  if (i < t.size() && (t[i] == '+' || t[i] == '-')) ++i;
  size_t ne = 0;
  while (i < t.size() && std::isdigit(static_cast<unsigned char>(t[i]))) ++i, ++ne;
  return ne >= 1 && ne <= 5 && i == t.size();
}

struct Expect {
  std::vector<uint32_t> v[4];
  int64_t rows = 0, consumed = 0, bad = -1;
};

static uint32_t strtof_bits(const std::string &t) {
  const float f = std::strtof(t.c_str(), nullptr);
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

static Expect reference(const std::string &w, const pa::RowCols &rc, bool final_window, int64_t max_rows) {
  Expect x;
  size_t pos = 0;
  while (x.rows < max_rows && pos < w.size()) {
    size_t e = w.find('\n', pos);
    if (e == std::string::npos) {
      if (!final_window) break;
      bool any = false;
      for (size_t k = pos; k < w.size(); ++k) any = any || !blank(static_cast<unsigned char>(w[k]));
      if (!any) break;
      e = w.size();
    }
    std::vector<std::string> tok;
    for (size_t i = pos; i < e;) {
      while (i < e && blank(static_cast<unsigned char>(w[i]))) ++i;
      size_t j = i;
      while (j < e && !blank(static_cast<unsigned char>(w[j]))) ++j;
      if (j > i) tok.push_back(w.substr(i, j - i));
      i = j;
    }
    bool ok = static_cast<int64_t>(e - pos) <= pa::kParseMaxRow && static_cast<int32_t>(tok.size()) >= rc.columns;
    uint32_t v[4] = {0, 0, 0, 0};
    for (int c = 0; ok && c < 4; ++c) {
      if (rc.c[c] < 0) continue;
      const std::string &t = tok[static_cast<size_t>(rc.c[c])];
      ok = t.find('\0') == std::string::npos && ref_token_ok(t);
      if (ok) v[c] = strtof_bits(t);
    }
    if (!ok) {
      x.bad = x.rows;
      break;
    }
    for (int c = 0; c < 4; ++c) x.v[c].push_back(v[c]);
    ++x.rows;
    pos = e < w.size() ? e + 1 : w.size();
  }
  x.consumed = static_cast<int64_t>(pos);
  return x;
}

static uint64_t g_checks = 0, g_bad = 0;

static void check(const Guarded &g, const std::string &w, const pa::RowCols &rc, bool final_window, int64_t max_rows, const char *what) {
  const Expect want = reference(w, rc, final_window, max_rows);
  const size_t cap = static_cast<size_t>(max_rows) + 1;
  std::vector<uint32_t> o[4];
  for (auto &a : o) a.assign(cap, 0xA5A5A5A5u);
  int64_t rows = -2, consumed = -2, bad = -2;
  pa::parse_window(g.place(w), static_cast<int32_t>(w.size()), rc, final_window, max_rows, o[0].data(), o[1].data(), o[2].data(),
                   o[3].data(), &rows, &consumed, &bad);
  bool ok = rows == want.rows && consumed == want.consumed && bad == want.bad;
  for (int c = 0; ok && c < 4; ++c) {
    for (int64_t r = 0; ok && r < rows; ++r) ok = o[c][static_cast<size_t>(r)] == want.v[c][static_cast<size_t>(r)];
    for (size_t r = static_cast<size_t>(rows); ok && r < cap; ++r) ok = o[c][r] == 0xA5A5A5A5u;
  }
  ++g_checks;
  if (!ok) {
    if (g_bad < 10)
      std::fprintf(stderr, "%s: window of %zu bytes (final %d, max_rows %lld): rows %lld / %lld, consumed %lld / %lld, bad %lld / %lld\n", what,
                   w.size(), final_window ? 1 : 0, static_cast<long long>(max_rows), static_cast<long long>(rows),
                   static_cast<long long>(want.rows), static_cast<long long>(consumed), static_cast<long long>(want.consumed),
                   static_cast<long long>(bad), static_cast<long long>(want.bad));
    ++g_bad;
  }
}

int main(int argc, char **argv) {
  const uint64_t count = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 20000ull;
  Guarded g(size_t(1) << 17);
  const pa::RowCols xyzi{4, {0, 1, 2, 3}}, xyz{3, {0, 1, 2, -1}}, perm{5, {1, 2, 4, 0}};
  const std::string three = "1.5 -2.25 3e2 0.125\n  7\t8.0625  9. .5 junk\r\n-0 1e-46 3.4028236e38 nan\n";
  for (size_t n = 0; n <= three.size(); ++n)
    for (int fin = 0; fin < 2; ++fin) {
      check(g, three.substr(0, n), xyzi, fin != 0, 8, "prefix");
      check(g, three.substr(0, n), xyz, fin != 0, 2, "prefix, max_rows 2");
      check(g, three.substr(n), xyzi, fin != 0, 8, "suffix");
    }
  for (const char *w : {"", "\n", " \t\r\n", "   ", "\n\n\n", "1 2 3 4\n \n5 6 7 8\n", "1 2 3 4\n\v\f", "1 2 3\n", "1 2 3 4"})
    for (int fin = 0; fin < 2; ++fin) check(g, w, xyzi, fin != 0, 8, "blanks");
  for (const char *tail : {"e", "-", ".", "+", "1e", "1e-", "1.", "-.", "E5", "in", "na", "infinit", "0x", "1,5"})
    for (int fin = 0; fin < 2; ++fin) {
      check(g, std::string("1 2 3 4\n5 6 7 ") + tail, xyzi, fin != 0, 8, "cut token");
      check(g, std::string("1 2 3 ") + tail + "\n", xyzi, fin != 0, 8, "short token");
      check(g, tail, pa::RowCols{1, {0, 0, 0, -1}}, fin != 0, 8, "token alone");
    }
  {  // a 5 000-byte row: blanks, unread junk columns, then the values; and rows around the length limit
    std::string row = "1.25 " + std::string(2400, ' ') + std::string(2500, 'x') + " -7.5 1e10 \t 4\n";
    row.insert(5, std::string(5000 - row.size(), '\t'));
    check(g, "0 0 0 0 0\n" + row + "1 1 1 1 1\n", perm, true, 8, "5000-byte row");
    for (int32_t extra = -1; extra <= 1; ++extra) {
      const std::string pad(static_cast<size_t>(pa::kParseMaxRow + extra - 7), ' ');
      check(g, "9 9 9 9\n" + pad + "1 2 3 4\n5 6 7 8\n", xyzi, true, 8, "row length limit");
    }
  }
  // random bytes (weighted towards the bytes that matter) and random decimal tokens
  const char alphabet[] = "0123456789.eE+-\n\n \t\rnaNiIfx,\0\xff";
  for (uint64_t it = 0; it < count; ++it) {
    uint64_t r = mix(it);
    std::string w;
    const size_t len = static_cast<size_t>(r % 97);
    for (size_t k = 0; k < len; ++k) {
      r = mix(r);
      w += (r & 7u) ? alphabet[(r >> 8) % (sizeof(alphabet) - 1)] : static_cast<char>(r >> 16);
    }
    check(g, w, (it & 1u) ? xyz : pa::RowCols{1, {0, 0, 0, -1}}, (it & 2u) != 0, 1 + static_cast<int64_t>((r >> 40) % 6), "random bytes");
    // rows of random tokens: 1 - 19 digits, a point anywhere, exponents -70 .. 50
    std::string rows;
    for (int t = 0; t < 8; ++t) {
      r = mix(r);
      const int nd = 1 + static_cast<int>(r % 19), point = static_cast<int>((r >> 8) % static_cast<uint64_t>(nd + 2)) - 1;
      if ((r >> 20) & 1u) rows += '-';
      for (int d = 0; d < nd; ++d) {
        if (d == point) rows += '.';
        r = mix(r);
        rows += static_cast<char>('0' + r % 10);
      }
      if (point == nd) rows += '.';
      r = mix(r);
      if (r & 3u) rows += "e" + std::to_string(static_cast<int>((r >> 4) % 121) - 70);
      rows += (t & 3) == 3 ? "\n" : " ";
    }
    check(g, rows, xyzi, true, 4, "random tokens");
  }
  std::printf("%llu windows, %llu mismatches\n", static_cast<unsigned long long>(g_checks), static_cast<unsigned long long>(g_bad));
  return g_bad ? 1 : 0;
}
