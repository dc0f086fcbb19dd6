// pcp_ascii_parse.hpp -- the floats of a PCD ASCII row, for host and device alike ("Device PCD reader", DR1-DR8):
// the mirror image of pcp_ascii.hpp.  parse_token turns one token into the bits glibc's strtof returns for it, or refuses it;
// parse_row walks the tokens of one row; parse_window is the sequential (host) twin of the kernels in pcp_ascii_parse.hip.
// No libc, no tables, fixed-width integers only; host/pcd_io.hpp does NOT use this header (its strtof reader is the
// independent implementation the tests compare with).
//
// A token is sign, significand w < 10^19 (at most 19 digits between its first and last non-zero digit) and decimal exponent
// q: |v| = w * 10^q = w * 5^q * 2^q.  The fp32 nearest the exact value, ties to even, is taken on integers in one of four ways:
//   q >= 39 (w >= 1) is inf, q < -65 is 0 (w * 10^q < 10^-46 < 2^-150, half the smallest subnormal);
//   0 <= q, w * 5^q < 2^64    one 64-bit product (exact: bitlen(w) + bitlen(5^q) <= 64), rounded once;
//   -16 <= q < 0              one 64-bit division: w is shifted to the top of the word, 5^-q < 2^38, so the quotient has at
//                             least 26 bits (24 + round + one more) and the remainder is the exact sticky bit;
//   otherwise                 three 64-bit limbs: the product w * 5^q (< 2^152) for q > 0; for q < 0 a compare-and-subtract
//                             long division by 5^-q (< 2^151) with numerator or divisor shifted so that the quotient has 26
//                             or 27 bits, the remainder the sticky bit.
// The quotient (or the top 64 bits of the product) with its sticky bit goes through one rounding (round_pack) that knows
// subnormals, the carry into the next binade and the overflow to inf.  Nothing goes through a double.
#pragma once

#include <stdint.h>

#include "pcp_ascii.hpp"

namespace pcp {
namespace ascii {

// DR5: a row of more bytes than this in front of its '\n' is bad (PCP_ASCII_PARSE_MAX_ROW in pcp_hip.h)
constexpr int32_t kParseMaxRow = 65536;

// the C-locale blanks that are not the row terminator: space \t \v \f \r (what `istream >>` skips inside a getline'd row)
PCP_ASCII_HD bool is_blank(uint32_t c) { return c == 0x20u || c == 9u || (c >= 11u && c <= 13u); }

PCP_ASCII_HD int bitlen64(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// 5^k, k <= 27 (< 2^63)
PCP_ASCII_HD uint64_t pow5_64(int k) {
  uint64_t p = 1;
  if (k & 1) p *= 5u;
  if (k & 2) p *= 25u;
  if (k & 4) p *= 625u;
  if (k & 8) p *= 390625u;
  if (k & 16) p *= 152587890625ull;
  return p;
}

struct U192 {
  uint64_t l0, l1, l2;
};
PCP_ASCII_HD U192 u192(uint64_t v) {
  U192 r;
  r.l0 = v;
  r.l1 = 0;
  r.l2 = 0;
  return r;
}
// a << n, 0 <= n < 192 (the caller keeps the result below 2^192)
PCP_ASCII_HD U192 shl192(U192 a, int n) {
  if (n >= 128) {
    a.l2 = a.l0;
    a.l1 = 0;
    a.l0 = 0;
    n -= 128;
  } else if (n >= 64) {
    a.l2 = a.l1;
    a.l1 = a.l0;
    a.l0 = 0;
    n -= 64;
  }
  if (n) {
    a.l2 = (a.l2 << n) | (a.l1 >> (64 - n));
    a.l1 = (a.l1 << n) | (a.l0 >> (64 - n));
    a.l0 <<= n;
  }
  return a;
}
// a >> n, 0 <= n < 192; *sticky |= a bit was shifted out
PCP_ASCII_HD U192 shr192(U192 a, int n, bool *sticky) {
  if (n >= 128) {
    *sticky = *sticky || (a.l0 | a.l1) != 0;
    a.l0 = a.l2;
    a.l1 = 0;
    a.l2 = 0;
    n -= 128;
  } else if (n >= 64) {
    *sticky = *sticky || a.l0 != 0;
    a.l0 = a.l1;
    a.l1 = a.l2;
    a.l2 = 0;
    n -= 64;
  }
  if (n) {
    *sticky = *sticky || (a.l0 & low_mask(n)) != 0;
    a.l0 = (a.l0 >> n) | (a.l1 << (64 - n));
    a.l1 = (a.l1 >> n) | (a.l2 << (64 - n));
    a.l2 >>= n;
  }
  return a;
}
PCP_ASCII_HD U192 shr192_1(U192 a) {
  a.l0 = (a.l0 >> 1) | (a.l1 << 63);
  a.l1 = (a.l1 >> 1) | (a.l2 << 63);
  a.l2 >>= 1;
  return a;
}
PCP_ASCII_HD bool ge192(const U192 &a, const U192 &b) {
  if (a.l2 != b.l2) return a.l2 > b.l2;
  if (a.l1 != b.l1) return a.l1 > b.l1;
  return a.l0 >= b.l0;
}
// a - b, a >= b
PCP_ASCII_HD U192 sub192(const U192 &a, const U192 &b) {
  U192 r;
  r.l0 = a.l0 - b.l0;
  const uint64_t b0 = a.l0 < b.l0 ? 1u : 0u;
  r.l1 = a.l1 - b.l1 - b0;
  const uint64_t b1 = (a.l1 < b.l1 || (a.l1 == b.l1 && b0)) ? 1u : 0u;
  r.l2 = a.l2 - b.l2 - b1;
  return r;
}
PCP_ASCII_HD int bitlen192(const U192 &a) {
  if (a.l2) return 128 + bitlen64(a.l2);
  if (a.l1) return 64 + bitlen64(a.l1);
  return bitlen64(a.l0);
}
// a * 5^k, 27 powers of five at a time (the caller keeps the result below 2^192)
PCP_ASCII_HD U192 mul192_pow5(U192 a, int k) {
  for (int left = k; left > 0; left -= 27) {
    const uint64_t c = pow5_64(left > 27 ? 27 : left);
    u128 t = static_cast<u128>(a.l0) * c;
    a.l0 = static_cast<uint64_t>(t);
    t = static_cast<u128>(a.l1) * c + static_cast<uint64_t>(t >> 64);
    a.l1 = static_cast<uint64_t>(t);
    t = static_cast<u128>(a.l2) * c + static_cast<uint64_t>(t >> 64);
    a.l2 = static_cast<uint64_t>(t);
  }
  return a;
}

// The fp32 nearest (Q + d) * 2^e2, ties to even: Q > 0, 0 <= d < 1, d != 0 iff sticky.  A caller that passes sticky gives a Q
// of at least 26 bits, so the bits below the result's last place always hold the round bit and one more.
PCP_ASCII_HD uint32_t round_pack(bool neg, uint64_t Q, bool sticky, int e2) {
  const uint32_t sign = neg ? 0x80000000u : 0u;
  const int t = bitlen64(Q) - 1;
  const int E = t + e2;  // 2^E <= value < 2^(E + 1)
  if (E >= 128) return sign | 0x7f800000u;
  const bool normal = E >= -126;
  const int shift = normal ? t - 23 : -149 - e2;  // bits of Q below the last place of the result
  uint64_t m;
  if (shift <= 0) {
    m = Q << -shift;  // exact
  } else {
    if (shift > 64) return sign;  // below 2^-150
    uint64_t half, low;
    if (shift == 64) {
      m = 0;
      half = Q >> 63;
      low = Q & low_mask(63);
    } else {
      m = Q >> shift;
      half = (Q >> (shift - 1)) & 1u;
      low = Q & low_mask(shift - 1);
    }
    if (half && (sticky || low != 0 || (m & 1u))) ++m;
  }
  if (!normal) return sign | static_cast<uint32_t>(m);  // m <= 2^23: a carry out of the subnormals is the smallest normal
  // m in [2^23, 2^24]: the hidden bit adds one to the exponent field, and so does the carry into the next binade
  uint32_t bits = (static_cast<uint32_t>(E + 126) << 23) + static_cast<uint32_t>(m);
  if (bits > 0x7f800000u) bits = 0x7f800000u;
  return sign | bits;
}

enum { kPathTrivial = 0, kPathProduct = 1, kPathDivide = 2, kPathLimbs = 3 };

// which of the four ways decimal_bits takes (the probe's statistics)
PCP_ASCII_HD int decimal_path(uint64_t w, int32_t q) {
  if (w == 0 || q >= 39 || q < -65) return kPathTrivial;
  if (q >= 0) return (q <= 27 && bitlen64(w) + bitlen64(pow5_64(q)) <= 64) ? kPathProduct : kPathLimbs;
  return q >= -16 ? kPathDivide : kPathLimbs;
}

// the bits of the fp32 nearest w * 10^q (w < 10^19)
PCP_ASCII_HD uint32_t decimal_bits(bool neg, uint64_t w, int32_t q) {
  const uint32_t sign = neg ? 0x80000000u : 0u;
  if (w == 0) return sign;
  if (q >= 39) return sign | 0x7f800000u;
  if (q < -65) return sign;
  const int bw = bitlen64(w);
  if (q >= 0) {
    if (q <= 27) {
      const uint64_t p = pow5_64(q);
      if (bw + bitlen64(p) <= 64) return round_pack(neg, w * p, false, q);  // w * p < 2^bw * 2^bitlen(p) <= 2^64: exact
    }
    U192 N = mul192_pow5(u192(w), q);  // < 2^64 * 5^38 < 2^153
    const int bl = bitlen192(N);
    bool sticky = false;
    const int sh = bl > 64 ? bl - 64 : 0;
    N = shr192(N, sh, &sticky);  // the top 64 bits: far more than 26
    return round_pack(neg, N.l0, sticky, q + sh);
  }
  const int k = -q;  // 1 .. 65
  if (k <= 16) {
    // w / 5^k * 2^-k: (w << s) / 5^k with w << s >= 2^63 and 5^k < 2^38 has at least 26 bits; the remainder is exact
    const uint64_t D = pow5_64(k);
    const int s = 64 - bw;
    const uint64_t num = w << s;
    const uint64_t Q = num / D;
    return round_pack(neg, Q, num - Q * D != 0, -s - k);
  }
  // numerator and divisor aligned 26 bits apart: the quotient is in [2^25, 2^27)
  U192 D = mul192_pow5(u192(1), k);  // < 2^151
  const int s = bitlen192(D) + 26 - bw;
  U192 num = u192(w);
  if (s >= 0)
    num = shl192(num, s);  // bitlen(D) + 26 <= 177 bits
  else
    D = shl192(D, -s);  // bw - 26 bits
  U192 dsh = shl192(D, 26);
  uint64_t Q = 0;
  for (int b = 26; b >= 0; --b) {
    if (ge192(num, dsh)) {
      num = sub192(num, dsh);
      Q |= uint64_t(1) << b;
    }
    dsh = shr192_1(dsh);
  }
  return round_pack(neg, Q, (num.l0 | num.l1 | num.l2) != 0, -s - k);
}

// DR3: the token s[p, e) (e > p, no blank inside) -> *bits, or false.  Reads no byte outside [p, e).
template <class Ptr>
PCP_ASCII_HD bool parse_token(Ptr s, int32_t p, int32_t e, uint32_t *bits) {
  int32_t i = p;
  uint32_t c = static_cast<uint8_t>(s[i]);
  bool neg = false;
  if (c == '+' || c == '-') {
    neg = c == '-';
    if (++i == e) return false;
    c = static_cast<uint8_t>(s[i]);
  }
  const uint32_t lc = c | 0x20u;
  if (lc == 'n' || lc == 'i') {  // nan | inf | infinity, any case
    const int32_t n = e - i;
    if (n != 3 && n != 8) return false;
    uint64_t word = 0;
    for (int32_t j = 0; j < n; ++j) word |= static_cast<uint64_t>(static_cast<uint8_t>(s[i + j]) | 0x20u) << (8 * j);
    if (n == 3 && word == 0x6e616eull) {  // "nan": the quiet NaN strtof returns, the sign kept
      *bits = (neg ? 0x80000000u : 0u) | 0x7fc00000u;
      return true;
    }
    if ((n == 3 && word == 0x666e69ull) || (n == 8 && word == 0x7974696e69666e69ull)) {  // "inf", "infinity"
      *bits = (neg ? 0x80000000u : 0u) | 0x7f800000u;
      return true;
    }
    return false;
  }
  uint64_t w = 0;
  int32_t q = 0, nd = 0;  // nd: digits taken into w from its first non-zero digit on
  bool any = false, frac = false;
  for (; i < e; ++i) {
    c = static_cast<uint8_t>(s[i]);
    const uint32_t d = c - '0';
    if (d <= 9u) {
      any = true;
      if (w == 0 && d == 0) {  // a leading zero
        if (frac) --q;
      } else if (nd < 19) {
        w = w * 10u + d;
        ++nd;
        if (frac) --q;
      } else if (d == 0) {  // a zero past the 19th digit: a trailing zero unless a digit follows
        if (!frac) ++q;
      } else {
        return false;  // 20 or more significant digits
      }
    } else if (c == '.' && !frac) {
      frac = true;
    } else {
      break;
    }
  }
  if (!any) return false;
  if (i < e) {
    c = static_cast<uint8_t>(s[i]);
    if (c != 'e' && c != 'E') return false;
    if (++i == e) return false;
    c = static_cast<uint8_t>(s[i]);
    bool eneg = false;
    if (c == '+' || c == '-') {
      eneg = c == '-';
      ++i;
    }
    int32_t ex = 0, ed = 0;
    for (; i < e; ++i) {
      const uint32_t d = static_cast<uint32_t>(static_cast<uint8_t>(s[i])) - '0';
      if (d > 9u || ++ed > 5) return false;
      ex = ex * 10 + static_cast<int32_t>(d);
    }
    if (ed == 0) return false;
    q += eneg ? -ex : ex;
  }
  *bits = decimal_bits(neg, w, q);
  return true;
}

// the columns a row is read by: `columns` tokens per row, x y z intensity at token c[0..3] (c[3] < 0: none, 0.0f)
struct RowCols {
  int32_t columns, c[4];
};

// DR2, DR5: the row s[b, e) (e: its '\n', or the end of a final window) -> v[0..3] = the bits of x y z intensity; false = bad.
// Reads no byte outside [b, e).
template <class Ptr>
PCP_ASCII_HD bool parse_row(Ptr s, int32_t b, int32_t e, const RowCols &rc, uint32_t *v0, uint32_t *v1, uint32_t *v2, uint32_t *v3) {
  if (e - b > kParseMaxRow) return false;
  *v3 = 0u;
  int32_t i = b;
  for (int32_t t = 0; t < rc.columns; ++t) {
    while (i < e && is_blank(static_cast<uint8_t>(s[i]))) ++i;
    if (i == e) return false;  // too few tokens
    int32_t j = i + 1;
    while (j < e && !is_blank(static_cast<uint8_t>(s[j]))) ++j;
    if (t == rc.c[0] || t == rc.c[1] || t == rc.c[2] || t == rc.c[3]) {
      uint32_t bits;
      if (!parse_token(s, i, j, &bits)) return false;
      if (t == rc.c[0]) *v0 = bits;
      if (t == rc.c[1]) *v1 = bits;
      if (t == rc.c[2]) *v2 = bits;
      if (t == rc.c[3]) *v3 = bits;
    }
    i = j;
  }
  return true;
}

// DR1: the sequential twin of the kernels.  The window s[0, bytes), bytes < 2^31; out arrays of max_rows words.
template <class Ptr>
PCP_ASCII_HD void parse_window(Ptr s, int32_t bytes, const RowCols &rc, bool final_window, int64_t max_rows, uint32_t *x, uint32_t *y,
                               uint32_t *z, uint32_t *in, int64_t *rows, int64_t *consumed, int64_t *bad_row) {
  int64_t r = 0;
  int32_t pos = 0;
  *bad_row = -1;
  while (r < max_rows && pos < bytes) {
    int32_t e = pos;
    while (e < bytes && static_cast<uint8_t>(s[e]) != '\n') ++e;
    if (e == bytes) {  // the bytes after the last '\n'
      if (!final_window) break;
      bool any = false;
      for (int32_t k = pos; k < bytes && !any; ++k) any = !is_blank(static_cast<uint8_t>(s[k]));
      if (!any) break;
    }
    uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if (!parse_row(s, pos, e, rc, &v0, &v1, &v2, &v3)) {
      *bad_row = r;
      break;
    }
    x[r] = v0;
    y[r] = v1;
    z[r] = v2;
    in[r] = v3;
    ++r;
    pos = e < bytes ? e + 1 : bytes;
  }
  *rows = r;
  *consumed = pos;
}

}  // namespace ascii
}  // namespace pcp
