// pcp_ascii.hpp -- the text of a PCD ASCII row, for host and device alike ("Device PCD writer").
//
// put_g8(v, dst) writes what host/pcd_io.hpp's detail::put_float writes: glibc's snprintf("%.8g", (double)v), every NaN
// as "nan".  put_u32 is "%u" (the rgb and segmentMask columns).  No libc, no tables outside this file, fixed-width
// integers only; host/pcd_io.hpp does NOT use this header (it is the independent implementation the tests compare with).
//
// |v| = m * 2^e (m < 2^24, -149 <= e <= 104).  With X the decimal exponent (10^X <= |v| < 10^(X+1)) and k = 7 - X the
// eight significant digits are N = round-half-even(m * 2^e * 10^k), taken on the exact value in one of three ways:
//   0 <= k <= 12  (1e-5 <= |v| < 1e8: every fixed-notation value)  m * 5^k < 2^52: one 64-bit product, one shift;
//   k > 12        (|v| < 1e-5, subnormals included)  m * 5^k in three 64-bit limbs (<= 145 bits), shifted right by -(e + k);
//   k < 0         (|v| >= 1e8)  the integer m << (e + k) (<= 127 bits) divided by 5^-k (< 2^75) by 31 compare-and-subtract
//                 steps: no 128-bit division.
// X starts from floor(floor(log2 |v|) * log10 2), which is X or X - 1; N >= 1e8 moves it up (that is also the carry of
// 9.99999995 into the next decade), so N ends in [1e7, 1e8).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PCP_ASCII_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PCP_ASCII_HD inline
#endif

namespace pcp {
namespace ascii {

typedef unsigned __int128 u128;

constexpr int kMaxFloat = 14;  // "-1.1754944e-38"
constexpr int kMaxU32 = 10;    // "4294967295"

// 5^k, k <= 15
PCP_ASCII_HD uint64_t pow5(int k) {
  uint64_t p = 1;
  if (k & 1) p *= 5u;
  if (k & 2) p *= 25u;
  if (k & 4) p *= 625u;
  if (k & 8) p *= 390625u;
  return p;
}

// bits [0, s) set, 0 <= s <= 63
PCP_ASCII_HD uint64_t low_mask(int s) { return (uint64_t(1) << s) - 1u; }

// round-half-even(m * 2^e * 10^k) where the result is below 2^31 (k within one of 7 - X)
PCP_ASCII_HD uint64_t scaled_digits(uint32_t m, int e, int k) {
  if (k >= 0 && k <= 12) {
    const uint64_t num = static_cast<uint64_t>(m) * pow5(k);  // < 2^52
    const int sh = e + k;
    if (sh >= 0) return num << sh;
    const int r = -sh;  // < 64: num >> r is at least 1e6
    uint64_t q = num >> r;
    const uint64_t rem = num & low_mask(r), half = uint64_t(1) << (r - 1);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return q;
  }
  if (k > 12) {
    // m * 5^k in limbs l2:l1:l0, 13 powers of five at a time (5^13 < 2^31)
    uint64_t l0 = m, l1 = 0, l2 = 0;
    for (int left = k; left > 0; left -= 13) {
      const uint64_t c = pow5(left > 13 ? 13 : left);
      u128 t = static_cast<u128>(l0) * c;
      l0 = static_cast<uint64_t>(t);
      t = static_cast<u128>(l1) * c + static_cast<uint64_t>(t >> 64);
      l1 = static_cast<uint64_t>(t);
      t = static_cast<u128>(l2) * c + static_cast<uint64_t>(t >> 64);
      l2 = static_cast<uint64_t>(t);
    }
    const int r = -(e + k);  // 1 .. 127 here (|v| < 1e-5: e + k < 0)
    uint64_t q, half;
    bool sticky;
    if (r > 128) {
      const int s = r - 128;  // 1 .. 63 (not reached by fp32; kept total)
      q = l2 >> s;
      half = (l2 >> (s - 1)) & 1u;
      sticky = (l0 | l1) != 0 || (l2 & low_mask(s - 1)) != 0;
    } else if (r > 64) {
      const int s = r - 64;  // 1 .. 64
      q = s < 64 ? (l1 >> s) | (l2 << (64 - s)) : l2;
      half = (l1 >> (s - 1)) & 1u;
      sticky = l0 != 0 || (l1 & low_mask(s - 1)) != 0;
    } else {
      const int s = r;  // 1 .. 64
      q = s < 64 ? (l0 >> s) | (l1 << (64 - s)) : l1;
      half = (l0 >> (s - 1)) & 1u;
      sticky = (l0 & low_mask(s - 1)) != 0;
    }
    if (half && (sticky || (q & 1u))) ++q;
    return q;
  }
  // k < 0: |v| >= 1e8 is the integer m << e; 10^-k = 5^d 2^d and e >= d
  const int d = -k;
  u128 den = 1;
  for (int i = 0; i < d; ++i) den *= 5u;  // d <= 32: < 2^75
  u128 num = static_cast<u128>(m) << (e - d);
  uint64_t q = 0;
  for (int b = 30; b >= 0; --b) {
    const u128 t = den << b;
    if (t <= num) {
      num -= t;
      q |= uint64_t(1) << b;
    }
  }
  const u128 twice = num << 1;
  if (twice > den || (twice == den && (q & 1u))) ++q;
  return q;
}

enum { kFinite = 0, kZero = 1, kInf = 2, kNan = 3 };

// What "%.8g" prints of one fp32: the sign, the decimal exponent X, the eight digits as ASCII bytes packed into a
// word (the leading digit in the lowest byte) and the position of the last digit that is not a trailing zero.
struct G8 {
  uint64_t digits;
  int32_t X, last, cls;
  bool neg;
};

PCP_ASCII_HD G8 decode_g8(uint32_t bits) {
  G8 g;
  g.digits = 0;
  g.X = 0;
  g.last = 0;
  g.neg = (bits >> 31) != 0;
  const int be = static_cast<int>((bits >> 23) & 0xffu);
  const uint32_t frac = bits & 0x7fffffu;
  if (be == 255) {
    g.cls = frac ? kNan : kInf;
    if (frac) g.neg = false;
    return g;
  }
  if (be == 0 && frac == 0) {
    g.cls = kZero;
    return g;
  }
  g.cls = kFinite;
  const uint32_t m = frac | (be ? 0x800000u : 0u);
  const int e = (be ? be : 1) - 150;
  const int top = 31 - __builtin_clz(m);         // floor(log2 m)
  int X = ((top + e) * 78913) >> 18;             // floor((top + e) * log10 2) for |top + e| < 1650: X or X - 1
  uint64_t N = 0;
  for (int it = 0; it < 4; ++it) {
    N = scaled_digits(m, e, 7 - X);
    if (N >= 100000000u)
      ++X;
    else if (N < 10000000u)
      --X;
    else
      break;
  }
  uint32_t n32 = static_cast<uint32_t>(N);
  uint64_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    d = (d << 8) | (0x30u + n32 % 10u);
    n32 /= 10u;
  }
  int last = 7;
  while (last > 0 && ((d >> (8 * last)) & 0xffu) == 0x30u) --last;
  g.digits = d;
  g.X = X;
  g.last = last;
  return g;
}

PCP_ASCII_HD int length_g8(const G8 &g) {
  const int sign = g.neg ? 1 : 0;
  if (g.cls == kNan || g.cls == kInf) return sign + 3;
  if (g.cls == kZero) return sign + 1;
  if (g.X >= 0 && g.X <= 7) return sign + g.X + 1 + (g.last > g.X ? 1 + g.last - g.X : 0);
  if (g.X < 0 && g.X >= -4) return sign + 1 - g.X + g.last + 1;
  return sign + 1 + (g.last > 0 ? 1 + g.last : 0) + 4;
}

template <class Ptr>
PCP_ASCII_HD int emit_g8(const G8 &g, Ptr dst) {
  int n = 0;
  if (g.neg) dst[n++] = '-';
  if (g.cls == kNan) {
    dst[n++] = 'n';
    dst[n++] = 'a';
    dst[n++] = 'n';
    return n;
  }
  if (g.cls == kInf) {
    dst[n++] = 'i';
    dst[n++] = 'n';
    dst[n++] = 'f';
    return n;
  }
  if (g.cls == kZero) {
    dst[n++] = '0';
    return n;
  }
  uint64_t d = g.digits;
  if (g.X >= 0 && g.X <= 7) {
    for (int i = 0; i <= g.last || i <= g.X; ++i) {
      if (i == g.X + 1) dst[n++] = '.';
      dst[n++] = static_cast<char>(d & 0xffu);
      d >>= 8;
    }
    return n;
  }
  if (g.X < 0 && g.X >= -4) {
    dst[n++] = '0';
    dst[n++] = '.';
    for (int i = 0; i < -g.X - 1; ++i) dst[n++] = '0';
    for (int i = 0; i <= g.last; ++i) {
      dst[n++] = static_cast<char>(d & 0xffu);
      d >>= 8;
    }
    return n;
  }
  dst[n++] = static_cast<char>(d & 0xffu);
  if (g.last > 0) {
    dst[n++] = '.';
    for (int i = 1; i <= g.last; ++i) {
      d >>= 8;
      dst[n++] = static_cast<char>(d & 0xffu);
    }
  }
  const int ax = g.X < 0 ? -g.X : g.X;  // <= 45: two digits
  dst[n++] = 'e';
  dst[n++] = g.X < 0 ? '-' : '+';
  dst[n++] = static_cast<char>('0' + ax / 10);
  dst[n++] = static_cast<char>('0' + ax % 10);
  return n;
}

PCP_ASCII_HD uint32_t float_bits(float v) {
  uint32_t bits;
  __builtin_memcpy(&bits, &v, 4);
  return bits;
}

template <class Ptr>
PCP_ASCII_HD int put_g8(float v, Ptr dst) {
  return emit_g8(decode_g8(float_bits(v)), dst);
}
PCP_ASCII_HD int len_g8(float v) { return length_g8(decode_g8(float_bits(v))); }

PCP_ASCII_HD int len_u32(uint32_t v) {
  int n = 1;
  if (v >= 10u) ++n;
  if (v >= 100u) ++n;
  if (v >= 1000u) ++n;
  if (v >= 10000u) ++n;
  if (v >= 100000u) ++n;
  if (v >= 1000000u) ++n;
  if (v >= 10000000u) ++n;
  if (v >= 100000000u) ++n;
  if (v >= 1000000000u) ++n;
  return n;
}
template <class Ptr>
PCP_ASCII_HD int put_u32(uint32_t v, Ptr dst) {
  const int n = len_u32(v);
  for (int i = n - 1; i >= 0; --i) {
    dst[i] = static_cast<char>('0' + v % 10u);
    v /= 10u;
  }
  return n;
}

// the rgb column: r g b bytes as PointXYZRGB packs them, alpha 255
PCP_ASCII_HD uint32_t rgb_word(uint32_t r, uint32_t g, uint32_t b) { return 0xff000000u | (r << 16) | (g << 8) | b; }

}  // namespace ascii
}  // namespace pcp
