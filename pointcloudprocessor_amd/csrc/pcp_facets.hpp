// pcp_facets.hpp -- the arithmetic of the planar facets of the map ("Planar facets", FA1-FA9), one copy for the
// kernels (pcp_facets.hip), the CPU forms (pcp_facets_host, pcp_facet_plane_host) and the host self-test
// (host/facets_selftest.cpp): which points take part, the quantised normal and its 8-byte record, the link between two facet
// points, the quantum of the moments, the check that keeps them inside 64 bits, and -- host only -- the brute-force partition
// and the plane of a facet from its integers.  The link is an integer predicate that is symmetric in its two points, so the
// facets are the connected components of an undirected graph: a function of the SET of points, independent of the order of
// the points, the lanes and the atomics.  Build without floating-point contraction.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "pcp_crack_fuse.hpp"
#include "pcp_eigen33_host.hpp"
#include "pcp_normals.hpp"

namespace pcp {
namespace fa {

constexpr float kNormalScale = 16384.0f;      // FA3: 2^14
constexpr float kMomentQuanta = 4096.0f;      // FA6: 2^12, the quantum is ~0.24 mm
constexpr int kRowWords = 10;                 // FA6: points S1x S1y S1z S2xx xy xz yy yz zz
constexpr int32_t kMinPointsHi = 1 << 24;     // FA5
constexpr int64_t kHostMaxPoints = 65536;     // pcp_facets_host
constexpr double kMomentBound = 4611686018427387904.0;  // FA6: 2^62

// ---- FA4: the constants of a call -----------------------------------------------------------------------------------------
struct Link {
  float t;       // GN2's threshold of the link radius
  int64_t c_q;   // ceil(cos(angle) * 2^28)
  int64_t t_q;   // floor(plane_tol * 2^34)
};

// nullptr, or what is wrong with the parameters
inline const char *refusal(float link_radius, float angle_deg, float plane_tol, float max_curvature, int32_t min_points) {
  if (!gn::radius_ok(link_radius)) return "link_radius outside [0.005, 1]";
  if (!(angle_deg > 0.0f && angle_deg <= 45.0f)) return "angle_deg outside (0, 45]";
  if (!(plane_tol >= 1e-4f && plane_tol <= 0.1f)) return "plane_tol outside [1e-4, 0.1]";
  if (!(max_curvature >= 0.0f && max_curvature <= 1.0f)) return "max_curvature outside [0, 1]";
  if (min_points < 1 || min_points > kMinPointsHi) return "min_points outside 1..2^24";
  return nullptr;
}

// host, fp64, once per call
inline Link link_of(float link_radius, float angle_deg, float plane_tol) {
  Link l;
  l.t = gn::threshold_of(link_radius);
  l.c_q = static_cast<int64_t>(std::ceil(std::cos(static_cast<double>(angle_deg) * (3.14159265358979323846 / 180.0)) * 268435456.0));
  l.t_q = static_cast<int64_t>(std::floor(static_cast<double>(plane_tol) * 17179869184.0));
  return l;
}

// ---- FA2 / FA3 ------------------------------------------------------------------------------------------------------------
struct Normal {
  int32_t x, y, z;
};

// a stored normal is valid when it is not (0, 0, 0) and no component exceeds 1 in magnitude (a NaN fails the comparison)
PCP_CF_HD bool normal_valid(float nx, float ny, float nz) {
  return fabsf(nx) <= 1.0f && fabsf(ny) <= 1.0f && fabsf(nz) <= 1.0f && (nx != 0.0f || ny != 0.0f || nz != 0.0f);
}

PCP_CF_HD bool facet_point(float x, float y, float z, float nx, float ny, float nz, float curvature, float max_curvature) {
  return gn::finite3(x, y, z) && normal_valid(nx, ny, nz) && curvature <= max_curvature;
}

// rint(c * 2^14), ties to even; the product is exact and |c| <= 1
PCP_CF_HD int32_t quantise_normal(float c) {
  const float p = c * kNormalScale;
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2int_rn(p);
#else
  return static_cast<int32_t>(lrintf(p));
#endif
}

PCP_CF_HD Normal normal_of(float nx, float ny, float nz) { return Normal{quantise_normal(nx), quantise_normal(ny), quantise_normal(nz)}; }

// the record: x | y << 16 in the low word, z | valid << 16 in the high one (components as 16-bit two's complement)
PCP_CF_HD void pack(const Normal &n, bool valid, uint32_t *lo, uint32_t *hi) {
  *lo = (static_cast<uint32_t>(n.x) & 0xffffu) | (static_cast<uint32_t>(n.y) << 16);
  *hi = (static_cast<uint32_t>(n.z) & 0xffffu) | (valid ? 0x10000u : 0u);
}
PCP_CF_HD Normal unpack(uint32_t lo, uint32_t hi) {
  return Normal{static_cast<int16_t>(lo & 0xffffu), static_cast<int16_t>(lo >> 16), static_cast<int16_t>(hi & 0xffffu)};
}
PCP_CF_HD bool record_valid(uint32_t hi) { return (hi & 0x10000u) != 0u; }

PCP_CF_HD int64_t dot(const Normal &a, int64_t x, int64_t y, int64_t z) { return (a.x * x + a.y * y) + a.z * z; }
PCP_CF_HD int64_t abs64(int64_t v) { return v < 0 ? -v : v; }

// FA4 on d = fl32(p_j - p_i) per axis.  The fp32 test first (most candidates of the neighbouring cells fail it), then the
// integers: |N . q| < 3 * 2^14 * (2^20 + 1) < 2^36.  Symmetric: from j, d and q change their signs and the absolute values stay.
PCP_CF_HD bool linked(float dx, float dy, float dz, const Normal &ni, const Normal &nj, const Link &l) {
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  if (!(d2 <= l.t)) return false;
  if (abs64(dot(ni, nj.x, nj.y, nj.z)) < l.c_q) return false;
  const int64_t qx = gn::quantise(dx), qy = gn::quantise(dy), qz = gn::quantise(dz);
  return abs64(dot(ni, qx, qy, qz)) <= l.t_q && abs64(dot(nj, qx, qy, qz)) <= l.t_q;
}

// ---- FA6 ------------------------------------------------------------------------------------------------------------------
// rint(d * 2^12) of d = fl32(p - p_root); |d * 2^12| < 2^31 for a facet that passed moments_fit
PCP_CF_HD int64_t moment_q(float d) {
  const float p = d * kMomentQuanta;
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2ll_rn(p);
#else
  return static_cast<int64_t>(llrintf(p));
#endif
}

// points * (D * 4096 + 1)^2 < 2^62 with D the largest extent of the facet's box (ordered integers): host, fp64
inline bool moments_fit(int64_t points, const uint32_t box[6]) {
  double extent = 0.0;
  for (int a = 0; a < 3; ++a)
    extent = std::fmax(extent, static_cast<double>(cf::value_of(box[3 + a])) - static_cast<double>(cf::value_of(box[a])));
  const double e = extent * 4096.0 + 1.0;
  return static_cast<double>(points) * (e * e) < kMomentBound;
}

// one member's ten additions to a row (points first)
PCP_CF_HD void add_member(int64_t row[kRowWords], int64_t qx, int64_t qy, int64_t qz) {
  row[1] += qx;
  row[2] += qy;
  row[3] += qz;
  row[4] += qx * qx;
  row[5] += qx * qy;
  row[6] += qx * qz;
  row[7] += qy * qy;
  row[8] += qy * qz;
  row[9] += qz * qz;
}

// ---- FA7: host only, fp64, from the integers -------------------------------------------------------------------------------
// x . y over three terms with error-free products and sums (Ogita, Rump and Oishi's Dot2): as if summed in twice the precision
inline double dot2(const double x[3], const double y[3]) {
  double p = x[0] * y[0];
  double s = std::fma(x[0], y[0], -p);
  for (int k = 1; k < 3; ++k) {
    const double h = x[k] * y[k], r = std::fma(x[k], y[k], -h);
    const double sum = p + h, bb = sum - p;
    const double q = (p - (sum - bb)) + (h - bb);
    p = sum;
    s += q + r;
  }
  return p + s;
}

// v^T C v / v^T v of C = xx xy xz yy yz zz: second-order accurate in v's error.  The closed form's own root is good to a few
// ulps of the LARGEST eigenvalue only -- 1e-9 of the smallest one of a 4 m wall with 1 mm of noise; its eigenvector is good
// to an ulp, and this quotient of it to ~1e-15 of the smallest eigenvalue.
inline double rayleigh(const double c[6], const double v[3]) {
  const double rows[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  const double cv[3] = {dot2(rows[0], v), dot2(rows[1], v), dot2(rows[2], v)};
  return dot2(v, cv) / dot2(v, v);
}

// out = centroid (3), unit normal (3, largest component positive; (0, 0, 0) when the members span no plane), rms (metres)
// from the smallest eigenvalue as the Rayleigh quotient of that normal.
// false: no member.
inline bool plane_of(const float root[3], const int64_t row[kRowWords], double out[7]) {
  if (row[0] < 1) return false;
  const double n = static_cast<double>(row[0]);
  for (int a = 0; a < 3; ++a) out[a] = static_cast<double>(root[a]) + (static_cast<double>(row[1 + a]) / n) * (1.0 / 4096.0);
  gn::Moments mo;
  mo.n = row[0];
  for (int a = 0; a < 3; ++a) mo.s1[a] = row[1 + a];
  for (int a = 0; a < 6; ++a) mo.s2[a] = row[4 + a];
  double c[6], scale = 0.0;
  gn::covariance(mo, c);
  for (int k = 0; k < 6; ++k) scale = std::fmax(scale, std::fabs(c[k]));
  if (!(scale > DBL_MIN)) scale = 1.0;
  double a[6], r[3], v[3];
  for (int k = 0; k < 6; ++k) a[k] = c[k] / scale;
  eig::roots3(a, r);
  eig::eigenvector(a, r[0], v);
  const bool spans = std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
  if (spans && v[eig::largest_component(v)] < 0.0)
    for (int k = 0; k < 3; ++k) v[k] = -v[k];
  for (int k = 0; k < 3; ++k) out[3 + k] = spans ? v[k] + 0.0 : 0.0;  // (+ 0.0: no negative zero)
  const double ev = spans ? rayleigh(c, v) : r[0] * scale;
  out[6] = std::sqrt(std::fmax(ev, 0.0) / n) * (1.0 / 4096.0);
  return true;
}

// ---- FA2-FA6 by brute force over the pairs (the core of pcp_facets_host) ---------------------------------------------------
struct Table {
  std::vector<int32_t> ids;      // ascending
  std::vector<int64_t> rows;     // kRowWords per facet
  std::vector<uint32_t> box;     // 6 per facet, ordered integers
  int64_t facet_points = 0, components = 0;
  int32_t unfit = -1;            // the id of a facet that failed moments_fit (the table is then without moments)
};

// label[i] = the lowest input index of i's facet, -1 for a point in none.  A plain union-find whose roots are the lowest
// indices.  false: a facet failed moments_fit (t.unfit).
inline bool partition_brute(int64_t n, const float *xyz, const float *normal, const float *curvature, const Link &l, float max_curvature,
                            int32_t min_points, int32_t *label, Table &t) {
  std::vector<int32_t> parent(static_cast<size_t>(n)), list;
  std::vector<Normal> nq(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    parent[static_cast<size_t>(i)] = static_cast<int32_t>(i);
    nq[static_cast<size_t>(i)] = Normal{0, 0, 0};
    if (!facet_point(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], curvature[i], max_curvature))
      continue;
    list.push_back(static_cast<int32_t>(i));
    nq[static_cast<size_t>(i)] = normal_of(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
  }
  auto find = [&](int32_t v) {
    while (parent[static_cast<size_t>(v)] != v) {
      parent[static_cast<size_t>(v)] = parent[static_cast<size_t>(parent[static_cast<size_t>(v)])];
      v = parent[static_cast<size_t>(v)];
    }
    return v;
  };
  for (size_t a = 0; a < list.size(); ++a) {
    const int32_t i = list[a];
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    for (size_t b = a + 1; b < list.size(); ++b) {
      const int32_t j = list[b];
      if (!linked(xyz[3 * j] - x, xyz[3 * j + 1] - y, xyz[3 * j + 2] - z, nq[static_cast<size_t>(i)], nq[static_cast<size_t>(j)], l)) continue;
      const int32_t ri = find(i), rj = find(j);
      if (ri < rj) parent[static_cast<size_t>(rj)] = ri;
      if (rj < ri) parent[static_cast<size_t>(ri)] = rj;
    }
  }
  // FA5: sizes, then the labels and the rows of the components that are large enough
  std::vector<int32_t> size(static_cast<size_t>(n), 0), row_of(static_cast<size_t>(n), -1);
  for (int32_t i : list) size[static_cast<size_t>(find(i))] += 1;
  for (int64_t i = 0; i < n; ++i) label[i] = -1;
  t = Table();
  t.facet_points = static_cast<int64_t>(list.size());
  for (int32_t i : list) {
    if (find(i) != i) continue;
    t.components += 1;
    if (size[static_cast<size_t>(i)] < min_points) continue;
    row_of[static_cast<size_t>(i)] = static_cast<int32_t>(t.ids.size());
    t.ids.push_back(i);
  }
  t.rows.assign(t.ids.size() * kRowWords, 0);
  t.box.resize(t.ids.size() * 6);
  std::vector<cf::Box> boxes(t.ids.size());
  for (cf::Box &b : boxes) cf::clear(b);
  for (int32_t i : list) {  // FA6, first pass
    const int32_t r = row_of[static_cast<size_t>(find(i))];
    if (r < 0) continue;
    label[i] = t.ids[static_cast<size_t>(r)];
    t.rows[static_cast<size_t>(r) * kRowWords] += 1;
    cf::add(boxes[static_cast<size_t>(r)], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  }
  for (size_t r = 0; r < t.ids.size(); ++r) {
    for (int a = 0; a < 3; ++a) {
      t.box[6 * r + a] = boxes[r].lo[a];
      t.box[6 * r + 3 + a] = boxes[r].hi[a];
    }
    if (t.unfit < 0 && !moments_fit(t.rows[r * kRowWords], &t.box[6 * r])) t.unfit = t.ids[r];
  }
  if (t.unfit >= 0) return false;
  for (int32_t i : list) {  // second pass
    if (label[i] < 0) continue;
    const int32_t id = label[i];
    add_member(&t.rows[static_cast<size_t>(row_of[static_cast<size_t>(id)]) * kRowWords], moment_q(xyz[3 * i] - xyz[3 * id]),
               moment_q(xyz[3 * i + 1] - xyz[3 * id + 1]), moment_q(xyz[3 * i + 2] - xyz[3 * id + 2]));
  }
  return true;
}

}  // namespace fa
}  // namespace pcp
