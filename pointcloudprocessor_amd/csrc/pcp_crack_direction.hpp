// pcp_crack_direction.hpp -- the arithmetic of the crack directions on the map ("Crack directions on the map",
// CD1-CD9), one copy for the kernel (pcp_crack_direction.hip), the CPU form (pcp_crack_directions_host, pcp_crack_axis_host)
// and the host self-test (host/crack_direction_selftest.cpp): the split of a moment word into the two halves a crack's row
// sums, the matrix whose smallest eigenpair is the covariance's largest, the sign rule, the vector of a degenerate pair, and
// the whole stage by brute force over the pairs.  The moments themselves are gn::Moments (pcp_normals.hpp).  Build without
// floating-point contraction.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "pcp_crack_fuse.hpp"
#include "pcp_normals.hpp"
#include "pcp_eigen33_host.hpp"

namespace pcp {
namespace cd {

constexpr int kRowWords = 2 * gn::kMomentWords;  // CD4: (lo, hi) of n, S1 x y z, S2 xx xy xz yy yz zz
constexpr int32_t kMinLinks = 2;                 // CD3

// ---- CD4: v = hi * 2^32 + lo with 0 <= lo < 2^32; both halves sum without a carry over fewer than 2^31 members ---------------
PCP_CF_HD uint64_t lo_of(int64_t v) { return static_cast<uint64_t>(v) & 0xffffffffull; }
PCP_CF_HD int64_t hi_of(int64_t v) { return v >> 32; }  // (arithmetic)
// CD5: the value of a summed word in fp64
PCP_CF_HD double value_of(int64_t lo, int64_t hi) { return static_cast<double>(hi) * 4294967296.0 + static_cast<double>(lo); }

// ---- CD3: M = trace(C) I - C is positive semi-definite with C, and its smallest eigenpair is C's largest -------------------
PCP_CF_HD double trace_of(const double C[6]) { return (C[0] + C[3]) + C[5]; }
PCP_CF_HD void flipped(const double C[6], double trace, double M[6]) {
  M[0] = trace - C[0];
  M[1] = -C[1];
  M[2] = -C[2];
  M[3] = trace - C[3];
  M[4] = -C[4];
  M[5] = trace - C[5];
}

// the sign rule: the component of largest magnitude is positive, ties go to the lowest axis
PCP_CF_HD void orient(double v[3]) {
  int b = 0;
  if (fabs(v[1]) > fabs(v[b])) b = 1;
  if (fabs(v[2]) > fabs(v[b])) b = 2;
  if (v[b] < 0.0) {
    v[0] = -v[0];
    v[1] = -v[1];
    v[2] = -v[2];
  }
}

PCP_CF_HD bool unit_ok(const double v[3]) {
  const double l = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  return l > 0.5 && l < 2.0;  // (false for a NaN)
}

// The closed form finds the vector as a cross product of two rows of (M - r I); with a double root (l1 == l2: no direction is
// preferred) all three vanish.  Then any unit vector orthogonal to the longest row is an eigenvector: that row crossed with the
// axis it has least of; with three equal roots the x axis.
PCP_CF_HD void degenerate_vector(const double M[6], double r, double v[3]) {
  const double rows[3][3] = {{M[0] - r, M[1], M[2]}, {M[1], M[3] - r, M[4]}, {M[2], M[4], M[5] - r}};
  int b = 0;
  double len[3];
  for (int i = 0; i < 3; ++i) {
    len[i] = (rows[i][0] * rows[i][0] + rows[i][1] * rows[i][1]) + rows[i][2] * rows[i][2];
    if (len[i] > len[b]) b = i;
  }
  v[0] = 1.0;
  v[1] = v[2] = 0.0;
  if (!(len[b] > 0.0)) return;
  const double ux = rows[b][0], uy = rows[b][1], uz = rows[b][2];
  int e = 0;
  if (fabs(uy) < fabs(ux)) e = 1;
  if (fabs(uz) < fabs(e == 0 ? ux : uy)) e = 2;
  // u x e_axis
  double cx, cy, cz;
  if (e == 0) {
    cx = 0.0, cy = uz, cz = -uy;
  } else if (e == 1) {
    cx = -uz, cy = 0.0, cz = ux;
  } else {
    cx = uy, cy = -ux, cz = 0.0;
  }
  const double l = sqrt((cx * cx + cy * cy) + cz * cz);
  if (!(l > 0.0)) return;
  v[0] = cx / l;
  v[1] = cy / l;
  v[2] = cz / l;
}

// ---- the largest eigenpair on the host (pcp_eigen33_host.hpp on M scaled to a largest magnitude of 1) ------------------------
// false: no direction (trace <= 0 or l1 <= 0); else v the oriented unit vector and *anisotropy = l1 / trace
inline bool largest_pair_host(const double C[6], double v[3], double *anisotropy) {
  v[0] = v[1] = v[2] = 0.0;
  *anisotropy = 0.0;
  const double trace = trace_of(C);
  if (!(trace > 0.0)) return false;
  double M[6], a[6], r[3];
  flipped(C, trace, M);
  double scale = 0.0;
  for (int k = 0; k < 6; ++k) scale = std::fmax(scale, std::fabs(M[k]));
  if (scale <= DBL_MIN) scale = 1.0;
  for (int k = 0; k < 6; ++k) a[k] = M[k] / scale;
  eig::roots3(a, r);
  const double l1 = trace - r[0] * scale;
  if (!(l1 > 0.0)) return false;
  eig::eigenvector(a, r[0], v);
  if (!unit_ok(v)) degenerate_vector(a, r[0], v);
  orient(v);
  *anisotropy = l1 / trace;
  return true;
}

// CD3 from the moments of one point
inline void tangent_host(const gn::Moments &mo, float tangent[3], float *anisotropy) {
  tangent[0] = tangent[1] = tangent[2] = 0.0f;
  *anisotropy = 0.0f;
  if (mo.n < kMinLinks) return;
  double C[6], v[3], an;
  gn::covariance(mo, C);
  if (!largest_pair_host(C, v, &an)) return;
  for (int a = 0; a < 3; ++a) tangent[a] = static_cast<float>(v[a]);
  *anisotropy = static_cast<float>(an);
}

// CD5: out5 = L, axis x y z, anisotropy
inline void axis_host(const int64_t row[kRowWords], double out5[5]) {
  const double L = value_of(row[0], row[1]);
  out5[0] = L;
  out5[1] = out5[2] = out5[3] = out5[4] = 0.0;
  if (!(L >= 2.0)) return;
  double C[6], v[3], an;
  for (int k = 0; k < 6; ++k) C[k] = value_of(row[2 * (4 + k)], row[2 * (4 + k) + 1]) / L;
  if (!largest_pair_host(C, v, &an)) return;
  out5[1] = v[0];
  out5[2] = v[1];
  out5[3] = v[2];
  out5[4] = an;
}

// ---- the whole stage on the host (the core of pcp_crack_directions_host) --------------------------------------------------
struct HostResult {
  std::vector<float> tangent;     // 3 n
  std::vector<float> anisotropy;  // n
  std::vector<int32_t> links;     // n
  std::vector<int64_t> moments;   // 10 n
  std::vector<int32_t> ids;       // C
  std::vector<int64_t> rows;      // 20 C
};

// xyz: n x 3; views: n.  Host only; quadratic in the crack points.  false: a point with gn::kMaxNeighbours links or more.
inline bool directions_brute(int64_t n, const float *xyz, const uint32_t *views, int32_t min_views, float t, HostResult &out) {
  const size_t sn = static_cast<size_t>(n);
  std::vector<int32_t> label(sn);
  cf::label_brute(n, xyz, views, min_views, t, label.data());
  std::vector<int32_t> list, row_of(sn, -1);
  out.ids.clear();
  for (int64_t i = 0; i < n; ++i)
    if (label[static_cast<size_t>(i)] >= 0) {
      list.push_back(static_cast<int32_t>(i));
      if (label[static_cast<size_t>(i)] == i) {  // (the rows ascend by id)
        row_of[static_cast<size_t>(i)] = static_cast<int32_t>(out.ids.size());
        out.ids.push_back(static_cast<int32_t>(i));
      }
    }
  out.tangent.assign(3 * sn, 0.0f);
  out.anisotropy.assign(sn, 0.0f);
  out.links.assign(sn, 0);
  out.moments.assign(static_cast<size_t>(gn::kMomentWords) * sn, 0);
  out.rows.assign(static_cast<size_t>(kRowWords) * out.ids.size(), 0);
  for (size_t a = 0; a < list.size(); ++a) {
    const size_t i = static_cast<size_t>(list[a]);
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    gn::Moments mo;
    gn::clear(mo);
    for (size_t b = 0; b < list.size(); ++b) {
      if (b == a) continue;
      const size_t j = static_cast<size_t>(list[b]);
      gn::visit(mo, xyz[3 * j] - x, xyz[3 * j + 1] - y, xyz[3 * j + 2] - z, t);
    }
    if (mo.n >= gn::kMaxNeighbours) return false;
    int64_t w[gn::kMomentWords];
    gn::store(mo, w);
    int64_t *row = out.rows.data() + static_cast<size_t>(kRowWords) * static_cast<size_t>(row_of[static_cast<size_t>(label[i])]);
    for (int k = 0; k < gn::kMomentWords; ++k) {
      out.moments[static_cast<size_t>(gn::kMomentWords) * i + static_cast<size_t>(k)] = w[k];
      row[2 * k] = static_cast<int64_t>(static_cast<uint64_t>(row[2 * k]) + lo_of(w[k]));
      row[2 * k + 1] += hi_of(w[k]);
    }
    out.links[i] = static_cast<int32_t>(mo.n);
    tangent_host(mo, out.tangent.data() + 3 * i, &out.anisotropy[i]);
  }
  return true;
}

}  // namespace cd
}  // namespace pcp
