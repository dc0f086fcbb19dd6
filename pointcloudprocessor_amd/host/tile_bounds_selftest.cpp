// tile_bounds_selftest -- csrc/pcp_tile_box.hpp compiled for the host: the inflation tile_classify_box gives the three camera
// coordinates of a tile's centre against brute force.  A tile is the eight corners of a random box and random points inside it
// (fp32); its centre, radius and half-extents are computed as the upload computes them (pcp_context.hip k_up_bounds); every
// member is transformed in fp32 as the kernels transform it (pcp_device.hpp xform) under random rigid matrices and under
// matrices with entries up to 2^40, and must land inside [X - rho_0, X + rho_0] x [Y - rho_1, Y + rho_1] x [Z - rho_2, Z + rho_2]
// around the fp64 image of the centre.  The program also counts how often a row's box bound beats the sphere's (on flat boxes it
// must).  CPU only.  Exit code 0 iff nothing lies outside.
// usage: tile_bounds_selftest [tiles]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/pcp_tile_box.hpp"

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static uint64_t next_u64() {
  rng_state += 0x9e3779b97f4a7c15ull;
  uint64_t v = rng_state;
  v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ull;
  v = (v ^ (v >> 27)) * 0x94d049bb133111ebull;
  return v ^ (v >> 31);
}
static double uniform(double lo, double hi) { return lo + (hi - lo) * (static_cast<double>(next_u64() >> 11) * 0x1p-53); }

static float next_up(float v) {  // as k_up_bounds rounds a bound up
  if (!std::isfinite(v)) return v;
  uint32_t b;
  std::memcpy(&b, &v, 4);
  b += 1u;
  std::memcpy(&v, &b, 4);
  return v;
}
static float inflate(double v) { return next_up(static_cast<float>(v * (1.0 + 1e-6))); }

// spectral-norm bound of the 3x3 part, as pcp_set_frames computes DevFrame::norm_bound
static double norm_bound(const float *m) {
  double rowmax = 0.0;
  for (int a = 0; a < 3; ++a) {
    double row = 0.0;
    for (int b = 0; b < 3; ++b) {
      double g = 0.0;
      for (int k = 0; k < 3; ++k) g += static_cast<double>(m[4 * k + a]) * static_cast<double>(m[4 * k + b]);
      row += std::fabs(g);
    }
    rowmax = std::max(rowmax, row);
  }
  return std::sqrt(rowmax) * (1.0 + 1e-9);
}

static void rigid_matrix(float *m) {
  double q[4], nrm = 0.0;
  for (double &v : q) {
    v = uniform(-1.0, 1.0);
    nrm += v * v;
  }
  nrm = std::sqrt(nrm) + 1e-12;
  for (double &v : q) v /= nrm;
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                       2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m[4 * r + c] = static_cast<float>(R[3 * r + c]);
    m[4 * r + 3] = static_cast<float>(uniform(-50.0, 50.0));
  }
}
static void wild_matrix(float *m) {  // entries of either sign and any magnitude from 2^-20 to 2^40, some of them zero
  for (int k = 0; k < 12; ++k) {
    const double mag = std::ldexp(uniform(1.0, 2.0), static_cast<int>(next_u64() % 61) - 20);
    m[k] = (next_u64() % 7 == 0) ? 0.0f : static_cast<float>((next_u64() & 1) ? mag : -mag);
  }
}

int main(int argc, char **argv) {
  const long tiles = argc > 1 ? std::atol(argv[1]) : 20000;
  const int kInterior = 24, kMatrices = 6;
  long outside = 0, points = 0, rows = 0, rows_box = 0, flat_rows = 0, flat_rows_box = 0;
  std::vector<float> px, py, pz;
  for (long t = 0; t < tiles; ++t) {
    // a box anywhere within +-60 m, a few centimetres to a few metres wide, every third one flat along a random axis
    float lo[3], hi[3];
    const bool flat = t % 3 == 0;
    const int flat_axis = static_cast<int>(next_u64() % 3);
    for (int a = 0; a < 3; ++a) {
      const double c = uniform(-60.0, 60.0), w = std::ldexp(uniform(1.0, 2.0), static_cast<int>(next_u64() % 8) - 6);
      lo[a] = static_cast<float>(c - w);
      hi[a] = (flat && a == flat_axis) ? (t % 6 == 0 ? lo[a] : static_cast<float>(c - w + 1e-3 * w)) : static_cast<float>(c + w);
      if (hi[a] < lo[a]) std::swap(lo[a], hi[a]);
    }
    px.clear(); py.clear(); pz.clear();
    for (int k = 0; k < 8; ++k) {
      px.push_back((k & 1) ? hi[0] : lo[0]);
      py.push_back((k & 2) ? hi[1] : lo[1]);
      pz.push_back((k & 4) ? hi[2] : lo[2]);
    }
    for (int k = 0; k < kInterior; ++k) {
      px.push_back(std::min(hi[0], std::max(lo[0], static_cast<float>(uniform(lo[0], hi[0])))));
      py.push_back(std::min(hi[1], std::max(lo[1], static_cast<float>(uniform(lo[1], hi[1])))));
      pz.push_back(std::min(hi[2], std::max(lo[2], static_cast<float>(uniform(lo[2], hi[2])))));
    }
    // the bound, as k_up_bounds builds it
    const float c[3] = {static_cast<float>(0.5 * (static_cast<double>(lo[0]) + hi[0])), static_cast<float>(0.5 * (static_cast<double>(lo[1]) + hi[1])),
                        static_cast<float>(0.5 * (static_cast<double>(lo[2]) + hi[2]))};
    double r2 = 0.0, h[3] = {0.0, 0.0, 0.0};
    for (size_t k = 0; k < px.size(); ++k) {
      const double dx = static_cast<double>(px[k]) - c[0], dy = static_cast<double>(py[k]) - c[1], dz = static_cast<double>(pz[k]) - c[2];
      r2 = std::fmax(r2, (dx * dx + dy * dy) + dz * dz);
      h[0] = std::fmax(h[0], std::fabs(dx));
      h[1] = std::fmax(h[1], std::fabs(dy));
      h[2] = std::fmax(h[2], std::fabs(dz));
    }
    const float r = inflate(std::sqrt(r2)), hx = inflate(h[0]), hy = inflate(h[1]), hz = inflate(h[2]);
    for (int mi = 0; mi < kMatrices; ++mi) {
      float m[12];
      if (mi < kMatrices / 2) rigid_matrix(m); else wild_matrix(m);
      const double s = norm_bound(m);
      const pcp::TileInflation inf = pcp::tile_inflation(m, s, c[0], c[1], c[2], r, hx, hy, hz);
      const double cx = c[0], cy = c[1], cz = c[2];
      const double C[3] = {(m[0] * cx + m[1] * cy) + (m[2] * cz + m[3]), (m[4] * cx + m[5] * cy) + (m[6] * cz + m[7]),
                           (m[8] * cx + m[9] * cy) + (m[10] * cz + m[11])};
      for (int k = 0; k < 3; ++k) {
        if (!(inf.row[k] <= inf.sphere)) ++outside;  // the minimum never exceeds the sphere's bound
        ++rows;
        if (inf.row[k] < inf.sphere) ++rows_box;
        if (flat && mi < kMatrices / 2) {
          ++flat_rows;
          if (inf.row[k] < inf.sphere) ++flat_rows_box;
        }
      }
      for (size_t k = 0; k < px.size(); ++k) {
        const float x = px[k], y = py[k], z = pz[k];
        const float got[3] = {x * m[0] + (y * m[1] + (z * m[2] + m[3])), x * m[4] + (y * m[5] + (z * m[6] + m[7])),
                              x * m[8] + (y * m[9] + (z * m[10] + m[11]))};
        ++points;
        for (int a = 0; a < 3; ++a) {
          if (!std::isfinite(got[a])) continue;  // (the classifier gives no verdict on a non-finite image)
          if (!(std::fabs(static_cast<double>(got[a]) - C[a]) <= inf.row[a])) {
            if (++outside <= 10)
              std::printf("outside: tile %ld matrix %d point %zu axis %d: |%.17g - %.17g| > %.17g (sphere %.17g)\n", t, mi, k, a,
                          static_cast<double>(got[a]), C[a], inf.row[a], inf.sphere);
          }
        }
      }
    }
  }
  std::printf("tile bounds: %ld tiles, %ld transformed points, %ld outside\n", tiles, points, outside);
  std::printf("rows: %ld, the box's bound is the smaller in %ld; rigid matrices on flat boxes: %ld of %ld\n", rows, rows_box, flat_rows_box,
              flat_rows);
  // on a flat box under a rotation the box's bound must win in most rows: a selftest in which the minimum always picked the sphere
  // would check nothing new
  const bool exercised = flat_rows_box * 2 > flat_rows;
  if (!exercised) std::printf("the box's bound was hardly ever the smaller\n");
  std::printf("tile_bounds_selftest: %ld outside\n", outside);
  return outside == 0 && exercised ? 0 : 1;
}
