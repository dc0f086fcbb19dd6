// ortho_selftest -- csrc/pcp_ortho.hpp compiled for the host (CPU only: never a GPU job).  Checks ord() on the signed zeros
// and against the floats' own order, the floor guard at the raster's borders and the depth window's, the frame rules, and a
// tiny map worked out by hand (nearest wins, ties to the lowest global index, the fill's radius).  Prints the number of
// mismatches; exit code 0 iff none.   usage: ortho_selftest [count]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pcp_ortho.hpp"

using namespace pcp;

static int bad = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("line %d: %s\n", __LINE__, #cond);         \
      ++bad;                                                 \
    }                                                        \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return static_cast<uint32_t>(rng_state >> 16);
}

// the view that looks down the z axis: pixel (col, row) covers x in [col, col + 1) * gsd, y in (-(row + 1), -row] * gsd
static om::Frame down(int32_t w, int32_t h, float gsd, float d_min, float d_max) {
  om::Frame f{};
  f.u[0] = 1.0f;
  f.v[1] = -1.0f;
  f.n[2] = -1.0f;
  f.inv = om::inverse_gsd(gsd);
  f.w = w;
  f.h = h;
  f.wf = static_cast<float>(w);
  f.hf = static_cast<float>(h);
  f.d_min = d_min;
  f.d_max = d_max;
  return f;
}

int main(int argc, char **argv) {
  const int count = argc > 1 ? std::atoi(argv[1]) : 100000;

  // ord: -0 sorts below +0, the key's depth comes back bit for bit, and the order is the floats'
  EXPECT(om::ord(0x80000000u) == 0x7fffffffu && om::ord(0u) == 0x80000000u);
  EXPECT(om::ord(om::float_bits(-0.0f)) < om::ord(om::float_bits(0.0f)));
  for (int i = 0; i < count; ++i) {
    uint32_t a = rnd(), b = rnd();
    if ((a & 0x7f800000u) == 0x7f800000u || (b & 0x7f800000u) == 0x7f800000u) continue;  // no NaN or infinity reaches ord
    const float fa = om::bits_float(a), fb = om::bits_float(b);
    if (fa < fb) EXPECT(om::ord(a) < om::ord(b));
    if (fa > fb) EXPECT(om::ord(a) > om::ord(b));
    EXPECT(om::unord(om::ord(a)) == a);
    EXPECT(om::float_bits(om::key_depth(om::key_of(a, b))) == a && om::key_index(om::key_of(a, b)) == b);
  }

  // OM2 at the borders: a raster of 4 x 3 pixels of 0.5 m, window [-1, 1]
  {
    const om::Frame f = down(4, 3, 0.5f, -1.0f, 1.0f);
    int32_t px = -1;
    uint32_t db = 1;
    EXPECT(om::project(f, 0.0f, 0.0f, 0.0f, &px, &db) && px == 0 && db == 0u);      // t = -0 * ... : b = 0, depth -0 -> +0
    EXPECT(om::project(f, -0.0f, -0.0f, 0.0f, &px, &db) && px == 0 && db == 0u);
    EXPECT(!om::project(f, -1e-30f, 0.0f, 0.0f, &px, &db));                          // a < 0 by any amount
    EXPECT(!om::project(f, 2.0f, 0.0f, 0.0f, &px, &db));                             // a == W
    EXPECT(om::project(f, 1.9999999f, 0.0f, 0.0f, &px, &db) && px == 3);             // the last column
    EXPECT(!om::project(f, 0.0f, -1.5f, 0.0f, &px, &db));                            // b == H
    EXPECT(om::project(f, 0.0f, -1.4999999f, 0.0f, &px, &db) && px == 2 * 4);        // the last row
    EXPECT(om::project(f, 0.7f, -0.6f, 1.0f, &px, &db) && px == 1 * 4 + 1 && om::bits_float(db) == -1.0f);  // depth == d_min
    EXPECT(om::project(f, 0.7f, -0.6f, -1.0f, &px, &db) && om::bits_float(db) == 1.0f);                      // depth == d_max
    EXPECT(!om::project(f, 0.7f, -0.6f, 1.0000001f, &px, &db) && !om::project(f, 0.7f, -0.6f, -1.0000001f, &px, &db));
    const float inf = om::bits_float(0x7f800000u), nan = om::bits_float(0x7fc00000u);
    EXPECT(!om::project(f, nan, 0.0f, 0.0f, &px, &db) && !om::project(f, 0.0f, inf, 0.0f, &px, &db) &&
           !om::project(f, 0.0f, 0.0f, -inf, &px, &db));
    EXPECT(!om::project(f, 3e38f, 0.0f, 0.0f, &px, &db));                            // a overflows to +inf: not < W
  }

  // OM1
  {
    const float o[3] = {0, 0, 0}, u[3] = {1, 0, 0}, v[3] = {0, -1, 0}, n[3] = {0, 0, -1}, left[3] = {0, 0, 1}, skew[3] = {0.999f, 0.05f, 0};
    const char *why = nullptr;
    double fit = 0.0;
    EXPECT(om::frame_check(o, u, v, n, 0.01f, 100, 100, 0.0f, 1.0f, &why, &fit) == 0);
    EXPECT(om::frame_check(o, u, v, left, 0.01f, 100, 100, 0.0f, 1.0f, &why, &fit) == 1);  // left-handed
    EXPECT(om::frame_check(o, skew, v, n, 0.01f, 100, 100, 0.0f, 1.0f, &why, &fit) == 1);
    EXPECT(om::frame_check(o, u, v, n, 2.0f, 100, 100, 0.0f, 1.0f, &why, &fit) == 1);
    EXPECT(om::frame_check(o, u, v, n, 0.01f, 100, 100, 1.0f, 1.0f, &why, &fit) == 1);
    EXPECT(om::frame_check(o, u, v, n, 0.01f, 0, 100, 0.0f, 1.0f, &why, &fit) == 1);
    EXPECT(om::frame_check(o, u, v, n, 0.01f, 20000, 100, 0.0f, 1.0f, &why, &fit) == 2 && fit > 0.0122 && fit < 0.01222);
    EXPECT(om::frame_check(o, u, v, n, 0.01f, 16384, 8192, 0.0f, 1.0f, &why, &fit) == 2 && fit > 0.01414 && fit < 0.01416);
    EXPECT(om::frame_check(o, u, v, n, 0.01f, 16384, 4096, 0.0f, 1.0f, &why, &fit) == 0);
  }

  // a map of 4 x 3 pixels of 1 m by hand: rows (x, y, z) under the global indices 10 + row
  {
    const om::Frame f = down(4, 3, 1.0f, -10.0f, 10.0f);
    const float pts[][3] = {
        {0.5f, -0.5f, -2.0f},  // row 0: pixel 0, depth 2
        {0.6f, -0.4f, -1.0f},  // row 1: pixel 0, depth 1: nearer, wins
        {0.7f, -0.3f, -1.0f},  // row 2: pixel 0, depth 1: a tie, the higher index loses
        {3.5f, -2.5f, 1.0f},   // row 3: pixel 11, depth -1
        {3.5f, -2.5f, 0.0f},   // row 4: pixel 11, depth -0 -> +0: loses to the negative depth
        {9.0f, -0.5f, 0.0f},   // row 5: outside
        {2.5f, -0.5f, -20.f},  // row 6: behind the window
    };
    std::vector<unsigned long long> keys(12, om::kEmptyKey);
    int contributors = 0;
    for (uint32_t i = 0; i < 7; ++i) {
      int32_t px;
      uint32_t db;
      if (!om::project(f, pts[i][0], pts[i][1], pts[i][2], &px, &db)) continue;
      ++contributors;
      const unsigned long long k = om::key_of(db, 10u + i);
      if (k < keys[static_cast<size_t>(px)]) keys[static_cast<size_t>(px)] = k;
    }
    EXPECT(contributors == 5);
    EXPECT(om::key_index(keys[0]) == 11u && om::key_depth(keys[0]) == 1.0f);
    EXPECT(om::key_index(keys[11]) == 13u && om::key_depth(keys[11]) == -1.0f);
    for (int p = 1; p < 11; ++p) EXPECT(keys[static_cast<size_t>(p)] == om::kEmptyKey);
    // the fill's rule on the distance transform's result of pixel 5 = (1, 1): nearest pixel 0 at d2 = 2
    EXPECT(om::fill_source(2u, 0, 1) == -1 && om::fill_source(2u, 0, 2) == 0 && om::fill_source(0xffffffffu, -1, 1024) == -1);
    EXPECT(om::payload_of(0x01c0b0a0u, 7u) == 0x07c0b0a0u);
  }

  std::printf("%d mismatches\n", bad);
  return bad ? 1 : 0;
}
