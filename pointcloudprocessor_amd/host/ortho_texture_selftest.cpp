// ortho_texture_selftest -- csrc/pcp_ortho_texture.hpp compiled for the host (CPU only: never a GPU job).  Checks the raster
// rules (OT2), the surface point of a small map worked out by hand (OT3: the weights, the neighbours an interpolation reads,
// the step that cuts it, the raster's border), and runs OT3 over a fixed pseudo-random map of 37 x 29 pixels at every scale the
// tests use, with the interpolation on and off.  Prints a checksum of every depth and position bit and the number of
// mismatches; exit code 0 iff none.   usage: ortho_texture_selftest
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/pcp_ortho_texture.hpp"

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

static uint64_t fnv = 0xcbf29ce484222325ull;
static void mix(uint32_t w) {
  for (int b = 0; b < 4; ++b) {
    fnv ^= (w >> (8 * b)) & 0xffu;
    fnv *= 0x100000001b3ull;
  }
}

int main() {
  // OT2
  {
    ot::Raster r{};
    const char *why = nullptr;
    int32_t fit = 0;
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 0, 0, 1, 1, 0.05f, &r, &why, &fit) == 0 && r.w == 100 && r.h == 80 && r.k == 4);
    EXPECT(ot::raster_check(100, 80, 16, 90, 70, 10, 10, 5, 0, 0.05f, &r, &why, &fit) == 0 && r.x0 == 90 && r.interpolate == 0);
    EXPECT(ot::raster_check(100, 80, 0, 0, 0, 0, 0, 1, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 17, 0, 0, 0, 0, 1, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 0, 0, 0, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 0, 0, 6, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 10, 0, 1, 1, 0.05f, &r, &why, &fit) == 1);   // one of w, h zero
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 0, 10, 1, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 91, 0, 10, 10, 1, 1, 0.05f, &r, &why, &fit) == 1);  // leaves the raster
    EXPECT(ot::raster_check(100, 80, 4, 0, 71, 10, 10, 1, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, -1, 0, 10, 10, 1, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 2147483647, 10, 1, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 5, 0, 0, 0, 1, 1, 0.05f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 0, 0, 1, 1, 0.0f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 0, 0, 1, 1, -1.0f, &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 0, 0, 1, 1, om::bits_float(0x7f800000u), &r, &why, &fit) == 1);
    EXPECT(ot::raster_check(100, 80, 4, 0, 0, 0, 0, 1, 1, om::bits_float(0x7fc00000u), &r, &why, &fit) == 1);
    // 8192 x 8192 ortho pixels: 2^26; scale 2 is 2^28 and fits, scale 3 does not
    EXPECT(ot::raster_check(8192, 8192, 2, 0, 0, 0, 0, 1, 1, 0.05f, &r, &why, &fit) == 0);
    EXPECT(ot::raster_check(8192, 8192, 3, 0, 0, 0, 0, 1, 1, 0.05f, &r, &why, &fit) == 2 && fit == 2);
    EXPECT(ot::raster_check(8192, 8192, 16, 0, 0, 2048, 2048, 1, 1, 0.05f, &r, &why, &fit) == 2 && fit == 8);
  }

  // OT3 by hand: a map of 3 x 2 pixels; pixel 2 is empty, pixel 4 takes its values from pixel 3 (a filled one)
  {
    const int32_t W = 3, H = 2;
    const int32_t source[6] = {0, 1, -1, 3, 3, 5};
    const float depth[6] = {1.0f, 2.0f, 0.0f, 3.0f, 3.0f, 9.0f};
    auto at = [&](int32_t s) { return depth[s]; };
    float d = -1.0f;
    ot::Raster r{2, 0, 0, W, H, 1, 4.0f};
    // fine pixel (1, 1) of parent (0, 0): a = b = 1, neighbours (1, 0), (0, 1), (1, 1); wx = wy = 1/4
    EXPECT(ot::surface_depth(r, W, H, source, at, 1, 1, &d));
    EXPECT(d == (1.0f + 0.25f * 1.0f) + 0.25f * ((3.0f + 0.25f * 0.0f) - (1.0f + 0.25f * 1.0f)));  // 1.25 + 0.25 * 1.75
    // fine pixel (0, 0): its neighbours lie outside the raster: the parent's depth
    EXPECT(ot::surface_depth(r, W, H, source, at, 0, 0, &d) && d == 1.0f);
    // fine pixel (3, 1) of parent (1, 0): the neighbour (2, 0) has no source
    EXPECT(ot::surface_depth(r, W, H, source, at, 3, 1, &d) && d == 2.0f);
    // no surface behind the fine pixels of pixel 2
    EXPECT(!ot::surface_depth(r, W, H, source, at, 4, 1, &d) && !ot::surface_depth(r, W, H, source, at, 5, 0, &d));
    // fine pixel (4, 2) of parent (2, 1) = 9: the step to pixel (1, 1) = 3 is 6 > 4
    EXPECT(ot::surface_depth(r, W, H, source, at, 4, 2, &d) && d == 9.0f);
    r.max_step = 6.0f;  // ... and at 6 the neighbour (2, 0) above it still has no source
    EXPECT(ot::surface_depth(r, W, H, source, at, 4, 2, &d) && d == 9.0f);
    // fine pixel (4, 3): below is outside
    EXPECT(ot::surface_depth(r, W, H, source, at, 4, 3, &d) && d == 9.0f);
    // interpolation off
    r.interpolate = 0;
    EXPECT(ot::surface_depth(r, W, H, source, at, 1, 1, &d) && d == 1.0f);
    // an odd scale: the centre column reads the row neighbour only (a == 0)
    ot::Raster r3{3, 0, 0, W, H, 1, 4.0f};
    EXPECT(ot::surface_depth(r3, W, H, source, at, 1, 2, &d) && d == 1.0f + (2.0f / 6.0f) * (3.0f - 1.0f));  // parent (0, 0), b = 2
    EXPECT(ot::surface_depth(r3, W, H, source, at, 1, 1, &d) && d == 1.0f);                                  // the very centre
    EXPECT(ot::surface_depth(r3, W, H, source, at, 2, 1, &d) && d == 1.0f + (2.0f / 6.0f) * (2.0f - 1.0f));  // b == 0, a = 2
    // the position: o + ((s u + t v) + d n), s = (Xg + 0.5) * (gsd / k)
    const float o[3] = {10.0f, 20.0f, 30.0f}, u[3] = {1, 0, 0}, v[3] = {0, -1, 0}, n[3] = {0, 0, -1};
    float p[3];
    ot::surface_point(o, u, v, n, 0.5f, 2, 3, 1, 2.0f, p);
    EXPECT(p[0] == 10.0f + 3.5f * 0.25f && p[1] == 20.0f - 1.5f * 0.25f && p[2] == 28.0f);
  }

  // OT3 over a fixed map: 37 x 29 pixels, a third of them empty, a tenth filled from the pixel to their left, depths a smooth
  // slope with steps, so that max_step 0.04 cuts some neighbours and 10 cuts none
  {
    const int32_t W = 37, H = 29;
    std::vector<int32_t> source(W * H);
    std::vector<float> depth(W * H);
    for (int32_t q = 0; q < W * H; ++q) {
      const uint32_t h = rnd();
      source[q] = (h % 3u == 0u) ? -1 : ((h % 10u == 1u && q % W > 0 && source[q - 1] >= 0) ? source[q - 1] : q);
      depth[q] = 2.0f + 0.01f * static_cast<float>(q % W) + 0.003f * static_cast<float>(q / W) + ((h >> 8) % 7u == 0u ? 0.2f : 0.0f);
    }
    for (int32_t q = 0; q < W * H; ++q)
      if (source[q] >= 0) depth[q] = depth[source[q]];
    auto at = [&](int32_t s) { return depth[s]; };
    const float o[3] = {-6.05f, 5.05f, 10.0f}, u[3] = {1, 0, 0}, v[3] = {0, -1, 0}, n[3] = {0, 0, -1};
    const int32_t scales[5] = {1, 2, 3, 4, 16};
    long long surfaces = 0, moved = 0;
    for (int32_t k : scales)
      for (int interp = 0; interp < 2; ++interp)
        for (float step : {0.04f, 10.0f}) {
          const ot::Raster r{k, 3, 2, 30, 25, interp, step};
          for (int32_t Y = 0; Y < r.h * k; ++Y)
            for (int32_t X = 0; X < r.w * k; ++X) {
              const int32_t Xg = r.x0 * k + X, Yg = r.y0 * k + Y;
              float d = 0.0f, p[3] = {0, 0, 0};
              const bool ok = ot::surface_depth(r, W, H, source.data(), at, Xg, Yg, &d);
              EXPECT(ok == (source[(Yg / k) * W + Xg / k] >= 0));
              if (ok) {
                ot::surface_point(o, u, v, n, 0.05f, k, Xg, Yg, d, p);
                surfaces += 1;
                const float d00 = depth[source[(Yg / k) * W + Xg / k]];
                moved += d != d00 ? 1 : 0;
                if (!interp || k == 1) EXPECT(d == d00);
                if (d != d00) EXPECT(d > d00 - step && d < d00 + step);  // between the parent and neighbours within the step
              }
              mix(ok ? 1u : 0u);
              mix(om::float_bits(d));
              for (int a = 0; a < 3; ++a) mix(om::float_bits(p[a]));
            }
        }
    EXPECT(surfaces > 100000 && moved > 10000);
    std::printf("surfaces %lld interpolated %lld\n", surfaces, moved);
  }

  std::printf("checksum %016llx\n", static_cast<unsigned long long>(fnv));
  std::printf("%d mismatches\n", bad);
  return bad ? 1 : 0;
}
