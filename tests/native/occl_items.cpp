// occl_items.cpp -- the host-testable arithmetic of an occlusion batch
// (csrc/rt_occl_items.h), pinned on the CPU (tests/test_occlusion_host.py
// builds it plain and with g++ -fsanitize=address,undefined; no GPU, no HIP).
//
// Which rays are traced and which of them make a query, by the bits of tmax;
// and the tmax -> t_cut bound: for seeded (o, d, t) whose new_dist in the
// reference's float arithmetic (cpu/hit.c:35-37,58) is <= tmax, t <= t_cut(tmax)
// always holds -- with the few ulps between the prefilter's t and the
// reference's to spare -- so the prefilter never drops a record the exact test
// would accept, ties at the bound included.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "rt_occl_items.h"

static int failures = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
      failures++;                                                \
    }                                                            \
  } while (0)

static uint32_t bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, sizeof b);
  return b;
}
static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, sizeof f);
  return f;
}

// vector3_length (cpu/vector3.c): the float sum of squares, a double sqrt
static float length3(float x, float y, float z) { return (float)std::sqrt((double)((x * x + y * y) + z * z)); }

// new_dist of parameter t on the ray (o, d): |(o + normalize(d) * (t * |d|)) - o|
static float new_dist(const float o[3], const float d[3], float t) {
  const float dl = length3(d[0], d[1], d[2]);
  const float s = t * dl;
  float p[3];
  for (int a = 0; a < 3; a++) p[a] = o[a] + (d[a] / dl) * s;
  return length3(p[0] - o[0], p[1] - o[1], p[2] - o[2]);
}

static void tmax_classes() {
  const float inf = std::numeric_limits<float>::infinity();
  const float qnan = std::numeric_limits<float>::quiet_NaN();
  const uint32_t o[3] = {bits(1.0f), bits(-2.0f), bits(0.0f)}, d[3] = {bits(0.0f), bits(-0.0f), bits(1e-30f)};
  struct {
    float t;
    int traced, queried;
  } rows[] = {{1.0f, 1, 1},  {inf, 1, 1},   {std::numeric_limits<float>::denorm_min(), 1, 1},
              {0.0f, 1, 0},  {-0.0f, 1, 0}, {-1.0f, 1, 0},
              {-inf, 1, 0},  {qnan, 0, 0},  {-qnan, 0, 0},
              {from_bits(0x7f800001u), 0, 0}, {from_bits(0xffc12345u), 0, 0}};
  for (const auto& r : rows) {
    CHECK(rt_occl_traced(o, d, bits(r.t)) == r.traced, "tmax bits %08x", bits(r.t));
    CHECK(rt_occl_queried(o, d, bits(r.t)) == r.queried, "tmax bits %08x", bits(r.t));
    // the bit tests are the float compares
    CHECK(rt_occl_tmax_nan(bits(r.t)) == (r.t != r.t), "nan %08x", bits(r.t));
    CHECK(rt_occl_tmax_positive(bits(r.t)) == (r.t > 0.0f), "positive %08x", bits(r.t));
  }
  // a ray a ray batch refuses is refused here whatever its tmax
  const uint32_t zero[3] = {bits(0.0f), bits(-0.0f), bits(0.0f)}, bad[3] = {bits(inf), bits(0.0f), bits(1.0f)};
  const uint32_t nano[3] = {bits(qnan), bits(0.0f), bits(0.0f)};
  CHECK(!rt_occl_traced(o, zero, bits(1.0f)) && !rt_occl_queried(o, zero, bits(1.0f)), "zero direction");
  CHECK(!rt_occl_traced(o, bad, bits(inf)) && !rt_occl_traced(nano, d, bits(1.0f)), "non-finite ray");
  // every bit pattern of a sweep agrees with the compares
  for (uint64_t b = 0; b <= 0xffffffffull; b += 0x10001ull) {
    const float t = from_bits((uint32_t)b);
    CHECK(rt_occl_tmax_nan((uint32_t)b) == (t != t) && rt_occl_tmax_positive((uint32_t)b) == (t > 0.0f), "bits %08x",
          (uint32_t)b);
    if (failures) return;
  }
}

static void t_cut_bound() {
  const float inf = std::numeric_limits<float>::infinity();
  CHECK(rt_occl_t_cut(inf, 3.0f, 0.5f) == inf, "no bound stays no bound");
  CHECK(rt_occl_t_cut(2.0f, 0.0f, 1.0f) >= 2.0f && rt_occl_t_cut(2.0f, 0.0f, 4.0f) >= 0.5f, "the bound is parametric");
  std::mt19937_64 rng(20261020);
  std::uniform_real_distribution<float> uni(-1.0f, 1.0f), u01(0.0f, 1.0f);
  unsigned long long cases = 0, ties = 0;
  for (int it = 0; it < 400000; it++) {
    // origins up to 1e4 from 0, directions of length 2^-6 .. 2^3, distances 0.01 .. 1e5
    const float os = std::pow(10.0f, 4.0f * u01(rng) - 0.5f * (it & 1));
    const float o[3] = {os * uni(rng), os * uni(rng), os * uni(rng)};
    float d[3] = {uni(rng), uni(rng), uni(rng)};
    if (it % 7 == 0) d[it % 3] = 0.0f;
    const float dl0 = length3(d[0], d[1], d[2]);
    if (!(dl0 > 1e-3f)) continue;
    const float want = std::pow(2.0f, 9.0f * u01(rng) - 6.0f);
    for (int a = 0; a < 3; a++) d[a] *= want / dl0;
    const float dl = length3(d[0], d[1], d[2]);
    const float dist = std::pow(10.0f, 7.0f * u01(rng) - 2.0f);
    const float t = dist / dl;
    const float nd = new_dist(o, d, t);
    if (!(nd > 0.0f) || !std::isfinite(nd)) continue;
    const float ao = std::fmax(std::fabs(o[0]), std::fmax(std::fabs(o[1]), std::fabs(o[2])));
    // tmax at the tie, one ulp above it and anywhere beyond
    const float tm[3] = {nd, std::nextafter(nd, inf), nd * (1.0f + 3.0f * u01(rng))};
    for (float tmax : tm) {
      const float cut = rt_occl_t_cut(tmax, ao, dl);
      cases++;
      ties += tmax == nd;
      CHECK(nd <= tmax && t <= cut, "o %g %g %g |d| %g t %g new_dist %g tmax %g t_cut %g", o[0], o[1], o[2], dl, t, nd,
            tmax, cut);
      // the prefilter's t is the reference's up to a few ulps (1 / a by v_rcp_f32)
      CHECK(t * (1.0f + 8.0f * std::numeric_limits<float>::epsilon()) <= cut, "no room for the prefilter's ulps: t %g t_cut %g",
            t, cut);
      if (failures > 8) return;
    }
    // below the tie the exact test refuses the record whatever the prefilter says
    CHECK(!(nd <= std::nextafter(nd, 0.0f)), "nextafter");
  }
  CHECK(cases > 1000000 && ties > 300000, "%llu cases, %llu ties", cases, ties);
  std::printf("t_cut: %llu (o, d, t, tmax) cases, %llu at the tie\n", cases, ties);
}

int main() {
  tmax_classes();
  t_cut_bound();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("occl items ok\n");
  return 0;
}
