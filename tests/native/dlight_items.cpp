// dlight_items.cpp -- the host-testable arithmetic of direct light for records
// (csrc/rt_dlight_items.h), pinned on the CPU (tests/test_direct_light_host.py
// builds it plain and with g++ -fsanitize=address,undefined; no GPU, no HIP).
//
// Without arguments: which records shade, row by row at the predicate's edges,
// the proof-box test at its edges, and the items of a batch.  With (in, out):
// in = u64 n, u32 nobj, u32 0, then n records of 10 words (rt_gsample); out =
// one byte per record, rt_dl_shades -- what rtgpu.direct_light_shades must say.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_dlight_items.h"

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

static int shades(int prim, int obj, uint32_t nobj, float px, float py, float pz, float nx, float ny, float nz) {
  const uint32_t P[3] = {bits(px), bits(py), bits(pz)}, N[3] = {bits(nx), bits(ny), bits(nz)};
  return rt_dl_shades(prim, obj, nobj, P, N);
}

static void predicate() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float den = std::numeric_limits<float>::denorm_min();
  CHECK(shades(0, 0, 1, 1, 2, 3, 0, 1, 0) == 1, "an ordinary record");
  CHECK(shades(0x7fffffff, 2, 3, 0, 0, 0, 0, 0, -1e-30f) == 1, "the last prim, the last object, P = 0");
  CHECK(shades(-1, 0, 1, 1, 2, 3, 0, 1, 0) == 0, "a miss");
  CHECK(shades(INT32_MIN, 0, 1, 1, 2, 3, 0, 1, 0) == 0, "prim = INT_MIN");
  CHECK(shades(0, -1, 1, 1, 2, 3, 0, 1, 0) == 0, "obj = -1");
  CHECK(shades(0, 1, 1, 1, 2, 3, 0, 1, 0) == 0, "obj = the object count");
  CHECK(shades(0, 0, 0, 1, 2, 3, 0, 1, 0) == 0, "no objects");
  CHECK(shades(0, 0, 1, 1, 2, 3, 0, 0, 0) == 0, "a zero normal");
  CHECK(shades(0, 0, 1, 1, 2, 3, -0.0f, 0.0f, -0.0f) == 0, "-0.0 is zero (vector3_is_zero compares with ==)");
  CHECK(shades(0, 0, 1, 1, 2, 3, den, 0, 0) == 1, "a denormal normal is not zero");
  CHECK(shades(0, 0, 1, 1, 2, 3, 0, -0.0f, -den) == 1, "a negative denormal neither");
  CHECK(shades(0, 0, 1, 1, 2, 3, 3e38f, 3e38f, 3e38f) == 1, "a huge finite normal");
  for (int a = 0; a < 3; a++) {
    float P[3] = {1, 2, 3}, N[3] = {0, 1, 0};
    for (float bad : {inf, -inf, nan, -nan}) {
      P[a] = bad;
      CHECK(shades(0, 0, 1, P[0], P[1], P[2], 0, 1, 0) == 0, "non-finite P[%d]", a);
      P[a] = 1;
      N[a] = bad;
      CHECK(shades(0, 0, 1, 1, 2, 3, N[0], N[1], N[2]) == 0, "non-finite N[%d]", a);
      N[a] = a == 1 ? 1.0f : 0.0f;
    }
  }
  CHECK(shades(0, 0, 1, 3.4e38f, -3.4e38f, 1e-45f, 0, 1, 0) == 1, "the largest finite P");
}

static void box() {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float lo[3] = {-1, -2, -3}, hi[3] = {1, 2, 3};
  const float in[3] = {0, 0, 0}, c0[3] = {-1, -2, -3}, c1[3] = {1, 2, 3};
  CHECK(rt_dl_in_box(in, lo, hi) && rt_dl_in_box(c0, lo, hi) && rt_dl_in_box(c1, lo, hi), "the box is closed");
  for (int a = 0; a < 3; a++) {
    float p[3] = {0, 0, 0};
    p[a] = std::nextafter(hi[a], 10.0f);
    CHECK(!rt_dl_in_box(p, lo, hi), "one float above hi[%d]", a);
    p[a] = std::nextafter(lo[a], -10.0f);
    CHECK(!rt_dl_in_box(p, lo, hi), "one float below lo[%d]", a);
    p[a] = nan;
    CHECK(!rt_dl_in_box(p, lo, hi), "NaN is outside");
    float l2[3] = {-1, -2, -3};
    l2[a] = nan;
    CHECK(!rt_dl_in_box(in, l2, hi), "a NaN bound holds nothing");
  }
  const float z[3] = {0, 0, 0};
  CHECK(rt_dl_in_box(z, z, z) && !rt_dl_in_box(c1, z, z), "a zeroed descriptor's box holds the origin alone");
}

static void items() {
  // a batch's items are a ray batch's: 64 records each, 8 streams, every item in exactly one stream slot
  for (unsigned long long n : {0ull, 1ull, 63ull, 64ull, 65ull, 513ull, 2304ull, 2335ull, 33177600ull}) {
    const uint32_t ni = rt_ray_item_count(n);
    CHECK((unsigned long long)ni * 64 >= n && (ni == 0 || (unsigned long long)(ni - 1) * 64 < n), "items of %llu", n);
    unsigned long long seen = 0, sum = 0;
    for (uint32_t x = 0; x < 8; x++) {
      const uint32_t m = rt_ray_stream_items(ni, x);
      seen += m;
      if (m) {
        CHECK(rt_ray_stream_item(m - 1, x) < ni, "stream %u's last item of %u", x, ni);
        CHECK(rt_ray_stream_item(m, x) >= ni, "stream %u ends", x);
      }
      for (uint32_t q = 0; q < m && ni <= 4096; q++) sum += rt_ray_stream_item(q, x);
    }
    CHECK(seen == ni, "%llu records: %llu of %u items in streams", n, seen, ni);
    if (ni <= 4096) CHECK(sum == (unsigned long long)ni * (ni ? ni - 1 : 0) / 2, "each item once");
  }
}

int main(int argc, char** argv) {
  if (argc == 3) {
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned long long n = 0;
    uint32_t hdr[2] = {0, 0};
    if (std::fread(&n, sizeof n, 1, f) != 1 || std::fread(hdr, sizeof hdr, 1, f) != 1) return 2;
    std::vector<uint32_t> w(10 * (size_t)n);
    if (n && std::fread(w.data(), 40, (size_t)n, f) != (size_t)n) return 2;
    std::fclose(f);
    std::vector<unsigned char> out((size_t)n);
    for (size_t i = 0; i < (size_t)n; i++) {
      const uint32_t* r = &w[10 * i];
      out[i] = (unsigned char)rt_dl_shades((int)r[0], (int)r[1], hdr[0], r + 4, r + 7);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (n && std::fwrite(out.data(), 1, (size_t)n, f) != (size_t)n) return 2;
    std::fclose(f);
    std::printf("dlight items ok\n");
    return 0;
  }
  predicate();
  box();
  items();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("dlight items ok\n");
  return 0;
}
