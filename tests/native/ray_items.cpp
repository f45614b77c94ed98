// ray_items.cpp -- the host-testable arithmetic of a ray batch
// (csrc/rt_ray_items.h), pinned on the CPU (tests/test_rays_host.py builds it
// plain and with g++ -fsanitize=address,undefined; no GPU, no HIP).
//
// Item counts and the 8 item streams partition every batch's rays exactly
// once, as rays_trace_kernel's loop takes them; the hit buffers' first sizing
// holds two records per ray and stays inside the 29-bit slot field; the batch
// limit is what the record index addresses; which rays are traced; and the
// two ray orders of rt_hip_frame_rays are bijections, the quarter order's
// aligned 64 one 4x4 quarter in rt_item_pixel's lane layout.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rt_ray_items.h"

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

static bool traced(float ox, float oy, float oz, float dx, float dy, float dz) {
  const uint32_t o[3] = {bits(ox), bits(oy), bits(oz)}, d[3] = {bits(dx), bits(dy), bits(dz)};
  return rt_ray_traced(o, d) != 0;
}

// rays_trace_kernel's walk over the streams with `grid` one-wave workgroups,
// the counters' atomics taken in any order: the items each wave would take
static void walk_streams(uint32_t nitems, uint32_t grid, std::vector<int>& taken) {
  uint32_t counter[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t b = 0; b < grid; b++) {
    const uint32_t home = b & 7u;
    uint32_t probe = 0;
    bool first = true;
    for (;;) {
      const uint32_t x = (home + probe) & 7u;
      uint32_t q;
      if (first) {
        q = b >> 3;
        first = false;
      } else {
        q = counter[x]++ + (grid - x + 7u) / 8u;
      }
      if (q >= rt_ray_stream_items(nitems, x)) {
        if (++probe == 8u) break;
        continue;
      }
      const uint32_t item = rt_ray_stream_item(q, x);
      CHECK(item < nitems, "items %u grid %u: wave %u takes item %u", nitems, grid, b, item);
      if (item < nitems) taken[item]++;
    }
  }
}

int main() {
  // ---- item counts and streams
  const unsigned long long ns[] = {0, 1, 63, 64, 65, 8 * 64 + 1, 100000};
  for (unsigned long long n : ns) {
    const uint32_t items = rt_ray_item_count(n);
    CHECK((unsigned long long)items * 64 >= n && (items == 0 || (unsigned long long)(items - 1) * 64 < n),
          "%llu rays in %u items", n, items);
    uint32_t sum = 0;
    std::vector<int> seen(items, 0);
    for (uint32_t x = 0; x < 8; x++) {
      const uint32_t nx = rt_ray_stream_items(items, x);
      sum += nx;
      for (uint32_t q = 0; q < nx; q++) {
        const uint32_t k = rt_ray_stream_item(q, x);
        CHECK(k < items && k % 8 == x, "stream %u item %u of %u", x, k, items);
        if (k < items) seen[k]++;
      }
      CHECK(rt_ray_stream_item(nx, x) >= items, "stream %u holds more than %u of %u items", x, nx, items);
    }
    CHECK(sum == items, "%llu rays: streams hold %u of %u items", n, sum, items);
    for (uint32_t k = 0; k < items; k++) CHECK(seen[k] == 1, "item %u in %d streams", k, seen[k]);
    // the kernel's loop at grids below, at and above the item count
    const uint32_t grids[] = {1, 3, 8, 9, items ? items : 1, 5120};
    for (uint32_t g : grids) {
      if (g > (items ? items : 1)) continue;  // the host clamps the grid to the items
      std::vector<int> taken(items, 0);
      walk_streams(items, g, taken);
      for (uint32_t k = 0; k < items; k++) CHECK(taken[k] == 1, "%u items, grid %u: item %u taken %d times", items, g, k, taken[k]);
    }
  }
  // ---- the limit: what region | (slot << 3) addresses, and its items
  CHECK(RT_RAY_BATCH_MAX == 8ull * ((1ull << 29) - 1), "limit %llu", (unsigned long long)RT_RAY_BATCH_MAX);
  CHECK(RT_RAY_BATCH_MAX == 0xfffffff8ull, "limit %llx", (unsigned long long)RT_RAY_BATCH_MAX);
  {
    const uint32_t top = 7u | ((uint32_t)RT_REC_SLOT_MAX << 3);  // the last record index
    CHECK(top == 0xffffffffu, "the slot field fills the index (%x): RT_REC_SLOT_MAX itself is RT_NO_REC's slot", top);
    const uint32_t items = rt_ray_item_count(RT_RAY_BATCH_MAX);
    CHECK(items == (1u << 26), "%u items at the limit", items);
    CHECK((unsigned long long)items * 64 + 63 < (1ull << 33), "ray indices at the limit");
    uint32_t sum = 0;
    for (uint32_t x = 0; x < 8; x++) sum += rt_ray_stream_items(items, x);
    CHECK(sum == items, "streams at the limit hold %u of %u", sum, items);
  }
  // ---- sizing: two records per ray over 8 regions, never past the slot field
  for (unsigned long long n : ns) {
    const size_t items = rt_ray_item_count(n);
    const size_t per = rt_hit_region_records(items, 0);
    CHECK(per * 8 >= 2 * items * 64 && per >= 1024, "%llu rays: %zu records per region", n, per);
    CHECK(per <= (2 * items * 64 + 7) / 8 + 1024, "%llu rays: %zu records per region is more than asked", n, per);
    CHECK(rt_hit_region_records(items, per + 5) == per + 5, "a larger need wins");
    CHECK(rt_hit_region_records(items, 1) == per, "a smaller need does not");
  }
  CHECK(rt_hit_region_records(rt_ray_item_count(RT_RAY_BATCH_MAX), 0) == RT_REC_SLOT_MAX, "clamped to the slot field");
  CHECK(rt_hit_region_records(1, (size_t)1 << 40) == RT_REC_SLOT_MAX, "a huge need is clamped too");
  // a frame's buffers: 4 items per tile (what rt_hip_render has always asked for)
  CHECK(rt_hit_region_records(4 * 8100, 0) == (2 * 4 * 8100 * 64 + 7) / 8 + 1024, "1080p frame");
  // ---- which rays are traced
  {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float den = std::numeric_limits<float>::denorm_min(), big = std::numeric_limits<float>::max();
    CHECK(traced(0, 0, 0, 0, 0, 1), "a plain ray");
    CHECK(traced(-big, big, 0, den, 0, 0), "finite extremes and a denormal direction");
    CHECK(traced(0, 0, 0, -0.0f, -1, 0), "a negative zero beside a component");
    CHECK(!traced(0, 0, 0, 0, 0, 0), "zero direction");
    CHECK(!traced(0, 0, 0, -0.0f, 0, -0.0f), "negative-zero direction");
    CHECK(!traced(nan, 0, 0, 0, 0, 1) && !traced(0, nan, 0, 0, 0, 1) && !traced(0, 0, nan, 0, 0, 1), "NaN origin");
    CHECK(!traced(0, 0, 0, inf, 0, 1) && !traced(0, 0, 0, 0, -inf, 1) && !traced(0, 0, 0, 0, 1, nan), "inf / NaN direction");
    CHECK(!traced(inf, 0, 0, 0, 0, 1), "inf origin");
  }
  // ---- ray orders: n = 4 W H for frames whose ray counts cover the edge cases
  const int sizes[][2] = {{4, 4}, {8, 4}, {4, 8}, {12, 8}, {100, 52}, {96, 56}};
  for (const auto& wh : sizes) {
    const int W = wh[0], H = wh[1];
    const size_t n = 4 * (size_t)W * (size_t)H;
    std::vector<int> pix(n, 0), qua(n, 0);
    for (size_t i = 0; i < n; i++) {
      int row, col, smp;
      rt_pixel_order_ray(W, i, &row, &col, &smp);
      CHECK(row >= 0 && row < H && col >= 0 && col < W && smp >= 0 && smp < 4, "pixel order %zu", i);
      CHECK(i == 4 * ((size_t)row * W + col) + (size_t)smp, "pixel order %zu -> (%d, %d, %d)", i, row, col, smp);
      if (row >= 0 && row < H && col >= 0 && col < W) pix[4 * ((size_t)row * W + col) + (size_t)smp]++;
      rt_quarter_order_ray(W, i, &row, &col, &smp);
      CHECK(row >= 0 && row < H && col >= 0 && col < W && smp >= 0 && smp < 4, "%dx%d quarter order %zu -> (%d, %d, %d)",
            W, H, i, row, col, smp);
      if (!(row >= 0 && row < H && col >= 0 && col < W && smp >= 0 && smp < 4)) continue;
      qua[4 * ((size_t)row * W + col) + (size_t)smp]++;
      // an aligned 64: one quarter, scanline order, rt_item_pixel's lanes
      const size_t quarter = i / 64, lane = i % 64;
      CHECK((size_t)(row / 4) * (size_t)(W / 4) + (size_t)(col / 4) == quarter, "ray %zu lies in quarter (%d, %d)", i,
            row / 4, col / 4);
      CHECK(lane == 4u * (4u * (unsigned)(row & 3) + (unsigned)(col & 3)) + (unsigned)smp, "ray %zu is lane %zu", i, lane);
      int r2, c2, s2;
      rt_item_pixel(0, (uint32_t)lane, &r2, &c2, &s2);
      CHECK(r2 == (row & 3) && c2 == (col & 3) && s2 == smp, "ray %zu against rt_item_pixel", i);
    }
    for (size_t i = 0; i < n; i++) CHECK(pix[i] == 1 && qua[i] == 1, "%dx%d sample %zu: %d, %d times", W, H, i, pix[i], qua[i]);
  }
  // the quarter map at the batch sizes of the item scheme: ray idx of a wide
  // strip of quarters (W = 4 * quarters, H = 4) is quarter idx / 64
  for (unsigned long long n : ns) {
    const size_t quarters = (size_t)rt_ray_item_count(n);
    if (!quarters) continue;
    const int W = (int)(4 * quarters);
    for (size_t i : {(size_t)0, (size_t)(n - 1), (size_t)(64 * quarters - 1)}) {
      int row, col, smp;
      rt_quarter_order_ray(W, i, &row, &col, &smp);
      CHECK(row >= 0 && row < 4 && col / 4 == (int)(i / 64) && col < W, "%llu rays, ray %zu -> (%d, %d)", n, i, row, col);
    }
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ray items ok\n");
  return 0;
}
