// item_map.cpp -- the trace kernel's (item, lane) <-> (pixel, sample) map of
// csrc/rt_tiles.h, pinned on the CPU (tests/test_item_map.py builds it plain
// and with g++ -fsanitize=address,undefined; no GPU, no HIP).
//
// For every pixel and sample of a tile: rt_item_pixel and rt_item_slot are a
// bijection of the 4 x 64 (item, lane) slots onto the 64 x 4 (pixel, sample)
// pairs; the sample index orders (k, l) as cpu/raytracer.c:55-58 does; the
// slots fold_kernel (rt_pixel_slots + sample, one 16-byte load) and
// gbuffer_kernel (rt_item_slot) read are the ones the trace wrote; and the
// layout is the documented one, spelled here literally.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_tiles.h"

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

int main() {
  static_assert(RT_TILE_ITEMS == 4, "four work items per tile");
  const uint32_t tiles[] = {0u, 1u, 7u, 129599u, 0x00ffffffu};  // the last: indices past 2^32
  for (uint32_t t : tiles) {
    // trace_kernel writes slot (4t + q) * 64 + lane for the ray of rt_item_pixel(q, lane)
    std::vector<int> hits(256, 0);      // (pixel, sample) pairs reached
    std::vector<int> slot_hits(256, 0); // slots the inverse names
    const size_t base = (size_t)t * 256;
    for (uint32_t q = 0; q < 4; q++)
      for (uint32_t lane = 0; lane < 64; lane++) {
        int row = -1, col = -1, smp = -1;
        rt_item_pixel(q, lane, &row, &col, &smp);
        CHECK(row >= 0 && row < 8 && col >= 0 && col < 8 && smp >= 0 && smp < 4, "q %u lane %u -> %d %d %d", q, lane,
              row, col, smp);
        if (row < 0 || row >= 8 || col < 0 || col >= 8 || smp < 0 || smp >= 4) continue;
        hits[(size_t)(row * 8 + col) * 4 + (size_t)smp]++;
        const size_t written = ((size_t)t * 4 + q) * 64 + lane;
        // the inverse finds the slot the trace wrote
        const size_t s = rt_item_slot(t, row, col, smp);
        CHECK(s == written, "t %u q %u lane %u: inverse %zu, written %zu", t, q, lane, s, written);
        CHECK(s >= base && s < base + 256, "t %u: slot %zu outside the tile's 256", t, s);
        if (s >= base && s < base + 256) slot_hits[s - base]++;
        // the documented layout, literally
        CHECK(q == 2u * (uint32_t)(row >= 4) + (uint32_t)(col >= 4), "quarter of (%d, %d) is %u", row, col, q);
        CHECK(lane == 4u * (4u * (uint32_t)(row & 3) + (uint32_t)(col & 3)) + (uint32_t)smp, "lane of (%d, %d, %d) is %u",
              row, col, smp, lane);
      }
    for (int k = 0; k < 256; k++) {
      CHECK(hits[k] == 1, "t %u: (pixel %d, sample %d) reached %d times", t, k / 4, k % 4, hits[k]);
      CHECK(slot_hits[k] == 1, "t %u: slot %d named %d times", t, k, slot_hits[k]);
    }
    // the readers: one thread per tile-buffer slot = row * 8 + col
    for (uint32_t slot = 0; slot < 64; slot++) {
      const int row = (int)(slot >> 3), col = (int)(slot & 7u);
      const size_t b = rt_pixel_slots(t, row, col);  // fold_kernel's uint4 load
      CHECK(b % 4 == 0, "t %u pixel (%d, %d): slots start at %zu, not 16-byte aligned", t, row, col, b);
      for (int smp = 0; smp < 4; smp++) {
        const size_t g = rt_item_slot(t, row, col, smp);  // gbuffer_kernel's record (4 * slot + smp)
        CHECK(g == b + (size_t)smp, "t %u pixel (%d, %d) sample %d: %zu, fold reads %zu", t, row, col, smp, g,
              b + (size_t)smp);
        // ... and that slot's lane traces this pixel and sample
        int r2, c2, s2;
        rt_item_pixel((uint32_t)((g / 64) & 3u), (uint32_t)(g % 64), &r2, &c2, &s2);
        CHECK(r2 == row && c2 == col && s2 == smp && g / 256 == t, "slot %zu traces (%d, %d, %d) of tile %zu", g, r2,
              c2, s2, g / 256);
      }
    }
  }
  // cpu/raytracer.c:55-58: for (k = i; k < i + 1; k += 0.5) for (l = j; l < j + 1; l += 0.5)
  // -- the samples in order (k, l) = (0,0) (0,.5) (.5,0) (.5,.5); camera_sample
  // takes k from smp >> 1 and l from smp & 1
  {
    int smp = 0;
    for (float k = 0.0f; k < 1.0f; k += 0.5f)
      for (float l = 0.0f; l < 1.0f; l += 0.5f) {
        CHECK(0.5f * (float)(smp >> 1) == k && 0.5f * (float)(smp & 1) == l, "sample %d is (%g, %g)", smp, (double)k,
              (double)l);
        smp++;
      }
    CHECK(smp == 4, "%d samples", smp);
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("item map ok\n");
  return 0;
}
