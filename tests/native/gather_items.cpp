// gather_items.cpp -- the slot arithmetic of a gather (csrc/rt_gather_items.h)
// on the CPU (tests/test_gather_host.py builds it plain and with g++
// -fsanitize=address,undefined; no GPU, no HIP).  For every k in 1..130 (and
// the limit RT_AO_KMAX) and a ragged set of n: the slots of all rays are
// distinct, lie below the slot count, are the places the trace kernel's lanes
// write by ambient occlusion's item map (rt_ao_spi, rt_ao_lane_sample,
// rt_ao_rounds), and the item count is rt_ao_item_count's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_gather_items.h"

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

static void check(unsigned long long n, uint32_t k) {
  const unsigned long long items = rt_gather_item_count(n, k), slots = rt_gather_slot_count(n, k);
  const uint32_t spi = rt_ao_spi(k), kinv = rt_ao_kinv(k), rounds = rt_gather_rounds(k);
  CHECK(items == rt_ao_item_count(n, k), "items of n %llu k %u", n, k);
  CHECK(rounds == (k <= 64 ? 1u : rt_ao_rounds(k)), "rounds of k %u", k);
  CHECK(rt_gather_path_groups(n, k) == items * rounds && slots == 64 * items * rounds, "sizes of n %llu k %u", n, k);
  CHECK(slots >= n * k, "a slot for every ray: n %llu k %u", n, k);
  // every ray's slot: below the count, nobody else's
  std::vector<unsigned char> taken(slots, 0);
  for (unsigned long long i = 0; i < n; i++)
    for (uint32_t r = 0; r < k; r++) {
      const unsigned long long s = rt_gather_slot(i, r, k);
      CHECK(s < slots, "slot %llu of (%llu, %u), k %u: %llu slots", s, i, r, k, slots);
      if (s >= slots) return;
      CHECK(!taken[s], "slot %llu twice: (%llu, %u), k %u", s, i, r, k);
      taken[s] = 1;
    }
  // the kernel's side: lane `lane` of round `round` of item `item` holds ray
  // r of record i by the item map, and writes slot round_slot + lane
  unsigned long long rays = 0;
  for (unsigned long long item = 0; item < items; item++)
    for (uint32_t round = 0; round < rounds; round++)
      for (uint32_t lane = 0; lane < 64; lane++) {
        const bool wide = k > 64;
        const uint32_t lq = wide ? 0u : rt_ao_lane_sample(lane, kinv);
        const uint32_t r = lane - lq * k + 64u * round;
        const unsigned long long i = item * spi + lq;
        const unsigned long long s = rt_gather_round_slot(item, round, k) + lane;
        CHECK(s < slots, "lane's slot %llu: item %llu round %u lane %u k %u", s, item, round, lane, k);
        if (!((wide || lane < spi * k) && i < n && r < k)) {
          if (s < slots) CHECK(!taken[s], "an idle lane's slot %llu is a ray's: k %u", s, k);
          continue;
        }
        rays++;
        CHECK(rt_gather_slot(i, r, k) == s, "(%llu, %u) k %u: slot %llu, the lane writes %llu", i, r, k,
              rt_gather_slot(i, r, k), s);
      }
  CHECK(rays == n * k, "the lanes hold every ray once: %llu of %llu, k %u", rays, n * k, k);
}

int main() {
  const unsigned long long ns[] = {0, 1, 2, 20, 21, 22, 63, 64, 65, 127, 129, 200};
  for (uint32_t k = 1; k <= 130; k++)
    for (unsigned long long n : ns) check(n, k);
  for (unsigned long long n : {1ull, 3ull}) check(n, RT_AO_KMAX_D);
  // the largest batches: the counts do not wrap
  for (uint32_t k : {1u, 33u, 64u, 65u, 1024u}) {
    const unsigned long long n = (unsigned long long)RT_RAY_BATCH_MAX / k;
    CHECK(rt_gather_slot_count(n, k) >= n * k && rt_gather_slot_count(n, k) < 2 * (n * k + 64ull * rt_gather_rounds(k)),
          "slots of the largest batch, k %u", k);
    CHECK(rt_gather_slot(n - 1, k - 1, k) < rt_gather_slot_count(n, k), "the last ray's slot, k %u", k);
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("gather items ok\n");
  return 0;
}
