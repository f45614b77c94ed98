// rt_gather_items.h -- the slot arithmetic of a gather (rt_hip_gather,
// csrc/rt_gather.h, csrc/rt_gather.cpp): where the trace leaves the deepest
// hit record of ray r of record i (its KParams::last slot), and how many slots
// and work items a batch of n records with k rays each needs, so the host sizes
// the hit-record buffers from the same statement the kernels index by.  The
// items are ambient occlusion's (csrc/rt_ao_items.h): whole records, lane
// q k + r for k <= 64, one record in rt_ao_rounds(k) rounds for k > 64.  Every
// (item, round) owns 64 consecutive slots, one per lane, idle lanes included:
// a slot belongs to at most one ray.  Plain C++ (host and device): the kernels,
// the host layer and tests/native/gather_items.cpp include it.
#pragma once

#include "rt_ao_items.h"

// rounds of an item: one for k <= 64 (whole records side by side in the wave)
RT_TILES_FN uint32_t rt_gather_rounds(uint32_t k) { return k <= 64u ? 1u : rt_ao_rounds(k); }
// work items of n records (rt_ao_item_count: the same items)
RT_TILES_FN unsigned long long rt_gather_item_count(unsigned long long n, uint32_t k) {
  return rt_ao_item_count(n, k);
}
// the 64 slots of round `round` of item `item` start here
RT_TILES_FN unsigned long long rt_gather_round_slot(unsigned long long item, uint32_t round, uint32_t k) {
  return (item * rt_gather_rounds(k) + round) * RT_RAY_ITEM;
}
// the slot of ray r (r < k) of record i
RT_TILES_FN unsigned long long rt_gather_slot(unsigned long long i, uint32_t r, uint32_t k) {
  if (k > 64u) return rt_gather_round_slot(i, r / RT_RAY_ITEM, k) + r % RT_RAY_ITEM;
  const unsigned long long spi = rt_ao_spi(k);
  return rt_gather_round_slot(i / spi, 0u, k) + (i % spi) * k + r;
}
// groups of 64 paths of the batch: what the hit-record buffers are sized by
// (hit_buffers' `items`), and the slots they hold
RT_TILES_FN unsigned long long rt_gather_path_groups(unsigned long long n, uint32_t k) {
  return rt_gather_item_count(n, k) * rt_gather_rounds(k);
}
RT_TILES_FN unsigned long long rt_gather_slot_count(unsigned long long n, uint32_t k) {
  return rt_gather_path_groups(n, k) * RT_RAY_ITEM;
}
