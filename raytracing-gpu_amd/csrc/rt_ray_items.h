// rt_ray_items.h -- the arithmetic of a caller's ray batch (rt_hip_trace_rays,
// csrc/rt_rays.h, csrc/rt_rays.cpp) that needs no device: how many rays a
// batch may hold, its work items and their streams, the hit-record buffers'
// first sizing, which rays are traced at all, and the two ray orders of
// rt_hip_frame_rays.  Plain C++ (host and device): the kernels, the host layer
// and tests/native/ray_items.cpp include it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_tiles.h"

// Hit records (rt_kernels.h): a record index is region | (slot << 3), 8
// regions and a 29-bit slot, so RT_REC_SLOT_MAX records per region.
#define RT_REC_REGIONS 8u
#define RT_REC_SLOT_BITS 29
#define RT_REC_SLOT_MAX ((1ull << RT_REC_SLOT_BITS) - 1)
// The most rays of one batch: every ray can leave at least its first record,
// so no more rays than the record index addresses.  Their work items
// (rt_ray_item_count) then fit 32 bits with room to spare.
#define RT_RAY_BATCH_MAX (RT_REC_REGIONS * RT_REC_SLOT_MAX)  // include/rt_hip.h RT_RAYS_MAX
#define RT_RAY_ITEM 64u  // rays of a work item: one per lane

// work items of n rays (n <= RT_RAY_BATCH_MAX): item k holds rays [64 k, 64 k + 64)
RT_TILES_FN uint32_t rt_ray_item_count(unsigned long long n) {
  return (uint32_t)((n + RT_RAY_ITEM - 1) / RT_RAY_ITEM);
}
// Items come in 8 streams like a frame's (rt_render.hip trace_kernel): stream
// x holds the items k = x (mod 8) in order, and its hits go to region x.
RT_TILES_FN uint32_t rt_ray_stream_items(uint32_t nitems, uint32_t x) {
  return nitems > x ? (nitems - x + 7u) / 8u : 0u;
}
RT_TILES_FN uint32_t rt_ray_stream_item(uint32_t q, uint32_t x) { return 8u * q + x; }

// Records per region the hit buffers are given for `items` work items of 64
// paths: two hits per path spread over the regions, or what an overflowing
// frame or batch needed (`need`, rt_hip_stats), within the slot field.
RT_TILES_FN size_t rt_hit_region_records(size_t items, size_t need) {
  size_t want = (2 * items * 64 + RT_REC_REGIONS - 1) / RT_REC_REGIONS + 1024;
  if (need > want) want = need;
  if (want > RT_REC_SLOT_MAX) want = (size_t)RT_REC_SLOT_MAX;
  return want;
}

// A ray is traced if its six components are finite and its direction is not
// all zero (the bits of the floats: no libm, the same test everywhere).
RT_TILES_FN int rt_ray_finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }
RT_TILES_FN int rt_ray_traced(const uint32_t o[3], const uint32_t d[3]) {
  int fin = 1;
  for (int a = 0; a < 3; a++) fin = fin && rt_ray_finite_bits(o[a]) && rt_ray_finite_bits(d[a]);
  const int zero = !((d[0] | d[1] | d[2]) & 0x7fffffffu);
  return fin && !zero;
}

// rt_hip_frame_rays: the camera sample (PPM row, PPM column, cpu sample) of ray
// `idx` of a width-pixel frame.  Pixel order: ray 4 (row W + col) + s.
RT_TILES_FN void rt_pixel_order_ray(int width, size_t idx, int* row, int* col, int* smp) {
  const size_t px = idx >> 2;
  *row = (int)(px / (size_t)width);
  *col = (int)(px % (size_t)width);
  *smp = (int)(idx & 3u);
}
// Quarter order (width and height multiples of 4): each aligned 64 rays are
// one 4x4-pixel quarter's 16 pixels x 4 samples in rt_item_pixel's lane
// layout, the quarters in scanline order -- what one work item of a frame's
// trace holds, so a batch in this order is coherent the way a frame's items are.
RT_TILES_FN void rt_quarter_order_ray(int width, size_t idx, int* row, int* col, int* smp) {
  const size_t quarter = idx / RT_RAY_ITEM, qx = (size_t)width / 4;
  int r, c;
  rt_item_pixel(0u, (uint32_t)(idx % RT_RAY_ITEM), &r, &c, smp);
  *row = (int)(4 * (quarter / qx)) + r;
  *col = (int)(4 * (quarter % qx)) + c;
}
