// rt_gather.h -- traced light gathered over a record's hemisphere on the device
// (include/rt_hip.h rt_hip_gather): for every rt_gsample record the sum, in ray
// order, of the colours rt_hip_trace_rays gives the record's k hemisphere rays.
// The rays are ambient occlusion's (ao_ray of rt_ao.h, the rule of
// csrc/rt_ao_items.h), made in the trace kernel and never written out; each is
// the reference's trace(ray, 1.0) as in a ray batch (rt_rays.h): trace_path
// under RT_POLICY_RAYS appends its hit records, the frames' shade pass and
// off-box fixup shade them unchanged, and gather_fold_kernel sums each ray's
// chain deepest-first and then the record's k rays in order.
// gather_trace_kernel has the shape of rays_trace_kernel and the item of
// ao_kernel; where a ray's deepest record goes (KParams::last) is
// csrc/rt_gather_items.h.  Part of rt_render.hip's one translation unit, after
// rt_ao.h; its launches are csrc/rt_gather.cpp.
#pragma once

#include "rt_gather_items.h"

namespace rt {

// A work item is a.ao.spi whole records (rt_ao_items.h): lane q k + r is ray r
// of the item's record q for k <= 64; for k > 64 (WIDE, its own kernel, so
// k <= 64 has no round loop) the item's one record is walked in
// rt_ao_rounds(k) rounds of 64 rays.  The persistent one-wave workgroups and 8
// item streams of rays_trace_kernel: stream x = the items = x (mod 8), its hits
// in region x.  Every (item, round) writes its 64 lanes' deepest records to its
// own 64 slots (rt_gather_round_slot), RT_NO_REC for a lane without a ray: an
// idle lane, a record past n, a record that does not shoot, a ray a batch
// would not trace (rt_ray_traced).  Such a lane makes no query.  The ray is
// formed anew in every round, before the walk's state is live.
// (The item claim stays inline, as in the other kernels that pull items this
// way: through a shared function their scalar register allocation changed.)
template <int ACCEL, int POL, bool WIDE>
__global__ __launch_bounds__(64, RT_TRACE_MIN_WAVES) void gather_trace_kernel(KParams p, GatherArgs a) {
  const int lane = threadIdx.x & 63;
  WorkCount wc = {};
  __shared__ float4 s_stack[ACCEL == RT_ACCEL_FLAT_D ? 1 : kStackArea];
  __shared__ float4 s_stage[ACCEL == RT_ACCEL_FLAT_D ? kStageFlat : kStageOct];
  Stack stk;
  WaveCtx w;
  wave_state(p, s_stack, s_stage, lane, stk, w);
  constexpr bool wide = WIDE;
  const uint32_t rounds = wide ? rt_ao_rounds(a.ao.k) : 1u;
  const uint32_t home = (uint32_t)blockIdx.x & 7u;
  uint32_t probe = 0;
  bool first = true;
  for (;;) {
    const uint32_t x = (home + probe) & 7u;
    uint32_t q = 0;
    if (first) {
      q = (uint32_t)blockIdx.x >> 3;
      first = false;
    } else {
      if (lane == 0) q = atomicAdd(p.tile_counter + 32u * x, 1u);
      q = uni(q) + (gridDim.x - x + 7u) / 8u;
    }
    if (q >= rt_ray_stream_items(a.ao.nitems, x)) {
      if (++probe == 8u) break;  // every stream drained: the wave exits
      continue;
    }
    const uint32_t item = rt_ray_stream_item(q, x);
    const size_t i0 = (size_t)item * a.ao.spi;  // the item's first record
    for (uint32_t round = 0; round < rounds; round++) {
      // a lane without a ray walks nothing, but its ray takes part in the
      // packet walk's wave-wide arithmetic: a harmless one
      f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
      bool valid = false;
      {
        const uint32_t lq = wide ? 0u : rt_ao_lane_sample((uint32_t)lane, a.ao.kinv);
        const uint32_t r = (uint32_t)lane - lq * a.ao.k + 64u * round;
        const size_t i = i0 + (size_t)lq;
        f3 ro, rd;
        if ((wide || (uint32_t)lane < a.ao.spi * a.ao.k) && i < a.ao.n && r < a.ao.k && ao_ray(a.ao, i, r, ro, rd)) {
          const uint32_t ob[3] = {__float_as_uint(ro.x), __float_as_uint(ro.y), __float_as_uint(ro.z)};
          const uint32_t db[3] = {__float_as_uint(rd.x), __float_as_uint(rd.y), __float_as_uint(rd.z)};
          valid = rt_ray_traced(ob, db);
          if (valid) o = ro, d = rd;
        }
      }
      wc.pixels += (uint32_t)__popcll(__ballot(valid));  // the rays traced (rt_stats.camera of a batch)
      Capture cap;
      const uint32_t deepest =
          trace_path<ACCEL, false, POL>(p, valid, o, d, x, stk, w, wc, 0u, cap, 0, 1.0f, RT_NO_REC, a.ao.walk);
      p.last[(size_t)rt_gather_round_slot(item, round, a.ao.k) + (size_t)lane] = deepest;
    }
  }
  flush_counts(p, wc, lane);
}

// Per-record fold, the gather's last launch: for r = 0 .. k-1 the colour of ray
// r -- its path's terms summed deepest-first from 0, rays_fold_kernel's loop
// (kept inline here as there) -- added to the record's accumulator, which
// starts at +0: acc = color_add(acc, colour), one add per channel per ray, in
// ray order.  A ray that was not traced left RT_NO_REC: its colour is 0.  Three
// plain stores per record, every word of [0, 3 n) once; and the frame check's
// bookkeeping by thread 0.  One thread per record.
template <int>
__global__ __launch_bounds__(256) void gather_fold_kernel(KParams p, GatherArgs a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && p.frame_check) frame_check_account(p);
  if (i >= a.ao.n) return;
  col acc = init_color(0.0f, 0.0f, 0.0f);
  for (uint32_t ray = 0; ray < a.ao.k; ray++) {
    col sc = init_color(0.0f, 0.0f, 0.0f);
    uint32_t r = p.last[(size_t)rt_gather_slot(i, ray, a.ao.k)];
    while (r != RT_NO_REC && (r >> 3) < p.hit_cap) {
      const size_t at = rec_addr(p, r);
      const float4 tm = p.hit_term[at];
      sc = color_add(sc, col{tm.x, tm.y, tm.z});
      r = p.hit_prev[at];
    }
    acc = color_add(acc, sc);
  }
  float* o = a.rgb + 3 * i;
  o[0] = acc.r;
  o[1] = acc.g;
  o[2] = acc.b;
}

}  // namespace rt
