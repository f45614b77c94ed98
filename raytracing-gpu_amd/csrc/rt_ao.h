// rt_ao.h -- ambient occlusion from G-buffer records on the device
// (include/rt_hip.h rt_hip_ambient_occlusion): for every rt_gsample record the
// number of its k hemisphere rays that an occlusion batch would answer 1.  The
// rays are made in the kernel by the rule of csrc/rt_ao_items.h from the
// record's P and N, a caller's table and a hash of the record's index; the
// query is occl_q of rt_occl.h, unchanged.  ao_kernel has the shape of
// rays_occl_kernel; what differs is the item (whole samples, so a count is one
// wave's ballot and needs neither an atomic nor a cleared output).
// ao_rays_kernel writes the same rays out, for callers and tests that want
// them.  Part of rt_render.hip's one translation unit, after rt_occl.h; its
// launch is csrc/rt_ao.cpp.
#pragma once

#include "rt_ao_items.h"

namespace rt {

// Ray r of sample i by the rule: false (and nothing written) when the sample
// does not shoot.  The record's five 8-byte pairs are prim obj | queries dist |
// P.x P.y | P.z N.x | N.y N.z; the lanes of one sample load the same addresses.
__device__ __forceinline__ bool ao_ray(const AoArgs& a, size_t i, uint32_t r, f3& o, f3& d) {
  const uint2* s = a.samples + 5 * i;
  const uint2 w0 = s[0], w3 = s[3], w4 = s[4];
  const float N[3] = {__uint_as_float(w3.y), __uint_as_float(w4.x), __uint_as_float(w4.y)};
  const float l = rt_ao_length(N);
  if (!rt_ao_shoots((int)w0.x, l)) return false;
  const uint2 w2 = s[2];
  rt_ao_frame f;
  rt_ao_frame_of(N, l, &f);
  const uint32_t h = rt_ao_hash(a.base + (unsigned long long)i, a.seed);
  const float* row = a.table + 3 * (size_t)rt_ao_row(h, a.m, r);
  const float xyz[3] = {row[0], row[1], row[2]};
  float dd[3];
  rt_ao_dir(&f, xyz, h, dd);
  o = f3{__uint_as_float(w2.x), __uint_as_float(w2.y), __uint_as_float(w3.x)};
  d = f3{dd[0], dd[1], dd[2]};
  return true;
}

// A work item is a.spi whole samples (rt_ao_items.h): lane q k + r is ray r of
// the item's sample q for k <= 64; for k > 64 the item's one sample is walked
// in rt_ao_rounds(k) rounds of 64 rays, the count carried in a register.  A
// sample's count is the population count of its lanes in the ballot of hits;
// its lane with r == 0 stores it with one plain 4-byte store, whether or not
// the sample shot: every word [0, n) is written exactly once, none past n.
// The ray is formed anew in every round, before the walk's state is live.
template <int ACCEL, bool WIDE>
__global__ __launch_bounds__(64, RT_TRACE_MIN_WAVES) void ao_kernel(KParams p, AoArgs a) {
  const int lane = threadIdx.x & 63;
  WorkCount wc = {};
  __shared__ float4 s_stack[ACCEL == RT_ACCEL_FLAT_D ? 1 : kStackArea];
  __shared__ float4 s_stage[ACCEL == RT_ACCEL_FLAT_D ? kStageFlat : kStageOct];
  Stack stk;
  WaveCtx w;
  wave_state(p, s_stack, s_stage, lane, stk, w);
  // the lane's place in every item (worked out per item: a multiply and a
  // shift, rt_ao_lane_sample): sample lq of the item, and of that sample's
  // round ray lane - lq k; a lane from spi k up has no ray (k <= 64)
  constexpr bool wide = WIDE;  // k > 64 (the launch's choice): its own kernel, so k <= 64 has no round loop
  const uint64_t kmask = a.k >= 64u ? ~0ull : (1ull << a.k) - 1ull;  // a sample's lanes in a ballot, shifted down
  const uint32_t rounds = wide ? rt_ao_rounds(a.k) : 1u;
  const uint32_t tb = __float_as_uint(a.tmax);
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
    if (q >= rt_ray_stream_items(a.nitems, x)) {
      if (++probe == 8u) break;  // every stream drained: the wave exits
      continue;
    }
    const size_t i0 = (size_t)rt_ray_stream_item(q, x) * a.spi;  // the item's first sample
    uint64_t hits = 0;    // the last round's ballot
    uint32_t wcount = 0;  // k > 64: the sample's count so far (wave-uniform)
    for (uint32_t round = 0; round < rounds; round++) {
      // a lane without a query walks nothing, but its ray takes part in the
      // packet walk's wave-wide arithmetic: a harmless one
      f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
      float tmax = __builtin_inff();
      bool traced = false, query = false;
      {
        const uint32_t lq = wide ? 0u : rt_ao_lane_sample((uint32_t)lane, a.kinv);
        const uint32_t r = (uint32_t)lane - lq * a.k + 64u * round;
        const size_t i = i0 + (size_t)lq;
        f3 ro, rd;
        if ((wide || (uint32_t)lane < a.spi * a.k) && i < a.n && r < a.k && ao_ray(a, i, r, ro, rd)) {
          const uint32_t ob[3] = {__float_as_uint(ro.x), __float_as_uint(ro.y), __float_as_uint(ro.z)};
          const uint32_t db[3] = {__float_as_uint(rd.x), __float_as_uint(rd.y), __float_as_uint(rd.z)};
          traced = rt_occl_traced(ob, db, tb);
          query = rt_occl_queried(ob, db, tb);
          if (query) o = ro, d = rd, tmax = a.tmax;
        }
      }
      wc.pixels += (uint32_t)__popcll(__ballot(traced));  // the rays traced (rt_stats.camera of a batch)
      wc.shadow += (uint32_t)__popcll(__ballot(query));   // the queries
      const Ray ray = make_ray(p, o, d, p.eps_rel);
      hits = __ballot(occl_q<ACCEL>(p, ray, tmax, query, a.walk, stk, w, wc));
      if (wide) wcount += (uint32_t)__popcll(hits);
    }
    // the sample's first lane stores its count.  (Its place is worked out
    // again from an opaque copy of the lane: carried across the walk it costs
    // the walk registers.)
    uint32_t sl = (uint32_t)lane;
    asm volatile("" : "+v"(sl));
    const uint32_t sq = wide ? 0u : rt_ao_lane_sample(sl, a.kinv);
    const uint32_t sh = sq * a.k;
    const size_t i = i0 + (size_t)sq;
    if ((uint32_t)lane == sh && (wide || (uint32_t)lane < a.spi * a.k) && i < a.n)
      a.out[i] = wide ? wcount : (uint32_t)__popcll((hits >> sh) & kmask);
  }
  flush_counts(p, wc, lane, true);
}

// The generated rays themselves, one thread per ray j = i k + r: origin and
// direction in ray order, zeros for a sample that does not shoot (an all-zero
// direction is a ray no batch traces), and on request one byte per sample
// saying whether it shot.  (A template, like the other late kernels: emitted
// after every kernel that existed.)
template <int>
__global__ __launch_bounds__(256) void ao_rays_kernel(AoArgs a) {
  const unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n * a.k) return;
  const size_t i = (size_t)(j / a.k);
  const uint32_t r = (uint32_t)(j % a.k);
  f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 0.0f};
  const bool shot = ao_ray(a, i, r, o, d);
  float* po = a.org + 3 * (size_t)j;
  float* pd = a.dir + 3 * (size_t)j;
  po[0] = o.x, po[1] = o.y, po[2] = o.z;
  pd[0] = d.x, pd[1] = d.y, pd[2] = d.z;
  if (a.shot && r == 0u) a.shot[i] = shot ? 1 : 0;
}

}  // namespace rt
