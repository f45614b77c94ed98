// rt_dlight.h -- direct light for caller's surface records on the device
// (include/rt_hip.h rt_hip_direct_light): for every rt_gsample record the three
// channels of apply_light (cpu/light.c:33-100) at the record's (P, N) with its
// object's material, and on request the mask of the casting lights whose
// shadow ray is unoccluded.  The shadow rays are shade_record's (shadow_dir),
// the sum is lights_sum of rt_shading.h, unchanged; what is new is that the
// records are a caller's, so their origins may lie anywhere: each (record,
// light) is decided through the light's buffer when P lies in the buffer's
// proof box, and by the occlusion batches' walks otherwise -- nothing is
// deferred.  dlight_kernel has the shape of rays_occl_kernel / ao_kernel.
// Part of rt_render.hip's one translation unit, after rt_ao.h; its launch is
// csrc/rt_dlight.cpp; which records shade: csrc/rt_dlight_items.h.
#pragma once

#include "rt_dlight_items.h"

namespace rt {

// Record i as ao_ray loads it: five 8-byte pairs prim obj | queries dist |
// P.x P.y | P.z N.x | N.y N.z.  False (and P = N = 0, obj = 0) when the record
// does not shade.
__device__ __forceinline__ bool dlight_record(const DlArgs& a, size_t i, f3& P, f3& N, uint32_t& obj) {
  const uint2* s = a.samples + 5 * i;
  const uint2 w0 = s[0], w2 = s[2], w3 = s[3], w4 = s[4];
  const uint32_t pb[3] = {w2.x, w2.y, w3.x}, nb[3] = {w3.y, w4.x, w4.y};
  P = N = f3{0.0f, 0.0f, 0.0f};
  obj = 0;
  if (!rt_dl_shades((int)w0.x, (int)w0.y, a.nobj, pb, nb)) return false;
  P = f3{__uint_as_float(pb[0]), __uint_as_float(pb[1]), __uint_as_float(pb[2])};
  N = f3{__uint_as_float(nb[0]), __uint_as_float(nb[1]), __uint_as_float(nb[2])};
  obj = w0.y;
  return true;
}

// has_direct_hit (cpu/light.c:24-31) of ray r for the lanes of `act` by the
// walks of an occlusion batch with no distance bound: occl_q's routes with the
// bound's two words +inf as constants (occl_bound would divide +inf by |d|:
// NaN for a direction whose length overflows).  Unlike a batch, every ray is
// asked, a zero or huge direction too: the reference asks them, and they end
// in mt_candidate's |a| < 1e-7 or t < 1e-7 on every route.
// walk is wave-uniform.  Converged call.
template <int ACCEL>
__device__ __forceinline__ bool dlight_q(const KParams& p, const Ray& r, bool act, uint32_t walk, Stack& s,
                                         WaveCtx& w, WorkCount& wc) {
  const OcclBound ob{__builtin_inff(), __builtin_inff()};
  if (ACCEL == RT_ACCEL_FLAT_D) return use_tp(p, act) ? flat_occl_tp(p, r, ob, act, wc) : flat_occl_w(p, r, ob, act, w, wc);
  return occl_oct<false>(p, r, ob, act, walk, s, w, wc);  // the exact route: any winner shadows
}

// Phase 1 of a chunk of 32 lights: the mask of the chunk's casting lights that
// do not shadow P (bit li - l0), light by light with a wave-uniform li.  Only P
// is live across the queries.  Route per lane: brute force on FLAT; the
// light's buffer when it has one and P lies in its proof box (lbuf_scan, the
// shade pass's scan, proven for origins in that box); dlight_q otherwise, those
// of a buffered light counted in wc.hits (rt_stats.shadow_deferred of the call).
template <int ACCEL>
__device__ __forceinline__ uint32_t dlight_mask(const KParams& p, bool shades, f3 P, uint32_t l0, uint32_t l1,
                                                uint32_t walk, Stack& s, WaveCtx& w, WorkCount& wc) {
  uint32_t lit = 0;
  for (uint32_t li = l0; li < l1; li++) {
    const LightShade L = LightRowsUniform{p.lshade}[li];
    const uint32_t type = L.type;
    if (type != 1 && type != 2) continue;
    wc.shadow += (uint32_t)__popcll(__ballot(shades));
    // the shadow ray; a lane without a query carries a harmless one through
    // the packet walk's wave-wide arithmetic
    const f3 d = shades ? shadow_dir(type, L.v, P) : f3{0.0f, 0.0f, 1.0f};
    f3 nd;
    Ray r;
    if (type == 1 && shades) {  // |d| and d / |d| from the light's row: the same operations, done once
      r = make_ray_len(p, P, d, L.dlen, p.eps_rel);
      nd = L.nd;
    } else {
      r = make_ray(p, P, d, p.eps_rel);
      nd = unit_dir(r);
    }
    bool hit = false, walks = shades;
    if (ACCEL != RT_ACCEL_FLAT_D && p.lbuf) {
      const RtLightBuf Lb = lbuf_desc(p.lbuf, li);
      if (Lb.kind != RT_LB_NONE) {  // wave-uniform
        const float Pv[3] = {P.x, P.y, P.z};
        const bool in = shades && rt_dl_in_box(Pv, Lb.olo, Lb.ohi);
        LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
        if (in) hit = lbuf_scan<false>(p, Lb, r, nd, lbuf_range(Lb, r), lc);
        absorb<false>(wc, lc, true);
        walks = shades && !in;
        wc.hits += (uint32_t)__popcll(__ballot(walks));
      }
    }
    if (__ballot(walks)) hit = dlight_q<ACCEL>(p, r, walks, walk, s, w, wc) || hit;
    if (shades && !hit) lit |= 1u << (li - l0);
  }
  return lit;
}

// A work item is 64 consecutive records, lane = record, on rays_occl_kernel's
// persistent one-wave workgroups and 8 item streams (rt_ray_items.h).  Per
// chunk of 32 lights: the shadow decisions (dlight_mask; the walk's state is
// live, the record's N and material are not loaded yet), then the record loaded
// again and lights_sum over the same chunk with that mask (the Phong
// temporaries live, the walk's state dead).  The lane stores its three colour
// words and, if asked, the first chunk's mask: every word of [0, n) is written
// exactly once, none past n.
template <int ACCEL>
__global__ __launch_bounds__(64, RT_TRACE_MIN_WAVES) void dlight_kernel(KParams p, DlArgs a) {
  const int lane = threadIdx.x & 63;
  WorkCount wc = {};
  __shared__ float4 s_stack[ACCEL == RT_ACCEL_FLAT_D ? 1 : kStackArea];
  __shared__ float4 s_stage[ACCEL == RT_ACCEL_FLAT_D ? kStageFlat : kStageOct];
  Stack stk;
  WaveCtx w;
  wave_state(p, s_stack, s_stage, lane, stk, w);
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
    const size_t i0 = (size_t)rt_ray_stream_item(q, x) * RT_RAY_ITEM;  // the item's first record
    const size_t i = i0 + (size_t)lane;
    const bool in = i < a.n;
    bool shades = false;
    f3 P{0.0f, 0.0f, 0.0f};
    {
      f3 N;
      uint32_t obj;
      if (in) shades = dlight_record(a, i, P, N, obj);
    }
    wc.pixels += (uint32_t)__popcll(__ballot(shades));  // the records that shade (rt_stats.camera of the call)
    col acc = init_color(0.0f, 0.0f, 0.0f);
    uint32_t lit0 = 0;
    for (uint32_t l0 = 0; l0 < p.nlight; l0 += 32) {
      const uint32_t l1 = p.nlight - l0 < 32u ? p.nlight : l0 + 32u;
      const uint32_t lit = dlight_mask<ACCEL>(p, shades, P, l0, l1, a.walk, stk, w, wc);
      if (l0 == 0) lit0 = lit;
      if (!shades) continue;
      // (the record again: carried across the walks, N and the object would
      // cost the walks their registers)
      f3 Pr, N;
      uint32_t obj;
      uint32_t sl = (uint32_t)lane;
      asm volatile("" : "+v"(sl));
      (void)dlight_record(a, i0 + (size_t)sl, Pr, N, obj);
      const float* ms = p.mshade + RT_MAT_FLOATS_D * (size_t)obj;
      acc = lights_sum(LightRowsUniform{p.lshade}, acc, l0, l1, lit, ms, Pr, N);
    }
    if (in) {
      float* o = a.rgb + 3 * i;
      o[0] = acc.r, o[1] = acc.g, o[2] = acc.b;
      if (a.lit) a.lit[i] = lit0;
    }
  }
  flush_counts(p, wc, lane, true);
}

}  // namespace rt
