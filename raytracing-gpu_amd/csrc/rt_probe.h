// rt_probe.h -- the query probes of tests and tools: probe_shadow_kernel and
// probe_closest_kernel (include/rt_hip_test.h, csrc/rt_verify.cpp).
// Part of rt_render.hip's one translation unit, included after shade_kernel:
// needs rt_query.h and rt_shading.h (included here) and kLaneStackArea.
#pragma once

#include "rt_query.h"
#include "rt_shading.h"

namespace rt {

// Shadow-query probe (tests, tools): the shadow ray of light li from each
// given origin (cpu/light.c:53,78), answered through the light's buffer
// (brute = 0) or by brute force over the nprim prim-order records (brute = 1,
// cpu/hit.c:93-109).  One thread per origin; out[i] = shadowed.
__global__ __launch_bounds__(256) void probe_shadow_kernel(KParams p, const float* __restrict__ org, uint32_t n,
                                                           uint32_t li, uint32_t nprim, int brute,
                                                           uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* L = p.light + RT_LIGHT_FLOATS_D * li;
  const uint32_t type = __float_as_uint(L[0]);
  const f3 o{org[3 * (size_t)i], org[3 * (size_t)i + 1], org[3 * (size_t)i + 2]};
  const Ray r = make_ray(p, o, shadow_dir(type, f3{L[4], L[5], L[6]}, o), p.eps_rel);
  bool hit = false;
  if (brute) {
    uint32_t risk = 0;
    for (uint32_t k = 0; k < nprim && !hit; k++) {
      const float4* t = p.tri_prim + 3 * (size_t)k;
      hit = any_hit_rec(r, t[0], t[1], t[2], risk);
    }
  } else {
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    hit = lbuf_any<false>(p, p.lbuf[li], r, lc);
  }
  out[i] = hit ? 1u : 0u;
}

// Closest-hit probe (tests, tools): ray i = (org[i], dir[i]) as a
// reflection ray queries it -- the per-lane octree walk at the secondary
// rays' culling slack (closest_q at depth > 0, default policy), or brute force
// over the nprim prim-order records (cpu/hit.c:72-91) -- out[2 i] = the
// winner's prim (~0: none), out[2 i + 1] = its new_dist bits.  One-wave
// workgroups: the walk's LDS stack is per wave, its spill area per lane.
__global__ __launch_bounds__(64) void probe_closest_kernel(KParams p, const float* __restrict__ org,
                                                           const float* __restrict__ dir, uint32_t n,
                                                           uint32_t nprim, int brute, uint32_t* __restrict__ out) {
  __shared__ float4 s_stack[kLaneStackArea];
  const int lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 64u + (uint32_t)lane;
  Stack stk;
  lane_stack(p, s_stack, lane, stk);
  const bool act = i < n;
  f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
  if (act) {
    o = f3{org[3 * (size_t)i], org[3 * (size_t)i + 1], org[3 * (size_t)i + 2]};
    d = f3{dir[3 * (size_t)i], dir[3 * (size_t)i + 1], dir[3 * (size_t)i + 2]};
  }
  const Ray r = make_ray(p, o, d, p.eps_rel);
  Best b = best_none();
  if (brute) {
    if (act)
      for (uint32_t k = 0; k < nprim; k++) {
        const float4* t = p.tri_prim + 3 * (size_t)k;
        consider(r, t[0], t[1], t[2], b);
      }
  } else {
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) {
      if (p.node_rf)  // the exact reflection mode's walk (rt_hip_set_exact_reflections)
        oct_closest_rf<false>(p, r, b, stk, lc);
      else
        oct_closest<false>(p, r, b, stk, lc);
    }
    if (act && lc.unproven) out[2 * (size_t)i + 1] = 0x7fc00001u;  // (never: |d| past RT_RF_DLMAX)
  }
  if (act) {
    out[2 * (size_t)i] = b.dist == __builtin_inff() ? 0xffffffffu : b.prim;
    out[2 * (size_t)i + 1] = __float_as_uint(b.dist);
  }
}

}  // namespace rt
