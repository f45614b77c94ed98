// rt_recolour.h -- the relight's own kernels (rt_hip_relight, rt_hip.cpp):
// relight_zero_kernel, which clears what a shade pass adds to and nothing of
// the trace's, and recolour_kernel, the whole shade pass of a relight in which
// no light is dirty (csrc/rt_relight.h): every kept hit record's lights summed
// again from its stored unshadowed-light mask, no shadow query.
// Part of rt_render.hip's one translation unit (templates only so that they are
// emitted after every render kernel, which keep their places; the
// per-record sum is shade_record's and oob_reshade_kernel's: lights_sum,
// rt_shading.h).
#pragma once

#include "rt_shading.h"

namespace rt {

// The stat slots a shade pass adds to.  rt_counters.h's list decides them
// (rt_stat_shade_side); this chain only has to agree with it, and is kept in
// this shape -- the single slots, then the run as a range -- because the
// compiler's code for relight_zero_kernel follows the shape of the expression.
constexpr bool shade_stat_slot(uint32_t k) {
  return k == RT_ST_SHADOW || k == RT_ST_SHADOW_NODE_LANES || k == RT_ST_SHADOW_TRI_LANES ||
         k == RT_ST_CYCLES_SHADOW || k == RT_ST_CYCLES_SHADOW_DIRECTIONAL ||
         (k >= RT_ST_SHADOW_ZERO_RISK && k <= RT_ST_SHADOW_UNPROVEN);
}
constexpr bool shade_stat_slots_agree(uint32_t k = 0) {
  return k == RT_STAT_STRIDE || (shade_stat_slot(k) == rt_stat_shade_side(k) && shade_stat_slots_agree(k + 1));
}
static_assert(shade_stat_slots_agree(), "shade_stat_slot differs from the SHADE rows of RT_STAT_LIST");

// One workgroup: the RT_HIT_REGIONS shade chunk counters (RT_HIT_STRIDE apart)
// and the shade-side stat slots of every copy.  The hit-record counters, the item
// streams, the trace's stats and its cost sum stay: they are the traced
// frame's.
template <int K = 0>
__global__ __launch_bounds__(256) void relight_zero_kernel(KParams p) {
  static_assert(RT_HIT_REGIONS * RT_HIT_STRIDE <= 256 && RT_STAT_SETS * RT_STAT_STRIDE <= 256,
                "one workgroup covers both");
  const uint32_t t = threadIdx.x;
  if (t < RT_HIT_REGIONS * RT_HIT_STRIDE) p.shade_counter[t] = 0u;
  if (t < RT_STAT_SETS * RT_STAT_STRIDE && shade_stat_slot(t % RT_STAT_STRIDE)) p.stats[t] = 0ull;
}

// lights a workgroup stages in LDS (their shading rows, RT_LSHADE_FLOATS_D
// floats each); a longer table is read from global memory instead
static constexpr uint32_t kRecolourLights = 64;

// A record's local colour under `nlight` lights from its stored mask (lights
// 0..31; a casting light from index 32 up has no bit and the host never takes
// this path with one): shade_record's blocks of 32 in the same order.
template <class Rows>
__device__ __forceinline__ col recolour_sum(const Rows& rows, uint32_t nlight, uint32_t mask, const float* ms,
                                            f3 P, f3 N) {
  col acc = init_color(0.0f, 0.0f, 0.0f);
  for (uint32_t l0 = 0; l0 < nlight; l0 += 32) {
    const uint32_t l1 = nlight - l0 < 32u ? nlight : l0 + 32u;
    acc = lights_sum(rows, acc, l0, l1, l0 == 0 ? mask : 0u, ms, P, N);
  }
  return acc;
}

// One lane per kept record, grid-stride over the records of the 8 regions in
// region order (their counts read here: min(hit_count, hit_cap), no host
// read-back): 2 float4 of the record and its mask word in, the term
// color_mul(local, coef) (cpu/raytracer.c:30) out -- 36 B read, 16 B written.
// The light table is staged in LDS once per workgroup; a record's material
// row (10 floats of 48 B, gathered by object) comes through the vector cache.
template <int K = 0>
__global__ __launch_bounds__(256) void recolour_kernel(KParams p) {
  __shared__ float4 s_light[kRecolourLights * RT_LSHADE_FLOATS_D / 4];
  const bool staged = p.nlight <= kRecolourLights;
  if (staged)
    for (uint32_t i = threadIdx.x; i < p.nlight * (RT_LSHADE_FLOATS_D / 4); i += blockDim.x)
      s_light[i] = ((const float4*)p.lshade)[i];
  __syncthreads();
  uint32_t end[RT_HIT_REGIONS];  // exclusive ends of the regions in the flattened order (wave-uniform)
  uint32_t total = 0;
#pragma unroll
  for (int x = 0; x < RT_HIT_REGIONS; x++) {
    const uint32_t hc = p.hit_count[RT_HIT_STRIDE * x];
    total += hc < p.hit_cap ? hc : p.hit_cap;
    end[x] = total;
  }
  // (8 regions of at most 2^29 - 1 records: the flattened index fits 32 bits)
  const uint32_t nth = gridDim.x * blockDim.x;
  for (uint64_t g64 = blockIdx.x * blockDim.x + threadIdx.x; g64 < total; g64 += nth) {  // (no 32-bit wrap near 2^32)
    const uint32_t g = (uint32_t)g64;
    uint32_t x = 0, first = 0;
#pragma unroll
    for (int k = 0; k < RT_HIT_REGIONS - 1; k++)
      if (g >= end[k]) {
        x = k + 1;
        first = end[k];
      }
    const size_t a = (size_t)x * p.hit_cap + (g - first);
    const float4 r0 = p.hit[2 * a], r1 = p.hit[2 * a + 1];
    const uint32_t mask = p.hit_lit[a];
    const f3 P{r0.x, r0.y, r0.z}, N{r0.w, r1.x, r1.y};
    const float* ms = p.mshade + RT_MAT_FLOATS_D * (size_t)__float_as_uint(r1.w);
    const col local = staged ? recolour_sum(LightRowsMem{s_light}, p.nlight, mask, ms, P, N)
                             : recolour_sum(LightRowsUniform{p.lshade}, p.nlight, mask, ms, P, N);
    const col tm = color_mul(local, r1.z);  // coef
    p.hit_term[a] = make_float4(tm.r, tm.g, tm.b, 0.0f);
  }
}

}  // namespace rt
