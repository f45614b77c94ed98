// rt_shading.h -- Phong shading of cpu/light.c: the specular term (spec_pow,
// specular), a light's shadow-ray direction and unshadowed contribution
// (shadow_dir, light_lit) and the light loop with its shadow queries
// (apply_light).
// Part of rt_render.hip's one translation unit.  Needs rt_query.h (included
// here: shadow_q).
#pragma once

#include "rt_query.h"

namespace rt {

// pow of cpu/light.c:20, out of line: inlined, its f64 polynomial
// coefficients were hoisted out of the path loop and spilled to scratch.
#ifndef RT_SPEC_POW_INLINE
#define RT_SPEC_POW_INLINE __noinline__
#endif
__device__ RT_SPEC_POW_INLINE float spec_pow(double x, double e) { return (float)pow(fmax(x, 0.0), e); }

// cpu/light.c:7-22
__device__ __forceinline__ col specular(col tmp, f3 inc_o, f3 inc_d, f3 P, f3 N, const float* m) {
  col k = init_color(m[6], m[7], m[8]);
  f3 V = sub(inc_o, P);
  f3 R = sub(inc_d, scale(N, 2.0f * dot(N, inc_d)));
  R = normalize(R);
  V = normalize(V);
  float ls = spec_pow((double)dot(R, V), (double)m[9]);
  k = color_mul(k, ls);
  return color_add(tmp, k);
}

// Shadow-ray direction of a directional (type 1) or point (type 2) light at
// P: cpu/light.c:53,78 (unnormalised).
__device__ __forceinline__ f3 shadow_dir(uint32_t type, f3 lv, f3 P) {
  return type == 1 ? scale(lv, -1.0f) : sub(lv, P);
}

// The unshadowed contribution of a directional or point light,
// cpu/light.c:49-66 and 68-98; P = hit point, N = interpolated (unnormalised)
// normal, m = material.
__device__ __forceinline__ col light_lit(uint32_t type, col lc, f3 lv, const float* m, f3 P,
                                         f3 N) {
  if (type == 1) {  // DIRECTIONAL
    f3 Ldir = scale(lv, -1.0f);
    col tmp = color_mul2(lc, init_color(m[3], m[4], m[5]));
    tmp = color_mul(tmp, dot(Ldir, N));
    f3 inc_o = add(P, scale(lv, -10.0f));
    return specular(tmp, inc_o, lv, P, N, m);
  }
  // POINT: "L" is minus the light position
  f3 to_l = sub(lv, P);
  f3 Lp = scale(lv, -1.0f);
  f3 Nf = N;
  if (dot(Lp, Nf) < 0.0f) Nf = scale(Nf, -1.0f);
  float dist = length(sub(lv, P));
  col tmp = color_mul2(lc, init_color(m[3], m[4], m[5]));
  tmp = color_mul(tmp, dot(Lp, Nf) * 1.0f / dist);
  f3 inc_o = add(P, scale(to_l, -10.0f));
  return specular(tmp, inc_o, to_l, P, N, m);
}

// The lights l0 .. l1 - 1 of a record summed onto acc in the file order of the
// lights (light = the table, RT_LIGHT_FLOATS_D floats each, in global memory
// or staged in LDS), as cpu/light.c:33-100 does: an ambient light's term, and a
// directional or point light's when bit li - l0 of `lit` says no shadow ray hit.
// The one per-record sum of shade_record's second phase, oob_reshade_kernel
// and recolour_kernel (rt_recolour.h), so the three cannot drift.
__device__ __forceinline__ col lights_sum(const float* light, col acc, uint32_t l0, uint32_t l1, uint32_t lit,
                                          const float* m, f3 P, f3 N) {
  for (uint32_t li = l0; li < l1; li++) {
    const float* L = light + RT_LIGHT_FLOATS_D * li;
    const uint32_t type = __float_as_uint(L[0]);
    const col lc = init_color(L[1], L[2], L[3]);
    if (type == 0)  // AMBIENT
      acc = color_add(acc, color_mul2(lc, init_color(m[0], m[1], m[2])));
    else if ((type == 1 || type == 2) && ((lit >> (li - l0)) & 1u))
      acc = color_add(acc, light_lit(type, lc, f3{L[4], L[5], L[6]}, m, P, N));
  }
  return acc;
}

// cpu/light.c:33-100 for the lanes with hit.  The light loop is wave-uniform
// so shadow queries run converged.
template <int ACCEL, bool COUNT, int POL>
__device__ col apply_light(const KParams& p, bool hit, const float* m, f3 P, f3 N, Stack& s,
                           WaveCtx& w, WorkCount& wc) {
  col acc = init_color(0.0f, 0.0f, 0.0f);
  for (uint32_t li = 0; li < p.nlight; li++) {
    const float* L = p.light + RT_LIGHT_FLOATS_D * li;
    uint32_t type = __float_as_uint(L[0]);
    col lc = init_color(L[1], L[2], L[3]);
    f3 lv = f3{L[4], L[5], L[6]};
    if (type == 0) {  // AMBIENT
      if (hit) acc = color_add(acc, color_mul2(lc, init_color(m[0], m[1], m[2])));
    } else if (type == 1 || type == 2) {
      const uint64_t c0 = COUNT ? __builtin_readcyclecounter() : 0ull;
      bool sh = shadow_q<ACCEL, COUNT, POL>(p, P, shadow_dir(type, lv, P), type, li, hit, s, w, wc);
      if (COUNT) {
        const uint32_t dc = (uint32_t)(__builtin_readcyclecounter() - c0);
        wc.cy_shadow += dc;
        if (type == 1) wc.cy_shadow_dir += dc;
      }
      if (hit && !sh) acc = color_add(acc, light_lit(type, lc, lv, m, P, N));
    }
  }
  return acc;
}

}  // namespace rt
