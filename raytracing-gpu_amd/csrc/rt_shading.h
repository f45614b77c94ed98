// rt_shading.h -- Phong shading of cpu/light.c: the specular term (spec_pow,
// specular), a light's shadow-ray direction and unshadowed contribution
// (shadow_dir, light_lit) and a record's sum over the lights (lights_sum).
// The constants of a light and of a material come from the shading tables
// (rt_shade_rows.h).
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

// cpu/light.c:7-22; ms = the material's shading row (rt_shade_rows.h): its
// [6..8] are init_color(ks)'s channels over 255, the first factor of
// color_mul(k, ls)
__device__ __forceinline__ col specular(col tmp, f3 inc_o, f3 inc_d, f3 P, f3 N, const float* ms) {
  f3 V = sub(inc_o, P);
  f3 R = sub(inc_d, scale(N, 2.0f * dot(N, inc_d)));
  R = normalize(R);
  V = normalize(V);
  float ls = spec_pow((double)dot(R, V), (double)ms[9]);
  col k = init_color(ms[6] * ls, ms[7] * ls, ms[8] * ls);
  return color_add(tmp, k);
}

// Shadow-ray direction of a directional (type 1) or point (type 2) light at
// P: cpu/light.c:53,78 (unnormalised).
__device__ __forceinline__ f3 shadow_dir(uint32_t type, f3 lv, f3 P) {
  return type == 1 ? scale(lv, -1.0f) : sub(lv, P);
}

// The unshadowed contribution of a directional or point light,
// cpu/light.c:49-66 and 68-98; P = hit point, N = interpolated (unnormalised)
// normal, L and ms = the light's and the material's shading rows:
// color_mul2(lc, init_color(kd)) is init_color of the products of their
// channels over 255, which the rows hold.
__device__ __forceinline__ col light_lit(const LightShade& L, const float* ms, f3 P, f3 N) {
  const f3 lv = L.v;
  col tmp = init_color(L.cr * ms[3], L.cg * ms[4], L.cb * ms[5]);
  if (L.type == 1) {  // DIRECTIONAL
    f3 Ldir = scale(lv, -1.0f);
    tmp = color_mul(tmp, dot(Ldir, N));
    f3 inc_o = add(P, L.back);
    return specular(tmp, inc_o, lv, P, N, ms);
  }
  // POINT: "L" is minus the light position
  f3 to_l = sub(lv, P);
  f3 Lp = scale(lv, -1.0f);
  f3 Nf = N;
  if (dot(Lp, Nf) < 0.0f) Nf = scale(Nf, -1.0f);
  float dist = length(sub(lv, P));
  tmp = color_mul(tmp, dot(Lp, Nf) * 1.0f / dist);
  f3 inc_o = add(P, scale(to_l, -10.0f));
  return specular(tmp, inc_o, to_l, P, N, ms);
}

// The lights l0 .. l1 - 1 of a record summed onto acc in the file order of the
// lights (rows = the light shading table: LightRowsUniform in global memory,
// LightRowsMem staged in LDS), as cpu/light.c:33-100 does: an ambient light's
// term, and a directional or point light's when bit li - l0 of `lit` says no
// shadow ray hit.  ms = the material's shading row.
// The one per-record sum of shade_record's second phase, oob_reshade_kernel
// and recolour_kernel (rt_recolour.h), so the three cannot drift.
template <class Rows>
__device__ __forceinline__ col lights_sum(const Rows& rows, col acc, uint32_t l0, uint32_t l1, uint32_t lit,
                                          const float* ms, f3 P, f3 N) {
  for (uint32_t li = l0; li < l1; li++) {
    const LightShade L = rows[li];
    if (L.type == 0)  // AMBIENT
      acc = color_add(acc, init_color(L.cr * ms[0], L.cg * ms[1], L.cb * ms[2]));
    else if ((L.type == 1 || L.type == 2) && ((lit >> (li - l0)) & 1u))
      acc = color_add(acc, light_lit(L, ms, P, N));
  }
  return acc;
}

}  // namespace rt
