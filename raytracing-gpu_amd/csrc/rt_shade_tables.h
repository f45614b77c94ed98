// rt_shade_tables.h -- shade_tables_kernel: the shading tables
// (rt_shade_rows.h) derived from the raw material and light rows on the
// device, by the rt_device.h functions the shade pass itself called on those
// rows before: no host arithmetic has to equal the device's.  Launched by the
// host wherever it uploads KParams::mat or KParams::light (rt_hip.cpp).
// Part of rt_render.hip's one translation unit (a template so that it is
// emitted after every render kernel, as rt_recolour.h's).
#pragma once

#include "rt_shade_rows.h"

namespace rt {

// Thread t: light row t (t < nlight) and material row t (t < nobj).
template <int K = 0>
__global__ __launch_bounds__(256) void shade_tables_kernel(const float* light, uint32_t nlight, float* lshade,
                                                           const float* mat, uint32_t nobj, float* mshade) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nlight) {
    const float* L = light + RT_LIGHT_FLOATS_D * (size_t)t;
    const col lc = init_color(L[1], L[2], L[3]);
    LightShade s;
    s.type = __float_as_uint(L[0]);
    s.cr = lc.r / 255.0f, s.cg = lc.g / 255.0f, s.cb = lc.b / 255.0f;  // color_mul2's first factor
    s.v = f3{L[4], L[5], L[6]};
    s.dlen = 0.0f;
    s.nd = s.back = f3{0.0f, 0.0f, 0.0f};
    if (s.type == 1) {  // DIRECTIONAL: shadow_dir, make_ray, hit_point; light_lit's inc_o
      const f3 d = scale(s.v, -1.0f);
      s.dlen = length(d);
      s.nd = f3{d.x / s.dlen, d.y / s.dlen, d.z / s.dlen};
      s.back = scale(s.v, -10.0f);
    }
    light_shade_store(lshade + RT_LSHADE_FLOATS_D * (size_t)t, s);
  }
  if (t < nobj) {
    const float* m = mat + RT_MAT_FLOATS_D * (size_t)t;
    float* ms = mshade + RT_MAT_FLOATS_D * (size_t)t;
#pragma unroll
    for (int g = 0; g < 3; g++) {  // ka, kd, ks: color_mul2's second factor, color_mul's first
      const col k = init_color(m[3 * g], m[3 * g + 1], m[3 * g + 2]);
      ms[3 * g] = k.r / 255.0f, ms[3 * g + 1] = k.g / 255.0f, ms[3 * g + 2] = k.b / 255.0f;
    }
    ms[9] = m[9], ms[10] = m[10], ms[11] = m[11];
  }
}

}  // namespace rt
