// rt_shade_rows.h -- the shading tables' rows (KParams::mshade, KParams::lshade)
// and how the kernels read them.  The tables hold what the shade pass needs of
// a material or a light and what cpu/light.c computes from the row alone, the
// same float operations in the same order, performed once per row by
// shade_tables_kernel (rt_shade_tables.h) instead of once per record or query.
//
//   material row, RT_MAT_FLOATS_D floats as KParams::mat:
//     [0..8]  chan(m[i]) / 255.0f   (ka, kd, ks as color_mul2 / color_mul take them)
//     [9]     the specular exponent, [10] nr, [11] as mat
//   light row, RT_LSHADE_FLOATS_D floats (LightShade below, in its order):
//     [0]      the type's bits
//     [1..3]   chan(L[1..3]) / 255.0f
//     [4..6]   v
//     directional lights only (zeros otherwise) -- every shadow ray of one has
//     the direction d = scale(v, -1) (cpu/light.c:53):
//     [7]      dlen = length(d)
//     [8..10]  d / dlen, the three quotients of hit_point (rt_isect.h)
//     [11..13] scale(v, -10) (cpu/light.c:57)
//
// The tables are written by a kernel that has ended before any reader starts
// and by nothing else, so a wave-uniform row may be read through the constant
// address space (scalar loads into SGPRs); the same holds for the light
// buffers' descriptors (KParams::lbuf) and the pointers in them, and does not
// hold for the counters the kernels add to.
// Part of rt_render.hip's one translation unit.  Needs rt_walk_wave.h (ldu).
#pragma once

#include "rt_kernels.h"
#include "rt_walk_wave.h"

namespace rt {

struct LightShade {
  uint32_t type;
  float cr, cg, cb;
  f3 v;
  float dlen;
  f3 nd, back;
};

__device__ __forceinline__ LightShade light_shade_of(const float4& a, const float4& b, const float4& c,
                                                     const float4& d) {
  LightShade s;
  s.type = __float_as_uint(a.x);
  s.cr = a.y, s.cg = a.z, s.cb = a.w;
  s.v = f3{b.x, b.y, b.z};
  s.dlen = b.w;
  s.nd = f3{c.x, c.y, c.z};
  s.back = f3{c.w, d.x, d.y};
  return s;
}
__device__ __forceinline__ void light_shade_store(float* row, const LightShade& s) {
  float4* r = (float4*)row;
  r[0] = make_float4(__uint_as_float(s.type), s.cr, s.cg, s.cb);
  r[1] = make_float4(s.v.x, s.v.y, s.v.z, s.dlen);
  r[2] = make_float4(s.nd.x, s.nd.y, s.nd.z, s.back.x);
  r[3] = make_float4(s.back.y, s.back.z, 0.0f, 0.0f);
}

// Row li of a table in global memory, li wave-uniform: scalar loads.
struct LightRowsUniform {
  const float* tab;
  __device__ __forceinline__ LightShade operator[](uint32_t li) const {
    const float4* r = (const float4*)tab + (RT_LSHADE_FLOATS_D / 4) * (size_t)li;
    return light_shade_of(ldu(r, 0), ldu(r, 1), ldu(r, 2), ldu(r, 3));
  }
};
// Row li through ordinary loads (a table staged in LDS).
struct LightRowsMem {
  const float4* tab;
  __device__ __forceinline__ LightShade operator[](uint32_t li) const {
    const float4* r = tab + (RT_LSHADE_FLOATS_D / 4) * (size_t)li;
    return light_shade_of(r[0], r[1], r[2], r[3]);
  }
};

// A light's buffer descriptor, li wave-uniform, by value through the constant
// address space: its fields arrive in SGPRs.
__device__ __forceinline__ RtLightBuf lbuf_desc(const RtLightBuf* lbuf, uint32_t li) {
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(sizeof(RtLightBuf) % sizeof(uint32_t) == 0, "copied word by word");
  typedef const __attribute__((address_space(4))) uint32_t cword;
  const cword* src = (const cword*)(lbuf + li);
  uint32_t w[sizeof(RtLightBuf) / sizeof(uint32_t)];
#pragma unroll
  for (uint32_t k = 0; k < sizeof(RtLightBuf) / sizeof(uint32_t); k++) w[k] = src[k];
  RtLightBuf L;
  __builtin_memcpy(&L, w, sizeof L);
  return L;
#else
  return lbuf[li];  // host pass only parses device code
#endif
}

}  // namespace rt
