// rt_lightbuf_cell.h -- the query's half of the light buffers' contract
// (rt_lightbuf.h, DESIGN.md §4 "Light buffers"): the cells a shadow ray looks
// up and the key limit of the first.  The build's margins (0.01 cs and 0.02
// cells around a footprint, 6 eps s1 on a key; rt_lightbuf_geom.h) are sized
// for exactly these float operations in this order, without contraction.
// __host__ __device__: the shade kernels call it through lbuf_range
// (rt_query.h), tests/native/lightbuf_geom.cpp on the CPU.
#pragma once

#include <cmath>
#include <cstdint>

#include "rt_lightbuf.h"

// The cells of the shadow ray (o, d) and the key limit of cell[0] (cell[1]:
// none), written where the ray has them: the caller starts from cell[0] =
// cell[1] = 0xffffffff (none) and lim = inf.  (Returned through the arguments
// and not as a struct: the shade kernels' register allocation differs
// otherwise.)  V3: any vector of floats x, y, z (rt::f3 on the device).
template <class V3>
__host__ __device__ __forceinline__ void lbuf_cells(const RtLightBuf& L, const V3& o, const V3& d, uint32_t cell[2],
                                                    float& lim) {
  if (L.kind == RT_LB_DIR) {
    // the same float operations the build's margins assume (no contraction)
    const float pu = o.x * L.u[0] + o.y * L.u[1] + o.z * L.u[2];
    const float pv = o.x * L.v[0] + o.y * L.v[1] + o.z * L.v[2];
    const float pw = o.x * L.w[0] + o.y * L.w[1] + o.z * L.w[2];
    const float fx = (pu - L.u0) * L.inv_cs, fy = (pv - L.v0) * L.inv_cs;
    if (fx >= 0.0f && fy >= 0.0f && fx < (float)L.nx && fy < (float)L.ny) {
      cell[0] = (uint32_t)fy * L.nx + (uint32_t)fx;
      lim = -pw;  // keys are minus the triangles' depth bounds toward the light
    }
  } else {
    // from the light to the origin: -d, the ray's own direction negated
    const V3 x{-d.x, -d.y, -d.z};
    const float ax = fabsf(x.x), ay = fabsf(x.y), az = fabsf(x.z);
    uint32_t a = 0;
    float m = ax, xa = x.x, xj = x.y, xk = x.z;
    if (ay > m) {
      a = 1;
      m = ay;
      xa = x.y;
      xj = x.z;
      xk = x.x;
    }
    if (az > m) {
      a = 2;
      m = az;
      xa = x.z;
      xj = x.x;
      xk = x.y;
    }
    if (m > 0.0f) {
      const uint32_t n = L.nx;
      const float sc = xj / m, tc = xk / m;
      const uint32_t f = 2u * a + (xa < 0.0f ? 1u : 0u);
      const auto umin = [](uint32_t p, uint32_t q) { return p < q ? p : q; };
      const uint32_t ix = umin((uint32_t)((sc + 1.0f) * L.half_n), n - 1u);
      const uint32_t iy = umin((uint32_t)((tc + 1.0f) * L.half_n), n - 1u);
      const uint32_t jx = umin((uint32_t)((1.0f - sc) * L.half_n), n - 1u);
      const uint32_t jy = umin((uint32_t)((1.0f - tc) * L.half_n), n - 1u);
      cell[0] = (f * n + iy) * n + ix;
      cell[1] = ((f ^ 1u) * n + jy) * n + jx;
      // |x| as rt_device.h's length(): float sum, double sqrt, cast to float
      const float s = x.x * x.x + x.y * x.y + x.z * x.z;
      lim = (float)__builtin_sqrt((double)s) * (1.0f + 1e-6f);  // keys: nearest distance from the light
    }
  }
}
