// rt_dlight_items.h -- the arithmetic of direct light for caller's records
// (rt_hip_direct_light, csrc/rt_dlight.h, csrc/rt_dlight.cpp) that needs no
// device: which records shade, by the bits of their words, and whether a point
// lies in a light buffer's proof box (the route of its shadow query).  Items
// and streams are a ray batch's (rt_ray_items.h): 64 consecutive records, lane
// = record.  Plain C++ (host and device): the kernel, the host layer and
// tests/native/dlight_items.cpp include it; rtgpu.direct_light_shades is its
// numpy twin.
#pragma once

#include <stdint.h>

#include "rt_ray_items.h"

// A record shades iff it is a hit (prim >= 0) of an object of the context
// (0 <= obj < nobj), every component of P and N is finite, and N is not zero
// by the reference's vector3_is_zero (x == 0 && y == 0 && z == 0: -0.0 is
// zero, a denormal is not).  P and N by their bits: no libm, the same test
// everywhere.  Every other record -- a miss, the G-buffer's zero-normal winner
// (P = N = 0), a record a ray batch would not trace -- gets colour 0 0 0 and
// mask 0.
RT_TILES_FN int rt_dl_shades(int prim, int obj, uint32_t nobj, const uint32_t P[3], const uint32_t N[3]) {
  int fin = 1;
  for (int a = 0; a < 3; a++) fin = fin && rt_ray_finite_bits(P[a]) && rt_ray_finite_bits(N[a]);
  const int zero = !((N[0] | N[1] | N[2]) & 0x7fffffffu);
  return prim >= 0 && obj >= 0 && (uint32_t)obj < nobj && fin && !zero;
}

// P inside the closed box lo..hi (a light buffer's proof box, RtLightBuf::olo,
// ohi): the negation of the shade pass's "off the box" test, so a NaN bound or
// coordinate is outside.
RT_TILES_FN int rt_dl_in_box(const float P[3], const float lo[3], const float hi[3]) {
  return P[0] >= lo[0] && P[0] <= hi[0] && P[1] >= lo[1] && P[1] <= hi[1] && P[2] >= lo[2] && P[2] <= hi[2];
}
