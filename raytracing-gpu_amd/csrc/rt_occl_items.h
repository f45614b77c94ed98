// rt_occl_items.h -- the arithmetic of an occlusion batch (rt_hip_occluded,
// csrc/rt_occl.h, csrc/rt_occl.cpp) that needs no device: which rays are
// traced and which of them make a query, by the bits of their floats, and the
// parametric bound t_cut a record's prefilter may use for a distance bound
// tmax.  Items and streams are a ray batch's (rt_ray_items.h).  Plain C++
// (host and device): the kernel, the host layer and
// tests/native/occl_items.cpp include it.  Compiled without FMA contraction
// everywhere, so t_cut has the same bits on both sides.
#pragma once

#include <stdint.h>

#include "rt_ray_items.h"

// tmax by its bits: NaN; > 0 (+inf included).  -0.0, 0 and every negative
// value, -inf included, are "not positive".
RT_TILES_FN int rt_occl_tmax_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
RT_TILES_FN int rt_occl_tmax_positive(uint32_t b) {
  return !(b >> 31) && (b & 0x7fffffffu) != 0u && !rt_occl_tmax_nan(b);
}

// A ray of an occlusion batch is traced (counted in rt_stats.camera) if a ray
// batch would trace it (rt_ray_traced) and its tmax is not NaN; a traced ray
// makes a query (rt_stats.shadow) if its tmax > 0.  Every other ray answers 0.
RT_TILES_FN int rt_occl_traced(const uint32_t o[3], const uint32_t d[3], uint32_t tmax) {
  return rt_ray_traced(o, d) && !rt_occl_tmax_nan(tmax);
}
RT_TILES_FN int rt_occl_queried(const uint32_t o[3], const uint32_t d[3], uint32_t tmax) {
  return rt_occl_traced(o, d, tmax) && rt_occl_tmax_positive(tmax);
}

// The Moller-Trumbore parameter beyond which no record's new_dist can be <=
// tmax: consider_exact's bound for a winner at distance tmax (rt_isect.h) --
// a record's new_dist is |(o + nd (t |d|)) - o|, t |d| up to a few ulps of
// itself plus the rounding of the hit point (ulps of |o|_max + the distance),
// so new_dist <= tmax implies t <= this, ties included.  ao = max |o|
// component, dlen = |d| as the reference computes it.  tmax = +inf: +inf.
RT_TILES_FN float rt_occl_t_cut(float tmax, float ao, float dlen) {
  return (tmax * (1.0f + 1e-5f) + (ao + tmax) * 2e-6f) / dlen;
}
