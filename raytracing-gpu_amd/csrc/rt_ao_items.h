// rt_ao_items.h -- the ray rule of ambient occlusion from G-buffer records
// (rt_hip_ambient_occlusion, csrc/rt_ao.h, csrc/rt_ao.cpp): which samples
// shoot, the frame about a sample's normal, the hash that picks a sample's
// table rows and their symmetry, ray r's direction, and the work items of a
// batch.  A ray is a function of its sample's P and N, a small table of local
// directions and an index: no ray array exists anywhere.  Plain C++ (host and
// device): the kernels, the host layer and tests/native/ao_items.cpp include
// it; rtgpu.ao_rays_host is its numpy float32 twin.  Only float multiply, add
// and divide and one double sqrt, each correctly rounded, compiled without FMA
// contraction everywhere: the same bits on every side.  The order of every
// expression below is the rule; do not reassociate.
#pragma once

#include <stdint.h>

#include "rt_ray_items.h"

#define RT_AO_KMAX_D 1024u  // include/rt_hip.h RT_AO_KMAX

// ---- which samples shoot: a hit (prim >= 0) whose normal has a length l with
// 0 < l < +inf; l = length(N) of rt_device.h (float sum of squares, double
// sqrt).  NaN, zero, underflowing and overflowing normals do not shoot.
RT_TILES_FN float rt_ao_length(const float N[3]) {
  const float s = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
  return (float)__builtin_sqrt((double)s);
}
RT_TILES_FN int rt_ao_shoots(int prim, float l) { return prim >= 0 && l > 0.0f && l < __builtin_inff(); }

// ---- the frame (T, B, n) about n = N / l: the branchless orthonormal basis
// with the sign of n.z carried through (no trigonometry, no cross product with
// a chosen axis).  n.z = -1 takes sg = -1: the pole is at sg + n.z = 0, which
// no unit n reaches.
struct rt_ao_frame {
  float n[3], T[3], B[3];
};
RT_TILES_FN void rt_ao_frame_of(const float N[3], float l, rt_ao_frame* f) {
  const float nx = N[0] / l, ny = N[1] / l, nz = N[2] / l;
  const float sg = __builtin_copysignf(1.0f, nz);
  const float a = -1.0f / (sg + nz);
  const float b = nx * ny * a;
  f->n[0] = nx, f->n[1] = ny, f->n[2] = nz;
  f->T[0] = 1.0f + sg * nx * nx * a;
  f->T[1] = sg * b;
  f->T[2] = -sg * nx;
  f->B[0] = b;
  f->B[1] = sg + ny * ny * a;
  f->B[2] = -ny;
}

// ---- the hash of sample g = base + i (64-bit: a batch cut into pieces with
// the right bases hashes as the whole)
RT_TILES_FN uint32_t rt_ao_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
RT_TILES_FN uint32_t rt_ao_hash(unsigned long long g, uint32_t seed) {
  return rt_ao_mix32((uint32_t)g ^ rt_ao_mix32((uint32_t)(g >> 32) + seed));
}

// ---- ray r of a sample with hash h: row ((h >> 3) % m + r) % m of the table
// (consecutive rows from a hashed start, wrapping), its (x, y, z) under the
// symmetry of h's low bits -- bit 0 swaps x and y, then bit 1 negates x and
// bit 2 negates y -- and d = (x T + y B) + z n, not normalised afterwards.
RT_TILES_FN uint32_t rt_ao_row(uint32_t h, uint32_t m, uint32_t r) { return ((h >> 3) % m + r) % m; }
RT_TILES_FN void rt_ao_dir(const rt_ao_frame* f, const float row[3], uint32_t h, float d[3]) {
  float x = row[0], y = row[1];
  const float z = row[2];
  if (h & 1u) {
    const float t = x;
    x = y;
    y = t;
  }
  if (h & 2u) x = -x;
  if (h & 4u) y = -y;
  for (int c = 0; c < 3; c++) d[c] = (x * f->T[c] + y * f->B[c]) + z * f->n[c];
}

// ---- work items: a whole number of samples each, so a sample's count is one
// wave's and needs no atomic.  k <= 64: an item is spi = 64 / k consecutive
// samples, lane q k + r = ray r of the item's sample q, lanes from spi k up
// idle.  k > 64: an item is one sample, walked in ceil(k / 64) rounds.
RT_TILES_FN uint32_t rt_ao_spi(uint32_t k) { return k <= 64u ? 64u / k : 1u; }
// lane / k for lane < 64 and k <= 64 without a division: kinv = ceil(2^16 / k)
// errs by less than k / 2^16 per unit of lane, and 63 * 64 < 2^16
RT_TILES_FN uint32_t rt_ao_kinv(uint32_t k) { return (65536u + k - 1u) / k; }
RT_TILES_FN uint32_t rt_ao_lane_sample(uint32_t lane, uint32_t kinv) { return (lane * kinv) >> 16; }
RT_TILES_FN uint32_t rt_ao_rounds(uint32_t k) { return (k + 63u) / 64u; }
RT_TILES_FN unsigned long long rt_ao_item_count(unsigned long long n, uint32_t k) {
  const unsigned long long spi = rt_ao_spi(k);
  return (n + spi - 1) / spi;
}
