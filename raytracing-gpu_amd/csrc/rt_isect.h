// rt_isect.h -- ray / triangle arithmetic of the render kernels: the
// reference's Moller-Trumbore test (mt_test), Ray and its hit point and
// distance, the conservative prefilters (mt_candidate*), the closest-hit
// record Best and its updates (consider*), the any-hit tests (any_hit*) and
// the LDS-broadcast record loop (stage_test).
// Part of rt_render.hip's one translation unit.  Needs rt_cull.h, rt_device.h
// and rt_kernels.h (included here).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cull.h"
#include "rt_device.h"
#include "rt_kernels.h"

namespace rt {

static constexpr float kEps = 0.0000001f;  // cpu/hit.c:7 (float)1e-7

// The workgroup is one wave and a wave's LDS instructions execute in issue
// order, so LDS staging needs no s_barrier: only a compiler barrier that
// keeps the LDS reads and writes in source order.
__device__ __forceinline__ void wave_sync() { __asm__ volatile("" ::: "memory"); }
// the compare's own scalar pair (__ballot goes through a select and a second compare)
__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

__device__ __forceinline__ f3 ld3(const float* p) { return f3{p[0], p[1], p[2]}; }

// Moller-Trumbore, cpu/hit.c:15-33 with e1/e2 precomputed (same bits).
__device__ __forceinline__ bool mt_test(f3 o, f3 d, f3 v0, f3 e1, f3 e2, float& t, float& u,
                                        float& v) {
  f3 h = cross(d, e2);
  float a = dot(e1, h);
  if (a > -kEps && a < kEps) return false;
  float f = 1.0f / a;
  f3 s = sub(o, v0);
  u = f * dot(s, h);
  if (u < 0.0f || u > 1.0f) return false;
  f3 q = cross(s, e1);
  v = f * dot(d, q);
  if (v < 0.0f || u + v > 1.0f) return false;
  t = f * dot(e2, q);
  return t > kEps;
}

struct Ray {
  f3 o, d;     // origin, direction (as the reference holds them)
  float dlen;  // length(d)
  float eps;   // culling slack (world units) for this origin
  f3 oh, ol;   // o + eps, o - eps: the grown slab planes' offsets (rt_cull.h)
};

// dlen = length(d), computed by the caller or taken from where it was
// computed before (a directional light's row, rt_shade_rows.h)
__device__ __forceinline__ Ray make_ray_len(const KParams& p, f3 o, f3 d, float dlen, float eps_rel) {
  Ray r;
  r.o = o;
  r.d = d;
  r.dlen = dlen;
  r.eps = rt_cull_eps(eps_rel, o.x - p.scene_c.x, o.y - p.scene_c.y, o.z - p.scene_c.z,
                      p.scene_cmag, p.scene_r);
  r.oh = f3{o.x + r.eps, o.y + r.eps, o.z + r.eps};
  r.ol = f3{o.x - r.eps, o.y - r.eps, o.z - r.eps};
  return r;
}
__device__ __forceinline__ Ray make_ray(const KParams& p, f3 o, f3 d, float eps_rel) {
  return make_ray_len(p, o, d, length(d), eps_rel);
}

// normalize(d) as the hit point takes it: the three IEEE quotients d / |d|
__device__ __forceinline__ f3 unit_dir(const Ray& r) { return f3{r.d.x / r.dlen, r.d.y / r.dlen, r.d.z / r.dlen}; }

// The hit point o + normalize(d) * (t*|d|) (cpu/hit.c:35-37,58), with
// normalize(d) recomputed here (the same IEEE divisions every time, so the
// same bits) rather than kept live through the walks.
__device__ __forceinline__ f3 hit_point(const Ray& r, float t) {
  f3 nd{r.d.x / r.dlen, r.d.y / r.dlen, r.d.z / r.dlen};
  return add(r.o, scale(nd, t * r.dlen));
}

// new_dist = |hit point - o| (cpu/hit.c:58)
__device__ __forceinline__ float hit_dist(const Ray& r, float t) {
  return length(sub(hit_point(r, t), r.o));
}
// the same with nd = unit_dir(r) from the caller (the light buffers' scan: a
// directional light's is a constant of the light)
__device__ __forceinline__ float hit_dist(const Ray& r, f3 nd, float t) {
  return length(sub(add(r.o, scale(nd, t * r.dlen)), r.o));
}

// Conservative pre-filter of the Moller-Trumbore test.  h, a, s.h, d.q, e2.q
// are the reference's own float values (same operations); only the IEEE
// division f = 1/a is replaced by v_rcp_f32 (1 ulp).  A triangle is dropped
// only when the reference's u, v, t (which differ from these by a few ulps)
// are certain to fail cpu/hit.c:20-33, or when its distance certainly exceeds
// t_cut (closest hit: it cannot beat the current winner, ties included);
// survivors are re-tested exactly.  DESIGN.md "Exact MT with a cheap reject".
__device__ __forceinline__ bool mt_candidate(f3 o, f3 d, f3 v0, f3 e1, f3 e2, float t_cut) {
  // same staging as cpu/hit.c:15-33, so a wave whose lanes all fail u skips
  // the v and t work (coherent packets mostly agree)
  const float m = 1e-5f;  // >> the few-ulp gap between (u,v,t) and the reference's
  f3 h = cross(d, e2);
  float a = dot(e1, h);
  if (a > -kEps && a < kEps) return false;  // identical test, identical a
  float r = __builtin_amdgcn_rcpf(a);
  f3 s = sub(o, v0);
  float u = dot(s, h) * r;
  if (u < -1e-30f || u > 1.0f + m) return false;
  f3 q = cross(s, e1);
  float v = dot(d, q) * r;
  if (v < -1e-30f || u + v > 1.0f + m) return false;
  float t = dot(e2, q) * r;
  return !(t < kEps * (1.0f - m) || t > t_cut);
}

// mt_candidate for two triangles at once (brute-force loops): the two
// dependency chains are independent, so they interleave and hide each
// other's VALU latency; the stages still end early when every lane of the
// wave has rejected both (ballot).  Same float operations, same decisions.
__device__ __forceinline__ void mt_candidate2(f3 o, f3 d, const float4* qa, const float4* qb,
                                              float t_cut, bool& ca, bool& cb) {
  const float m = 1e-5f;
  const f3 v0a{qa[0].x, qa[0].y, qa[0].z}, e1a{qa[0].w, qa[1].x, qa[1].y}, e2a{qa[1].z, qa[1].w, qa[2].x};
  const f3 v0b{qb[0].x, qb[0].y, qb[0].z}, e1b{qb[0].w, qb[1].x, qb[1].y}, e2b{qb[1].z, qb[1].w, qb[2].x};
  const f3 ha = cross(d, e2a), hb = cross(d, e2b);
  const float aa = dot(e1a, ha), ab = dot(e1b, hb);
  const float ra = __builtin_amdgcn_rcpf(aa), rb = __builtin_amdgcn_rcpf(ab);
  const f3 sa = sub(o, v0a), sb = sub(o, v0b);
  const float ua = dot(sa, ha) * ra, ub = dot(sb, hb) * rb;
  ca = !(aa > -kEps && aa < kEps) && !(ua < -1e-30f || ua > 1.0f + m);
  cb = !(ab > -kEps && ab < kEps) && !(ub < -1e-30f || ub > 1.0f + m);
  if (__ballot(ca || cb) == 0) return;
  const f3 qva = cross(sa, e1a), qvb = cross(sb, e1b);
  const float va = dot(d, qva) * ra, vb = dot(d, qvb) * rb;
  ca = ca && !(va < -1e-30f || ua + va > 1.0f + m);
  cb = cb && !(vb < -1e-30f || ub + vb > 1.0f + m);
  if (__ballot(ca || cb) == 0) return;
  const float ta = dot(e2a, qva) * ra, tb = dot(e2b, qvb) * rb;
  ca = ca && !(ta < kEps * (1.0f - m) || ta > t_cut);
  cb = cb && !(tb < kEps * (1.0f - m) || tb > t_cut);
}

struct Best {
  float dist;  // +inf = none
  float t_cut; // parametric bound beyond which no triangle can win (+inf = none)
  uint32_t prim, obj;
  float u, v;
  float t;  // the winner's MT t; its hit point is hit_point(r, t)
};

// No hit yet: what a closest-hit query starts from.
__device__ __forceinline__ Best best_none() {
  Best b;
  b.dist = __builtin_inff();
  b.t_cut = __builtin_inff();
  b.prim = 0xffffffffu;
  b.obj = 0;
  b.u = b.v = 0.0f;
  b.t = 0.0f;
  return b;
}

__device__ __forceinline__ void consider_exact(const Ray& r, const float4& q0, const float4& q1,
                                               const float4& q2, Best& b);

__device__ __forceinline__ void consider(const Ray& r, const float4& q0, const float4& q1,
                                         const float4& q2, Best& b) {
  f3 v0{q0.x, q0.y, q0.z}, e1{q0.w, q1.x, q1.y}, e2{q1.z, q1.w, q2.x};
  if (!mt_candidate(r.o, r.d, v0, e1, e2, b.t_cut)) return;
  consider_exact(r, q0, q1, q2, b);
}

// The reference's exact test of a prefilter survivor and the lexicographic
// (new_dist, prim) update (cpu/hit.c:15-37,58-59,82).
__device__ __forceinline__ void consider_exact(const Ray& r, const float4& q0, const float4& q1,
                                               const float4& q2, Best& b) {
  f3 v0{q0.x, q0.y, q0.z}, e1{q0.w, q1.x, q1.y}, e2{q1.z, q1.w, q2.x};
  float t, u, v;
  if (!mt_test(r.o, r.d, v0, e1, e2, t, u, v)) return;
  float nd = hit_dist(r, t);
  if (!((double)nd > 0.01)) return;
  uint32_t prim = __float_as_uint(q2.y);
  if (nd < b.dist || (nd == b.dist && prim < b.prim)) {
    b.dist = nd;
    // a rival's new_dist is |(o + nd*(t*|d|)) - o|: t*|d| up to a few ulps of
    // |t*|d||, plus the rounding of the hit point (ulps of |o|+dist)
    float ao = fmaxf(fabsf(r.o.x), fmaxf(fabsf(r.o.y), fabsf(r.o.z)));
    b.t_cut = (nd * (1.0f + 1e-5f) + (ao + nd) * 2e-6f) / r.dlen;
    b.prim = prim;
    b.obj = __float_as_uint(q2.z);
    b.u = u;
    b.v = v;
    b.t = t;
  }
}

// consider() for wave-converged loops over LDS-broadcast records (the packet
// walk's leaves, the candidate lists): the same prefilter decisions, but one
// wave-uniform exit after the u stage instead of a divergent branch per
// stage.  Each divergent stage cost an exec save / branch / restore of scalar
// instructions per record -- as many SALU as VALU in those loops
// (profiles/r04t_c5/pmc_sq.json: 2.13 G SALU to 3.89 G VALU per trace launch);
// the v and t stages run for the whole wave once any lane passes u (a
// divergent stage costs the wave the same VALU cycles anyway).  act: the
// lane's query, am: the wave's mask of act (wave_ballot(act), taken once by
// the caller, not per record); the call itself must be wave-uniform.  (The
// plain divergent `if (act) consider(...)` was the losing side of that
// measurement, removed.)
__device__ __forceinline__ void consider_w(const Ray& r, bool act, uint64_t am, const float4& q0,
                                           const float4& q1, const float4& q2, Best& b) {
  const float m = 1e-5f;  // as mt_candidate
  const f3 v0{q0.x, q0.y, q0.z}, e1{q0.w, q1.x, q1.y}, e2{q1.z, q1.w, q2.x};
  const f3 h = cross(r.d, e2);
  const float a = dot(e1, h);
  const float rc = __builtin_amdgcn_rcpf(a);
  const f3 s = sub(r.o, v0);
  const float u = dot(s, h) * rc;
  const bool ca = !(a > -kEps && a < kEps), cu0 = !(u < -1e-30f), cu1 = !(u > 1.0f + m);
  bool c = act && ca && cu0 && cu1;
  // the wave's verdict from the compares' own scalar pairs (one ballot each,
  // ANDed in scalar registers: a ballot of c itself goes through a select)
  if ((am & wave_ballot(ca) & wave_ballot(cu0) & wave_ballot(cu1)) == 0) return;
  const f3 q = cross(s, e1);
  const float v = dot(r.d, q) * rc;
  const float t = dot(e2, q) * rc;
  c = c && !(v < -1e-30f || u + v > 1.0f + m) && !(t < kEps * (1.0f - m) || t > b.t_cut);
  if (c) consider_exact(r, q0, q1, q2, b);
}

// Records [0, n) of the LDS stage tested as broadcasts (consider_w).
// Converged call.  (The next record's reads issued during a test -- the
// index clamped, no branch -- measured slower: trace 6.05 -> 6.51 ms on C5,
// profiles/r05q_consider_w/ab_lds_pipe.log; round 1 found the same.)
__device__ __forceinline__ void stage_test(const Ray& r, bool act, uint64_t am, uint32_t n, Best& b,
                                           const float4* stage) {
  uint32_t k3 = 0;  // 3 k, kept in a VGPR: the record's LDS address advances there
  __asm__ volatile("" : "+v"(k3));
  for (uint32_t k = 0; k < n; k++, k3 += 3) consider_w(r, act, am, stage[k3], stage[k3 + 1], stage[k3 + 2], b);
}

// Any hit with new_dist > 0.01 (cpu/hit.c:93-109: collide_dist > 0 <=>
// shadowed, cpu/light.c:24-31).  Early exit is exact for an object none of
// whose triangles can interpolate an exactly zero normal (record flag bit 0,
// host/accel.c): its closest hit then counts in collide_dist whatever
// triangle the walk met first.  A hit on a flagged object sets `risk`
// (reported as RT_EZERONORMAL, never silent).
__device__ __forceinline__ bool any_hit_exact(const Ray& r, f3 nd, const float4& q0, const float4& q1,
                                              const float4& q2, uint32_t& risk);

// nd = unit_dir(r), from the caller: the light buffers' scan has a directional
// light's from the light's row (rt_shade_rows.h)
__device__ __forceinline__ bool any_hit_rec(const Ray& r, f3 nd, const float4& q0, const float4& q1,
                                            const float4& q2, uint32_t& risk) {
  f3 v0{q0.x, q0.y, q0.z}, e1{q0.w, q1.x, q1.y}, e2{q1.z, q1.w, q2.x};
  if (!mt_candidate(r.o, r.d, v0, e1, e2, __builtin_inff())) return false;
  return any_hit_exact(r, nd, q0, q1, q2, risk);
}
__device__ __forceinline__ bool any_hit_rec(const Ray& r, const float4& q0, const float4& q1,
                                            const float4& q2, uint32_t& risk) {
  return any_hit_rec(r, unit_dir(r), q0, q1, q2, risk);
}

// the exact test of a prefilter survivor (any_hit_rec)
__device__ __forceinline__ bool any_hit_exact(const Ray& r, f3 nd, const float4& q0, const float4& q1,
                                              const float4& q2, uint32_t& risk) {
  f3 v0{q0.x, q0.y, q0.z}, e1{q0.w, q1.x, q1.y}, e2{q1.z, q1.w, q2.x};
  float t, u, v;
  if (!mt_test(r.o, r.d, v0, e1, e2, t, u, v)) return false;
  if (!((double)hit_dist(r, nd, t) > 0.01)) return false;
  risk |= __float_as_uint(q2.w) & RT_REC_ZERO_RISK;
  return true;
}
__device__ __forceinline__ bool any_hit_exact(const Ray& r, const float4& q0, const float4& q1,
                                              const float4& q2, uint32_t& risk) {
  return any_hit_exact(r, unit_dir(r), q0, q1, q2, risk);
}

}  // namespace rt
