// rt_walk_lane.h -- the per-lane octree walks: the lane's traversal stack (LDS
// + global spill), its counters (LaneCount, absorb), the box tests, the child
// pushes, a leaf's records (leaf_lane), the closest-hit and any-hit walks
// (oct_closest, oct_any) and the proven reflection walk (RfRay ..
// oct_closest_rf, csrc/rt_reflect.hip).
// Part of rt_render.hip's one translation unit.  Needs rt_isect.h and
// rt_reflect.h (included here).
#pragma once

#include "rt_isect.h"
#include "rt_reflect.h"

namespace rt {

// -------------------------------------------------------------- OCTREE
// Per-lane traversal stack: the first kLdsStack entries live in LDS, laid
// out [entry][lane] so every lane hits its own bank; deeper entries spill to
// a per-lane area in global memory (rare: typical depth is < 16).
#ifndef RT_LDS_STACK
#define RT_LDS_STACK 10
#endif
static constexpr int kLdsStack = RT_LDS_STACK;  // per-lane stack entries in LDS (deeper: global spill)
static constexpr int kSpillStack = RT_SPILL_STACK;

struct Stack {
  uint32_t* idx;  // LDS, kLdsStack x 64
  float* tt;      // LDS, kLdsStack x 64
  uint2* spill;   // this lane's first spill entry; entry k at spill[k * stride]
  uint32_t stride;  // lanes of the launch: spill entries are [entry][lane], so the
                    // lanes of a wave at the same depth touch adjacent words
  int lane;
  int sp;
};

// The empty stack of `lane` in a one-wave workgroup: its LDS entries in the
// kernel's stack area, its spill entries in p.spill.  (gl first, as the kernels
// had it: formed inside the pointer expression, eight kernels' registers moved.)
__device__ __forceinline__ void lane_stack(const KParams& p, float4* s_stack, int lane, Stack& stk) {
  const size_t gl = (size_t)blockIdx.x * 64 + (size_t)lane;
  stk.idx = (uint32_t*)s_stack;
  stk.tt = (float*)s_stack + kLdsStack * 64;
  stk.spill = p.spill + gl;
  stk.stride = gridDim.x * 64u;
  stk.lane = lane;
  stk.sp = 0;
}

// Counters of one lane's own walk (divergent code); folded into the wave's
// WorkCount after the walk (absorb).
struct LaneCount {
  uint32_t nodes, tris, overflow;
  uint32_t risk;           // any hit on an object whose normal can vanish (any_hit_rec)
  uint32_t lnodes, ltris;  // this lane's own visits / tests (COUNT pass)
  uint32_t spills;         // pushes beyond the LDS part of the stack (COUNT pass)
  uint32_t unproven;       // exact reflection walk: queries outside its bound's assumptions
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return __builtin_amdgcn_readfirstlane(x);
}

// Number of distinct keys among the lanes executing this call (divergent
// code: the lanes of the current loop iteration), added once to lane `first`.
// Algorithmic-byte accounting of the per-lane walks (COUNT pass only): a
// record that several lanes load with the same instruction counts once, the
// same rule as the packet walk's wave-uniform fetches.
__device__ __forceinline__ uint32_t lanes_distinct(uint32_t key) {
  uint64_t m = __ballot(1);
  uint32_t n = 0;
  int me = __lane_id();
  bool first = (int)(__ffsll((unsigned long long)m) - 1) == me;
  while (m) {
    int l = __ffsll((unsigned long long)m) - 1;
    uint32_t k = __shfl(key, l);
    m &= ~__ballot(key == k);
    n++;
  }
  return first ? n : 0u;
}

template <bool COUNT>
__device__ __forceinline__ void absorb(WorkCount& wc, const LaneCount& lc, bool shadow) {
  if (COUNT) {
    wc.nodes += wave_sum(lc.nodes);
    wc.tris += wave_sum(lc.tris);
    const uint32_t ln = wave_sum(lc.lnodes), lt = wave_sum(lc.ltris);
    if (shadow) {
      wc.sh_nodes += ln;
      wc.sh_tris += lt;
    } else {
      wc.cl_nodes += ln;
      wc.cl_tris += lt;
    }
  }
  wc.overflow += wave_sum(lc.overflow);
  wc.zero_risk += (uint32_t)__popcll(__ballot(lc.risk != 0));
  wc.cl_unproven += (uint32_t)__popcll(__ballot(lc.unproven != 0));
  if (COUNT) wc.stack_spills += wave_sum(lc.spills);
}

__device__ __forceinline__ void push(Stack& s, uint32_t i, float t, LaneCount& wc) {
  if (s.sp < kLdsStack) {
    s.idx[s.sp * 64 + s.lane] = i;
    s.tt[s.sp * 64 + s.lane] = t;
  } else if (s.sp < kLdsStack + kSpillStack) {
    s.spill[(size_t)(s.sp - kLdsStack) * s.stride] = make_uint2(i, __float_as_uint(t));
    wc.spills++;
  } else {
    wc.overflow++;  // reported as RT_EDEPTH by rt_hip_stats: never silent
    return;
  }
  s.sp++;
}

__device__ __forceinline__ void pop(Stack& s, uint32_t& i, float& t) {
  --s.sp;
  if (s.sp < kLdsStack) {
    i = s.idx[s.sp * 64 + s.lane];
    t = s.tt[s.sp * 64 + s.lane];
  } else {
    uint2 e = s.spill[(size_t)(s.sp - kLdsStack) * s.stride];
    i = e.x;
    t = __uint_as_float(e.y);
  }
}

__device__ __forceinline__ f3 inv_dir(f3 d) { return f3{rt_inv(d.x), rt_inv(d.y), rt_inv(d.z)}; }

// slab test of the eps-grown box (rt_cull.h): the hit flag, t = entry parameter
__device__ __forceinline__ bool box_hit(const Ray& r, f3 inv, float4 lo, float4 hi, float& t) {
  return rt_box_hit(r.oh.x, r.oh.y, r.oh.z, r.ol.x, r.ol.y, r.ol.z, inv.x, inv.y, inv.z, lo.x,
                    lo.y, lo.z, hi.x, hi.y, hi.z, &t);
}

// entry parameter of the eps-grown box, +inf on a miss
__device__ __forceinline__ float box_enter(const Ray& r, f3 inv, float4 lo, float4 hi) {
  float t;
  return box_hit(r, inv, lo, hi, t) ? t : __builtin_inff();
}

// Shadow walk box test (csrc/rt_shadow.hip): the box grown by mu eps instead
// of eps, and reaching parameters t >= -nu eps / |d| (a float accept may sit
// slightly behind the origin).  mn = the node's (mu, nu), both >= 1.
__device__ __forceinline__ bool box_hit_sh(const Ray& r, f3 inv, float4 lo, float4 hi, float2 mn) {
  const float e = r.eps * mn.x;
  float tmin;
  const float ohx = r.o.x + e, ohy = r.o.y + e, ohz = r.o.z + e;
  const float olx = r.o.x - e, oly = r.o.y - e, olz = r.o.z - e;
  float tx0 = fmaf(lo.x, inv.x, -(ohx * inv.x)), tx1 = fmaf(hi.x, inv.x, -(olx * inv.x));
  float ty0 = fmaf(lo.y, inv.y, -(ohy * inv.y)), ty1 = fmaf(hi.y, inv.y, -(oly * inv.y));
  float tz0 = fmaf(lo.z, inv.z, -(ohz * inv.z)), tz1 = fmaf(hi.z, inv.z, -(olz * inv.z));
  tmin = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fminf(tz0, tz1));
  const float tmax = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
  return tmax >= fmaxf(tmin, -(mn.y * r.eps) / r.dlen);
}

__device__ __forceinline__ bool rt_prune(float t_enter, float dlen, float best, float eps) {
  return t_enter * dlen > rt_prune_limit(best, eps);
}

// octant nearest to the origin side (rt_cull.h: bit a = upper half of axis a)
__device__ __forceinline__ uint32_t near_octant(f3 d) {
  return (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
}


// child-mask bit o moved to bit o ^ dm (the visiting order's index space)
__device__ __forceinline__ uint32_t mask_xor(uint32_t m, uint32_t dm) {
  if (dm & 1u) m = ((m & 0x55u) << 1) | ((m & 0xAAu) >> 1);
  if (dm & 2u) m = ((m & 0x33u) << 2) | ((m & 0xCCu) >> 2);
  if (dm & 4u) m = ((m & 0x0Fu) << 4) | ((m & 0xF0u) >> 4);
  return m;
}

// Interior node: test the children's boxes and push the hits far-to-near in
// octant order (j = 7..0, octant j ^ dm: a valid front-to-back order for the
// disjoint octant cells), so the nearest child is popped first.  Software-
// pipelined: child k+1's box is in flight while child k is tested.
// CLOSEST pushes (node, entry t) and prunes by best; any-hit pushes the
// child's own (first, info) words from its box record, so a pop needs no
// node fetch -- one dependent load per step instead of two.  (The per-lane
// any-hit walk uses push_children_any: measured on C5, 16.18 vs 16.33 ms.)
// (Two child boxes in flight while one is tested -- meant to halve the
// serialised load latencies of a cold node in the per-lane reflection walks of
// an 8-way split's longest items -- measured neutral: C5 9.94 / 9.90 vs 9.96 /
// 9.89 ms, slowest of 8 ranks 3.06 vs 3.05 ms, profiles/r05x_tuning/; trace
// 4.64 / 4.65 vs 4.64 / 4.61 ms, profiles/r08_knob_resweep/; removed.)
template <bool CLOSEST, bool COUNT>
__device__ __forceinline__ void push_children(const float4* __restrict__ node, const Ray& r, f3 inv,
                                              uint32_t dm, uint32_t first, uint32_t info,
                                              float best, Stack& s, LaneCount& wc) {
  uint32_t mask = RT_NODE_MASK(info);
  uint32_t mj = mask_xor(mask, dm);
  if (!mj) return;
  int j = 31 - __clz(mj);
  mj &= ~(1u << j);
  uint32_t ci = first + (uint32_t)__popc(mask & ((1u << ((uint32_t)j ^ dm)) - 1u));
  float4 nlo = node[2 * ci], nhi = node[2 * ci + 1];
  if (COUNT) wc.nodes += lanes_distinct(ci);
  for (;;) {
    float4 clo = nlo, chi = nhi;
    uint32_t cc = ci;
    bool more = mj != 0u;
    if (more) {
      j = 31 - __clz(mj);
      mj &= ~(1u << j);
      ci = first + (uint32_t)__popc(mask & ((1u << ((uint32_t)j ^ dm)) - 1u));
      nlo = node[2 * ci];
      nhi = node[2 * ci + 1];
      if (COUNT) wc.nodes += lanes_distinct(ci);
    }
    float t0 = box_enter(r, inv, clo, chi);
    if (CLOSEST) {
      if (t0 != __builtin_inff() && !(best != __builtin_inff() && rt_prune(t0, r.dlen, best, r.eps)))
        push(s, cc, t0, wc);
    } else if (t0 != __builtin_inff()) {
      push(s, __float_as_uint(clo.w), chi.w, wc);
    }
    if (!more) break;
  }
}

// Any-hit interior node: the children's boxes in storage order (increasing
// octant), reversed when the ray's direction octant is mostly negative, so
// the walk still tends to pop the nearer children first; no per-child
// octant arithmetic (any-hit needs no exact front-to-back order).  Child
// k+1's box is in flight while child k is tested.
template <bool COUNT>
__device__ __forceinline__ void push_children_any(const float4* __restrict__ node,
                                                  const float2* __restrict__ mu, const Ray& r,
                                                  f3 inv, uint32_t dm, uint32_t first,
                                                  uint32_t info, Stack& s, LaneCount& wc) {
  const int cnt = (int)RT_NODE_COUNT(info);
  const bool up = __popc(dm) >= 2;  // storage order = far-to-near for dm = 7
  int k = up ? 0 : cnt - 1;
  const int step = up ? 1 : -1;
  uint32_t ci = first + (uint32_t)k;
  float4 nlo = node[2 * ci], nhi = node[2 * ci + 1];
  // exact-shadow mode (mu != NULL, a kernel argument: a uniform branch)
  float2 nmu = mu ? mu[ci] : make_float2(1.0f, 0.0f);
  if (COUNT) wc.nodes += lanes_distinct(ci);
  for (int n = 0; n < cnt; n++) {
    float4 clo = nlo, chi = nhi;
    const float2 cmu = nmu;
    if (n + 1 < cnt) {
      ci += (uint32_t)step;
      nlo = node[2 * ci];
      nhi = node[2 * ci + 1];
      if (mu) nmu = mu[ci];
      if (COUNT) wc.nodes += lanes_distinct(ci);
    }
    const bool h = mu ? box_hit_sh(r, inv, clo, chi, cmu) : box_enter(r, inv, clo, chi) != __builtin_inff();
    if (h) push(s, __float_as_uint(clo.w), chi.w, wc);
  }
}

// A leaf's records, software-pipelined: record k+1 is in flight while record
// k is tested.  ANY: returns true at the first any-hit.  (Two records in
// flight for the closest hit spilled 20 VGPRs and measured slower: C5 10.01 vs
// 9.96 / 9.89 ms, slowest of 8 ranks 3.24 vs 3.05 ms, profiles/r05x_tuning/;
// trace 4.67 / 4.72 vs 4.64 / 4.61 ms, profiles/r08_knob_resweep/; removed.)
template <bool ANY, bool COUNT>
__device__ __forceinline__ bool leaf_lane(const float4* __restrict__ tri, uint32_t first,
                                          uint32_t cnt, const Ray& r, Best& b, LaneCount& wc) {
  const float4* q = tri + 3 * (size_t)first;
  float4 n0 = q[0], n1 = q[1], n2 = q[2];
  for (uint32_t k = 0; k < cnt; k++) {
    float4 q0 = n0, q1 = n1, q2 = n2;
    if (k + 1 < cnt) {
      n0 = q[3 * (k + 1)];
      n1 = q[3 * (k + 1) + 1];
      n2 = q[3 * (k + 1) + 2];
    }
    if (COUNT) {
      wc.tris += lanes_distinct(first + k);
      wc.ltris++;
    }
    if (ANY) {
      if (any_hit_rec(r, q0, q1, q2, wc.risk)) return true;
    } else {
      consider(r, q0, q1, q2, b);
    }
  }
  return false;
}

// Per-lane closest-hit walk (each lane its own stack).
template <bool COUNT>
__device__ void oct_closest(const KParams& p, const Ray& r, Best& b, Stack& s, LaneCount& wc) {
  const float4* __restrict__ node = p.node;
  f3 inv = inv_dir(r.d);
  uint32_t dm = near_octant(r.d);
  s.sp = 0;
  wave_sync();
  {
    float t0 = box_enter(r, inv, node[0], node[1]);
    if (t0 != __builtin_inff()) push(s, 0, t0, wc);
  }
  while (s.sp > 0) {
    uint32_t ni;
    float tn;
    pop(s, ni, tn);
    if (b.dist != __builtin_inff() && rt_prune(tn, r.dlen, b.dist, r.eps)) continue;
    float4 lo = node[2 * ni], hi = node[2 * ni + 1];
    uint32_t first = __float_as_uint(lo.w), info = __float_as_uint(hi.w);
    if (COUNT) {
      wc.nodes += lanes_distinct(ni);
      wc.lnodes++;
    }
    if (info & RT_NODE_LEAF)
      leaf_lane<false, COUNT>(p.tri, first, RT_LEAF_COUNT(info), r, b, wc);
    else
      push_children<true, COUNT>(node, r, inv, dm, first, info, b.dist, s, wc);
  }
  wave_sync();
}

// Per-lane any-hit walk; a stack entry holds the node's own (first, info).
template <bool COUNT>
__device__ bool oct_any(const KParams& p, const Ray& r, Stack& s, LaneCount& wc) {
  const float4* __restrict__ node = p.node;
  f3 inv = inv_dir(r.d);
  uint32_t dm = near_octant(r.d);
  s.sp = 0;
  wave_sync();
  {
    float4 lo = node[0], hi = node[1];
    if (COUNT) wc.nodes += lanes_distinct(0);
    const bool h = p.node_mu ? box_hit_sh(r, inv, lo, hi, p.node_mu[0])
                             : box_enter(r, inv, lo, hi) != __builtin_inff();
    if (h) push(s, __float_as_uint(lo.w), hi.w, wc);
  }
  Best unused;
  while (s.sp > 0) {
    uint32_t first;
    float info_bits;
    pop(s, first, info_bits);
    uint32_t info = __float_as_uint(info_bits);
    if (COUNT) wc.lnodes++;
    if (info & RT_NODE_LEAF) {
      if (leaf_lane<true, COUNT>(p.tri, first, RT_LEAF_COUNT(info), r, unused, wc)) {
        s.sp = 0;
        wave_sync();
        return true;
      }
    } else {
      push_children_any<COUNT>(node, p.node_mu, r, inv, dm, first, info, s, wc);
    }
  }
  wave_sync();
  return false;
}

// ------------------------------------------- exact reflection walk (policy 5)
// Reflection rays (bounce depth >= 1) with each node's box grown by the
// reach of the float Moller-Trumbore test's error region for THIS ray
// (csrc/rt_reflect.hip, DESIGN.md §2 "Reflection rays: exact by proof"): the
// node's normal cone bounds the ray's cosine with every plane below it, the
// 1e-7f accept threshold bounds it from below where the cone does not, and
// the origin's distance to the box bounds |S| = |o - v0|.  Pruning and the
// crossings behind the origin take the distance error the same way.
struct RfRay {
  f3 dh;     // d / |d| (rounded; psi covers the rounding of |axis . dh|)
  bool ok;   // |d| <= RT_RF_DLMAX (the floor factors' assumption), else counted
};

__device__ __forceinline__ RfRay rf_ray(const Ray& r) {
  RfRay q;
  const float inv = 1.0f / r.dlen;
  q.dh = f3{r.d.x * inv, r.d.y * inv, r.d.z * inv};
  q.ok = r.dlen <= RT_RF_DLMAX;
  return q;
}

// Node ni's bound for this ray: e = the box growth (world units, the walk's
// slack included; +inf: enter unconditionally), bh = how far behind the
// origin a crossing may lie (parametric), and the prune coefficients: a
// float accept below the node has t_f >= (t_enter * pa - pb) (parametric,
// when positive), so the node cannot win once that exceeds the best's t_cut.
struct RfB {
  float e, bh, pa, pb;
};

__device__ __forceinline__ RfB rf_bound(const float4* __restrict__ rf, uint32_t ni, const Ray& r, const RfRay& q,
                                        const float4& lo, const float4& hi) {
  const float4 A = rf[3 * (size_t)ni], B = rf[3 * (size_t)ni + 1], F = rf[3 * (size_t)ni + 2];
  const float inf = __builtin_inff();
  RfB o;
  // |S| <= (L1 distance to the box's farthest corner) + the longest edge below
  const float M = fmaxf(fabsf(r.o.x - lo.x), fabsf(r.o.x - hi.x)) + fmaxf(fabsf(r.o.y - lo.y), fabsf(r.o.y - hi.y)) +
                  fmaxf(fabsf(r.o.z - lo.z), fabsf(r.o.z - hi.z));
  const float Sb = M + B.w;
  const float c = fabsf(A.x * q.dh.x + A.y * q.dh.y + A.z * q.dh.z) - A.w;  // cosine lower bound
  float rps = inf, rho = 1.0f, kd = inf, r0 = inf;
  if (c > 2.0f * B.y) {  // the cone closes: rho <= Ra / c < 1/2
    rho = B.y / c;
    rps = B.x / (c - B.y);
    kd = B.z / c;
    r0 = B.w * (2.3841858e-7f + rho) / (1.0f - rho);
  }
  if (F.w < 0.5f) {  // the floor closes
    rps = fminf(rps, F.x);
    rho = fminf(rho, F.w);
    kd = fminf(kd, F.z);
    r0 = fminf(r0, F.y);
  }
  if (!(rho < 0.5f) || !q.ok) {
    o.e = inf;
    o.bh = inf;
    o.pa = 0.0f;
    o.pb = inf;
    return o;
  }
  // float evaluation of the bound: relative margins of 1e-5 (~100 roundings)
  const float up = 1.0f + 1e-5f, rho2 = rho * up;
  const float g = (rps * Sb + r0) * up;
  const float dist = Sb * kd * up;  // |S| kd: the crossing's distance error (world)
  o.e = r.eps + g;
  o.bh = dist / (1.0f - 2.0f * rho2) / r.dlen * up;
  // t* |d| <= [t_f |d| (1 + 2 eps)(1 - rho) + dist] / (1 - 2 rho) and t* >= the
  // grown box's entry (less the slab's rounding, covered by 2 eps as rt_prune):
  // t_f >= ((t_enter |d| (1 - 2^-21) - 2 eps)(1 - 2 rho) - dist) / (|d| (1 + 2 eps))
  const float s = (1.0f - 2.0f * rho2) * (1.0f - 4.8e-7f);
  o.pa = s * (1.0f - 1e-5f);
  o.pb = ((2.0f * r.eps) * (1.0f - 2.0f * rho2) + dist) / r.dlen * up;
  return o;
}

// slab test of the box grown by e (world), accepting parameters t >= -bh
__device__ __forceinline__ bool box_rf(const Ray& r, f3 inv, const float4& lo, const float4& hi, float e, float bh,
                                       float& tmin) {
  if (e == __builtin_inff()) {
    tmin = -__builtin_inff();
    return true;
  }
  const float ohx = r.o.x + e, ohy = r.o.y + e, ohz = r.o.z + e;
  const float olx = r.o.x - e, oly = r.o.y - e, olz = r.o.z - e;
  const float tx0 = fmaf(lo.x, inv.x, -(ohx * inv.x)), tx1 = fmaf(hi.x, inv.x, -(olx * inv.x));
  const float ty0 = fmaf(lo.y, inv.y, -(ohy * inv.y)), ty1 = fmaf(hi.y, inv.y, -(oly * inv.y));
  const float tz0 = fmaf(lo.z, inv.z, -(ohz * inv.z)), tz1 = fmaf(hi.z, inv.z, -(olz * inv.z));
  tmin = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fminf(tz0, tz1));
  const float tmax = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
  return tmax >= fmaxf(tmin, -bh);
}

// Test node ci's box for the rf walk; true: visit, key = the node's lower
// bound on an accept's t_f (-inf: none) for pruning at push and pop.
__device__ __forceinline__ bool rf_visit(const float4* __restrict__ rf, uint32_t ci, const Ray& r, const RfRay& q,
                                         f3 inv, const float4& lo, const float4& hi, float& key) {
  const RfB bd = rf_bound(rf, ci, r, q, lo, hi);
  float tmin;
  if (!box_rf(r, inv, lo, hi, bd.e, bd.bh, tmin)) return false;
  key = bd.e == __builtin_inff() ? -__builtin_inff() : tmin * bd.pa - bd.pb;  // unbounded: never pruned
  return true;
}

template <bool COUNT>
__device__ void oct_closest_rf(const KParams& p, const Ray& r, Best& b, Stack& s, LaneCount& wc) {
  const float4* __restrict__ node = p.node;
  const float4* __restrict__ rf = p.node_rf;
  const f3 inv = inv_dir(r.d);
  const uint32_t dm = near_octant(r.d);
  const RfRay q = rf_ray(r);
  if (!q.ok) wc.unproven++;  // counted (RT_EINEXACT), and walked with every node unbounded
  s.sp = 0;
  wave_sync();
  {
    float key;
    if (rf_visit(rf, 0, r, q, inv, node[0], node[1], key)) push(s, 0, key, wc);
  }
  while (s.sp > 0) {
    uint32_t ni;
    float key;
    pop(s, ni, key);
    if (b.dist != __builtin_inff() && key > b.t_cut) continue;
    const float4 lo = node[2 * ni], hi = node[2 * ni + 1];
    const uint32_t first = __float_as_uint(lo.w), info = __float_as_uint(hi.w);
    if (COUNT) {
      wc.nodes += lanes_distinct(ni);
      wc.lnodes++;
    }
    if (info & RT_NODE_LEAF) {
      leaf_lane<false, COUNT>(p.tri, first, RT_LEAF_COUNT(info), r, b, wc);
      continue;
    }
    // children far-to-near in octant order (push_children), each tested with
    // its own bound; child k+1's box and bound data in flight while k is tested
    const uint32_t mask = RT_NODE_MASK(info);
    uint32_t mj = mask_xor(mask, dm);
    if (!mj) continue;
    int j = 31 - __clz(mj);
    mj &= ~(1u << j);
    uint32_t ci = first + (uint32_t)__popc(mask & ((1u << ((uint32_t)j ^ dm)) - 1u));
    float4 nlo = node[2 * ci], nhi = node[2 * ci + 1];
    if (COUNT) wc.nodes += lanes_distinct(ci);
    for (;;) {
      const float4 clo = nlo, chi = nhi;
      const uint32_t cc = ci;
      const bool more = mj != 0u;
      if (more) {
        j = 31 - __clz(mj);
        mj &= ~(1u << j);
        ci = first + (uint32_t)__popc(mask & ((1u << ((uint32_t)j ^ dm)) - 1u));
        nlo = node[2 * ci];
        nhi = node[2 * ci + 1];
        if (COUNT) wc.nodes += lanes_distinct(ci);
      }
      float ck;
      if (rf_visit(rf, cc, r, q, inv, clo, chi, ck) && !(b.dist != __builtin_inff() && ck > b.t_cut))
        push(s, cc, ck, wc);
      if (!more) break;
    }
  }
  wave_sync();
}

}  // namespace rt
