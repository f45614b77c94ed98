// rt_occl.h -- the kernel of an occlusion batch (include/rt_hip.h
// rt_hip_occluded): for every ray of a caller's batch one byte, 1 if the
// reference's collide_dist (cpu/hit.c:93-109) is not 0 and <= the ray's tmax.
// The any-hit tests and walks of rt_isect.h, rt_walk_lane.h and rt_walk_wave.h
// with a distance bound, as new functions beside them (the existing ones take
// none and are left as they are), and rays_occl_kernel, which has the shape
// of rays_trace_kernel (rt_rays.h).
// Part of rt_render.hip's one translation unit, included after every other
// kernel: needs the walks, flush_counts and ld3.  The batch's host-testable
// arithmetic is csrc/rt_occl_items.h; its launch csrc/rt_occl.cpp.
#pragma once

#include "rt_occl_items.h"

namespace rt {

// A lane's distance bound: tmax as the caller gave it (world distance, the
// units of new_dist) and the prefilter's parametric bound for it.
struct OcclBound {
  float tmax, t_cut;
};

__device__ __forceinline__ OcclBound occl_bound(const Ray& r, float tmax) {
  const float ao = fmaxf(fabsf(r.o.x), fmaxf(fabsf(r.o.y), fabsf(r.o.z)));
  return OcclBound{tmax, rt_occl_t_cut(tmax, ao, r.dlen)};
}

// The exact test of a prefilter survivor: the reference's accept, its
// new_dist > 0.01 and new_dist <= tmax (any_hit_exact with the bound).  Early
// exit is exact under any_hit_exact's rule: an object none of whose triangles
// can interpolate a zero normal that has a hit in (0.01, tmax] has its closest
// hit there too.  A hit on a flagged object sets `risk`.
__device__ __forceinline__ bool occl_exact(const Ray& r, f3 nd, const OcclBound& ob, const float4& q0,
                                           const float4& q1, const float4& q2, uint32_t& risk) {
  f3 v0{q0.x, q0.y, q0.z}, e1{q0.w, q1.x, q1.y}, e2{q1.z, q1.w, q2.x};
  float t, u, v;
  if (!mt_test(r.o, r.d, v0, e1, e2, t, u, v)) return false;
  const float dist = hit_dist(r, nd, t);
  if (!((double)dist > 0.01 && dist <= ob.tmax)) return false;
  risk |= __float_as_uint(q2.w) & RT_REC_ZERO_RISK;
  return true;
}

// A record: skipped only by mt_candidate with the bound's t_cut, else tested exactly.
__device__ __forceinline__ bool occl_rec(const Ray& r, f3 nd, const OcclBound& ob, const float4& q0,
                                         const float4& q1, const float4& q2, uint32_t& risk) {
  f3 v0{q0.x, q0.y, q0.z}, e1{q0.w, q1.x, q1.y}, e2{q1.z, q1.w, q2.x};
  if (!mt_candidate(r.o, r.d, v0, e1, e2, ob.t_cut)) return false;
  return occl_exact(r, nd, ob, q0, q1, q2, risk);
}

// ---- FLAT: flat_any_w / flat_any_tp with the bounded record test
__device__ bool flat_occl_w(const KParams& p, const Ray& r, const OcclBound& ob, bool act, WaveCtx& w, WorkCount& wc) {
  bool alive = act, hit = false;
  uint32_t risk = 0;
  const uint32_t n = p.nrec;
  if (__ballot(alive) == 0 || n == 0) return false;
  const f3 nd = unit_dir(r);
  Fetch f = fetch_issue<kStageFlat>(p.tri, 3 * (int)chunk<kFlatRecs>(n, 0), w.lane);
  for (uint32_t base = 0; base < n; base += kFlatRecs) {
    uint32_t m = chunk<kFlatRecs>(n, base);
    fetch_commit<kStageFlat>(f, w);
    uint32_t nb = base + kFlatRecs;
    if (nb < n) f = fetch_issue<kStageFlat>(p.tri + 3 * (size_t)nb, 3 * (int)chunk<kFlatRecs>(n, nb), w.lane);
    uint32_t k = 0;
    for (; k + 1 < m; k += 2) {
      const float4 qa[3] = {w.stage[3 * k], w.stage[3 * k + 1], w.stage[3 * k + 2]};
      const float4 qb[3] = {w.stage[3 * k + 3], w.stage[3 * k + 4], w.stage[3 * k + 5]};
      bool ca = false, cb = false;
      if (alive) mt_candidate2(r.o, r.d, qa, qb, ob.t_cut, ca, cb);
      if ((ca && occl_exact(r, nd, ob, qa[0], qa[1], qa[2], risk)) ||
          (cb && occl_exact(r, nd, ob, qb[0], qb[1], qb[2], risk))) {
        hit = true;
        alive = false;
      }
      if (__ballot(alive) == 0) break;
    }
    if (k < m && __ballot(alive) != 0) {
      const float4 q0 = w.stage[3 * k], q1 = w.stage[3 * k + 1], q2 = w.stage[3 * k + 2];
      if (alive && occl_rec(r, nd, ob, q0, q1, q2, risk)) {
        hit = true;
        alive = false;
      }
    }
    if (__ballot(alive) == 0) break;
  }
  wc.zero_risk += (uint32_t)__popcll(__ballot(risk != 0));
  return hit;
}

__device__ bool flat_occl_tp(const KParams& p, const Ray& r, const OcclBound& ob, bool act, WorkCount& wc) {
  const uint32_t n = p.nrec;
  const int lane = (int)(threadIdx.x & 63);
  uint64_t am = __ballot(act);
  bool res = false;
  uint32_t risk = 0;  // per lane: any tested triangle's flag (conservative)
  while (am) {
    const int l = __ffsll((unsigned long long)am) - 1;
    am &= am - 1;
    const Ray q = ray_of_lane(r, l);
    const OcclBound qb{__shfl(ob.tmax, l), __shfl(ob.t_cut, l)};
    const f3 nd = unit_dir(q);
    bool hit = false;
    for (uint32_t base = 0; base < n && !hit; base += 64) {  // hit is wave-uniform (ballot)
      const uint32_t i = base + (uint32_t)lane;
      bool h = false;
      if (i < n) {
        const float4* t = p.tri + 3 * (size_t)i;
        h = occl_rec(q, nd, qb, t[0], t[1], t[2], risk);
      }
      hit = __ballot(h) != 0;
    }
    if (lane == l) res = hit;
  }
  wc.zero_risk += (uint32_t)__popcll(__ballot(risk != 0));
  return res;
}

// A leaf's records, record k+1 in flight while record k is tested (leaf_lane);
// true at the first record that occludes.
__device__ __forceinline__ bool occl_leaf(const float4* __restrict__ tri, uint32_t first, uint32_t cnt, const Ray& r,
                                          f3 nd, const OcclBound& ob, LaneCount& wc) {
  const float4* q = tri + 3 * (size_t)first;
  float4 n0 = q[0], n1 = q[1], n2 = q[2];
  for (uint32_t k = 0; k < cnt; k++) {
    const float4 q0 = n0, q1 = n1, q2 = n2;
    if (k + 1 < cnt) {
      n0 = q[3 * (k + 1)];
      n1 = q[3 * (k + 1) + 1];
      n2 = q[3 * (k + 1) + 2];
    }
    if (occl_rec(r, nd, ob, q0, q1, q2, wc.risk)) return true;
  }
  return false;
}

// ---- per-lane bounded any-hit walk.  oct_any's stack -- an entry is the
// node's own (first, info), so a pop needs no node fetch -- at the plain
// culling slack (no node_mu: that proof is about the scene's lights).  A child
// is pushed unless the ray misses its slack-grown box or rt_prune says no
// record below it can have new_dist <= tmax; the bound never tightens during
// the walk, so the test at the push is all the pruning there is and an ordered
// stack's entry parameters would never be looked at again.  The children go
// far-to-near in octant order (push_children's), so the nearest is popped
// first: measured against oct_any's storage order and against oct_closest's
// (node, t) stack on C5 -- the fastest of the three on
// incoherent rays, which is what the per-lane walk is for (coherent callers
// have RT_RAYS_PACKET).  With tmax = +inf the limit is +inf and nothing is
// pruned: the nodes oct_any visits without node_mu.
__device__ bool oct_occl(const KParams& p, const Ray& r, const OcclBound& ob, Stack& s, LaneCount& wc) {
  const float4* __restrict__ node = p.node;
  const f3 inv = inv_dir(r.d);
  const uint32_t dm = near_octant(r.d);
  const f3 nd = unit_dir(r);
  s.sp = 0;
  wave_sync();
  {
    const float4 lo = node[0], hi = node[1];
    const float t0 = box_enter(r, inv, lo, hi);
    if (t0 != __builtin_inff() && !rt_prune(t0, r.dlen, ob.tmax, r.eps)) push(s, __float_as_uint(lo.w), hi.w, wc);
  }
  while (s.sp > 0) {
    uint32_t first;
    float info_bits;
    pop(s, first, info_bits);
    const uint32_t info = __float_as_uint(info_bits);
    if (info & RT_NODE_LEAF) {
      if (occl_leaf(p.tri, first, RT_LEAF_COUNT(info), r, nd, ob, wc)) {
        s.sp = 0;
        wave_sync();
        return true;
      }
    } else {
      // child k+1's box in flight while child k is tested
      const uint32_t mask = RT_NODE_MASK(info);
      uint32_t mj = mask_xor(mask, dm);
      if (!mj) continue;
      int j = 31 - __clz(mj);
      mj &= ~(1u << j);
      uint32_t ci = first + (uint32_t)__popc(mask & ((1u << ((uint32_t)j ^ dm)) - 1u));
      float4 nlo = node[2 * ci], nhi = node[2 * ci + 1];
      for (;;) {
        const float4 clo = nlo, chi = nhi;
        const bool more = mj != 0u;
        if (more) {
          j = 31 - __clz(mj);
          mj &= ~(1u << j);
          ci = first + (uint32_t)__popc(mask & ((1u << ((uint32_t)j ^ dm)) - 1u));
          nlo = node[2 * ci];
          nhi = node[2 * ci + 1];
        }
        const float t0 = box_enter(r, inv, clo, chi);
        if (t0 != __builtin_inff() && !rt_prune(t0, r.dlen, ob.tmax, r.eps)) push(s, __float_as_uint(clo.w), chi.w, wc);
        if (!more) break;
      }
    }
  }
  wave_sync();
  return false;
}

// ---- packet form: the wave walks the union of its lanes' walks (staged_any),
// the children pushed through stage_push_children<false> with each lane's own
// limit rt_prune_limit(tmax, eps), the leaves' records tested as LDS
// broadcasts; a lane drops out at its first hit and the wave leaves when no
// lane searches.
__device__ bool staged_occl(const KParams& p, const Ray& r, const OcclBound& ob, bool act, WaveCtx& w, WorkCount& wc) {
  const float4* __restrict__ node = p.node;
  const float4* __restrict__ tri = p.tri;
  bool alive = act, hit = false;
  uint32_t risk = 0;
  const uint64_t am = __ballot(alive);
  if (am == 0) return false;
  const f3 inv = inv_dir(r.d);
  const uint32_t dm = wave_near_octant(act, r.d, am);
  const f3 nd = unit_dir(r);
  const float limit = rt_prune_limit(ob.tmax, r.eps);
  int sp = 0;
  wave_sync();
  if (w.lane < 2) w.stk2[w.lane] = node[w.lane];
  if (w.lane == 0) w.stkm[0] = am;
  sp = 1;
  while (sp > 0) {
    --sp;
    wave_sync();
    const float4 lo = w.stk2[2 * sp], hi = w.stk2[2 * sp + 1];
    const uint64_t lm = w.stkm[sp];
    const uint32_t first = uni(__float_as_uint(lo.w)), info = uni(__float_as_uint(hi.w));
    // the bound does not tighten: the lanes that wanted the node when it was
    // pushed and still search want it now (no re-test)
    bool want = alive && ((lm >> w.lane) & 1) != 0;
    if (__ballot(want) == 0) continue;
    if (info & RT_NODE_LEAF) {
      const uint32_t cnt = RT_LEAF_COUNT(info);
      for (uint32_t base = 0; base < cnt && __ballot(want) != 0; base += kOctRecs) {
        const uint32_t m = chunk<kOctRecs>(cnt, base);
        stage_load<kStageOct>(tri + 3 * (size_t)(first + base), 3 * (int)m, w);
        for (uint32_t k = 0; k < m; k++) {
          const float4 q0 = w.stage[3 * k], q1 = w.stage[3 * k + 1], q2 = w.stage[3 * k + 2];
          if (want && occl_rec(r, nd, ob, q0, q1, q2, risk)) {
            hit = true;
            alive = false;
            want = false;
          }
          if (__ballot(want) == 0) break;
        }
      }
      if (__ballot(alive) == 0) break;
    } else {
      stage_load<kStageOct>(node + 2 * (size_t)first, 2 * (int)RT_NODE_COUNT(info), w);
      stage_push_children<false>(r, inv, dm, info, wave_ballot(want), limit, sp, w, wc);
    }
  }
  wc.zero_risk += (uint32_t)__popcll(__ballot(risk != 0));
  return hit;
}

// The octree routes of a batch query with the bound `ob`, for occl_q and for
// direct light's dlight_q (rt_dlight.h); walk is wave-uniform (OcclArgs::walk).
// BOUNDED: the exact route's winner occludes only within ob.tmax (without it any
// winner does).  Converged call, act = the lane makes a query.
// (The FLAT route stays with the two callers: through this function the FLAT
// kernels' scalar register numbering changed.)
template <bool BOUNDED>
__device__ __forceinline__ bool occl_oct(const KParams& p, const Ray& r, const OcclBound& ob, bool act, uint32_t walk,
                                         Stack& s, WaveCtx& w, WorkCount& wc) {
  if (walk & RT_RAYS_WALK_EXACT) {
    // the proven closest walk, answering dist <= tmax; the winner's object
    // flag (its record, prim order) is the zero-normal risk
    Best b = best_none();
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) {
      oct_closest_rf<false>(p, r, b, s, lc);
      if (b.dist != __builtin_inff()) lc.risk |= __float_as_uint(p.tri_prim[3 * (size_t)b.prim + 2].w) & RT_REC_ZERO_RISK;
    }
    absorb<false>(wc, lc, true);
    return act && b.dist != __builtin_inff() && (!BOUNDED || b.dist <= ob.tmax);
  }
  if (walk & RT_RAYS_WALK_PACKET) return staged_occl(p, r, ob, act, w, wc);
  LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool hit = act && oct_occl(p, r, ob, s, lc);
  absorb<false>(wc, lc, true);
  return hit;
}

// The batch's query: within the ray's tmax.
template <int ACCEL>
__device__ __forceinline__ bool occl_q(const KParams& p, const Ray& r, float tmax, bool act, uint32_t walk, Stack& s,
                                       WaveCtx& w, WorkCount& wc) {
  const OcclBound ob = occl_bound(r, tmax);
  if (ACCEL == RT_ACCEL_FLAT_D) return use_tp(p, act) ? flat_occl_tp(p, r, ob, act, wc) : flat_occl_w(p, r, ob, act, w, wc);
  return occl_oct<true>(p, r, ob, act, walk, s, w, wc);
}

// Occlusion batch: a work item is 64 consecutive rays, lane = ray, on
// rays_trace_kernel's persistent one-wave workgroups and 8 item streams
// (rt_ray_items.h).  Each item loads o, d and tmax, decides which lanes are
// traced and which of them query (rt_occl_items.h), runs the batch's walk and
// stores the lane's byte; bytes past the batch's end are not written.
template <int ACCEL>
__global__ __launch_bounds__(64, RT_TRACE_MIN_WAVES) void rays_occl_kernel(KParams p, OcclArgs a) {
  const int lane = threadIdx.x & 63;
  WorkCount wc = {};
  __shared__ float4 s_stack[ACCEL == RT_ACCEL_FLAT_D ? 1 : kStackArea];
  __shared__ float4 s_stage[ACCEL == RT_ACCEL_FLAT_D ? kStageFlat : kStageOct];
  Stack stk;
  WaveCtx w;
  wave_state(p, s_stack, s_stage, lane, stk, w);
  const uint32_t home = (uint32_t)blockIdx.x & 7u;
  uint32_t probe = 0;
  bool first = true;
  for (;;) {
    const uint32_t x = (home + probe) & 7u;
    uint32_t q = 0;
    if (first) {
      q = (uint32_t)blockIdx.x >> 3;
      first = false;
    } else {
      if (lane == 0) q = atomicAdd(p.tile_counter + 32u * x, 1u);
      q = uni(q) + (gridDim.x - x + 7u) / 8u;
    }
    if (q >= rt_ray_stream_items(a.nitems, x)) {
      if (++probe == 8u) break;  // every stream drained: the wave exits
      continue;
    }
    const size_t i = (size_t)rt_ray_stream_item(q, x) * RT_RAY_ITEM + (size_t)lane;
    // a lane without a query walks nothing, but its ray takes part in the
    // packet walk's wave-wide arithmetic: a harmless one
    f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
    float tmax = __builtin_inff();
    bool traced = false, query = false;
    if (i < a.n) {
      const f3 ro = ld3(a.org + 3 * i), rd = ld3(a.dir + 3 * i);
      const float rt = a.tmax ? a.tmax[i] : __builtin_inff();
      const uint32_t ob[3] = {__float_as_uint(ro.x), __float_as_uint(ro.y), __float_as_uint(ro.z)};
      const uint32_t db[3] = {__float_as_uint(rd.x), __float_as_uint(rd.y), __float_as_uint(rd.z)};
      traced = rt_occl_traced(ob, db, __float_as_uint(rt));
      query = rt_occl_queried(ob, db, __float_as_uint(rt));
      if (query) o = ro, d = rd, tmax = rt;
    }
    wc.pixels += (uint32_t)__popcll(__ballot(traced));  // the rays traced (rt_stats.camera of a batch)
    wc.shadow += (uint32_t)__popcll(__ballot(query));   // the queries
    const Ray r = make_ray(p, o, d, p.eps_rel);
    const bool hit = occl_q<ACCEL>(p, r, tmax, query, a.walk, stk, w, wc);
    if (i < a.n) a.out[i] = hit ? 1 : 0;
  }
  flush_counts(p, wc, lane, true);
}

}  // namespace rt
