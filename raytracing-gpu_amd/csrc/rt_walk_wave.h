// rt_walk_wave.h -- the wave-wide walks: wave-uniform loads (uni, ldu), the
// wave's LDS stage and stack (WaveCtx, Fetch), the brute-force loops streamed
// through LDS (flat_*_w) or triangle-parallel (flat_*_tp), and the staged
// packet walk of the octree (stage_push_children, staged_closest, staged_any).
// Part of rt_render.hip's one translation unit.  Needs rt_walk_lane.h
// (included here: the box tests, kLdsStack for the shared stack area).
#pragma once

#include "rt_push_plan.h"
#include "rt_walk_lane.h"

namespace rt {

__device__ __forceinline__ uint32_t uni(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
// v_writelane_b32: `old` with lane `l` (wave-uniform) replaced by the wave-uniform x.  clang has
// no builtin of that name; the declaration binds the LLVM intrinsic itself.
__device__ int wave_writelane(int x, int l, int old) __asm("llvm.amdgcn.writelane");
// Wave-uniform loads through the constant address space: with a uniform
// address they become scalar (SMEM) loads straight into SGPRs.  The scene
// image is read-only for the whole launch.
__device__ __forceinline__ float4 ldu(const float4* p, size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) float4 cfloat4;
  return ((cfloat4*)p)[i];
#else
  return p[i];  // host pass only parses device code
#endif
}

// majority ray-direction octant of the active lanes (child push order)
__device__ __forceinline__ uint32_t wave_near_octant(bool act, f3 d, uint64_t am) {
  int na = __popcll(am);
  uint32_t dm = 0;
  if (2 * __popcll(__ballot(act && d.x < 0.0f)) > na) dm |= 1u;
  if (2 * __popcll(__ballot(act && d.y < 0.0f)) > na) dm |= 2u;
  if (2 * __popcll(__ballot(act && d.z < 0.0f)) > na) dm |= 4u;
  return dm;
}

// ------------------------------------------- PACKET walk, LDS-staged records
// The 64 lanes of a wave walk the octree together: every fetch is one
// coalesced vector load by the lanes (lane k loads float4 k of the records)
// staged in LDS, then read back as broadcasts: a leaf's triangle records (3
// float4 each, 32 per chunk) or an interior node's child boxes (2 float4
// each, <= 8 children, contiguous) cost one memory round trip instead of one
// per record.  The wave stack holds the pushed child's whole node record (box
// + first/info) and the mask of the lanes that wanted it, so a pop needs no
// memory access before the next fetch is issued.  Camera rays of an 8x8 tile
// are coherent, so the union of the lanes' walks is barely larger than each
// one's.
// float4 staging slots per wave: FLAT streams 64 triangle records at a time;
// the octree walk stages one node's payload (<= 8 children, or a leaf's
// records, RT_OCT_LEAF_CAP = 32 of them in one chunk).  LDS per one-wave
// workgroup must stay <= 10 KB for 16 workgroups per CU.
static constexpr int kStageFlat = 192;
static constexpr int kStageOct = 96;
static constexpr int kStageKids = 16;  // of them, an interior node's <= 8 child boxes
static constexpr int kStack2 = 96;  // wave stack entries (2 float4 each)
// float4 slots of the stack area: the staged walk's kStack2 x (2 float4 + a
// lane mask), or the per-lane stacks' kLdsStack x 64 x (index, t)
static constexpr int kStackArea = (2 * kStack2 * 16 + kStack2 * 8 > kLdsStack * 64 * 8
                                       ? 2 * kStack2 * 16 + kStack2 * 8
                                       : kLdsStack * 64 * 8) / 16;

struct WaveCtx {
  float4* stk2;    // kStack2 x 2 float4
  uint64_t* stkm;  // kStack2 lane masks: lanes that wanted the pushed node
  float4* stage;   // kStageFlat / kStageOct float4
  int lane;
};

// A wave's walk state from its kernel's two LDS arrays (declared there: their
// sizes differ per kernel).  The per-lane stacks and the staged wave stack
// share one LDS area: a wave runs one walk at a time and every walk starts and
// ends with an empty stack (wave_sync() at both ends orders the accesses).
__device__ __forceinline__ void wave_state(const KParams& p, float4* s_stack, float4* s_stage, int lane, Stack& stk,
                                           WaveCtx& w) {
  lane_stack(p, s_stack, lane, stk);
  w.stk2 = s_stack;
  w.stkm = (uint64_t*)(s_stack + 2 * kStack2);
  w.stage = s_stage;
  w.lane = lane;
}

// A fetch in flight: the wave's lanes hold float4 k, k+64, k+128 of src[0, n)
// in registers (issued early so its latency overlaps other work), then commit
// it to the LDS stage; n <= NMAX <= kStageFlat.  NMAX is the caller's bound on
// n: the octree walks stage at most kStageOct float4, so their third slot
// (l + 128 < n) can never be taken and is not compiled; the flat walks keep it.
struct Fetch {
  float4 v0, v1, v2;
  int n;
};

template <int NMAX>
__device__ __forceinline__ Fetch fetch_issue(const float4* __restrict__ src, int n, int l) {
  static_assert(NMAX <= kStageFlat, "a fetch is at most three float4 per lane");
  Fetch f;
  f.n = n;
  if (l < n) f.v0 = src[l];
  if (NMAX > 64 && l + 64 < n) f.v1 = src[l + 64];
  if (NMAX > 128 && l + 128 < n) f.v2 = src[l + 128];
  return f;
}

template <int NMAX>
__device__ __forceinline__ void fetch_commit(const Fetch& f, WaveCtx& w) {
  const int l = w.lane;
  wave_sync();  // after the previous readers of stage
  if (l < f.n) w.stage[l] = f.v0;
  if (NMAX > 64 && l + 64 < f.n) w.stage[l + 64] = f.v1;
  if (NMAX > 128 && l + 128 < f.n) w.stage[l + 128] = f.v2;
  wave_sync();
}

template <int NMAX>
__device__ __forceinline__ void stage_load(const float4* __restrict__ src, int n, WaveCtx& w) {
  fetch_commit<NMAX>(fetch_issue<NMAX>(src, n, w.lane), w);
}

template <int RECS>
__device__ __forceinline__ uint32_t chunk(uint32_t n, uint32_t base) {
  return n - base < (uint32_t)RECS ? n - base : (uint32_t)RECS;
}
static constexpr int kFlatRecs = kStageFlat / 3;
static constexpr int kOctRecs = kStageOct / 3;

// Brute force over every triangle record (cpu/hit.c:72-109 order-free, the
// (new_dist, prim) key makes the winner order-independent), streamed through
// LDS 64 records at a time with the next chunk's fetch in flight while the
// current one is tested; converged calls.
template <bool COUNT>
__device__ void flat_closest_w(const KParams& p, const Ray& r, bool act, Best& b, WaveCtx& w,
                               WorkCount& wc) {
  if (__ballot(act) == 0) return;
  const uint32_t n = p.nrec;
  Fetch f = fetch_issue<kStageFlat>(p.tri, 3 * (int)chunk<kFlatRecs>(n, 0), w.lane);
  for (uint32_t base = 0; base < n; base += kFlatRecs) {
    uint32_t m = chunk<kFlatRecs>(n, base);
    fetch_commit<kStageFlat>(f, w);
    uint32_t nb = base + kFlatRecs;
    if (nb < n) f = fetch_issue<kStageFlat>(p.tri + 3 * (size_t)nb, 3 * (int)chunk<kFlatRecs>(n, nb), w.lane);
    // two records per step (mt_candidate2: two independent chains), the
    // survivors tested exactly in record order
    uint32_t k = 0;
    for (; k + 1 < m; k += 2) {
      const float4 qa[3] = {w.stage[3 * k], w.stage[3 * k + 1], w.stage[3 * k + 2]};
      const float4 qb[3] = {w.stage[3 * k + 3], w.stage[3 * k + 4], w.stage[3 * k + 5]};
      bool ca = false, cb = false;
      if (act) mt_candidate2(r.o, r.d, qa, qb, b.t_cut, ca, cb);
      if (ca) consider_exact(r, qa[0], qa[1], qa[2], b);
      if (cb) consider_exact(r, qb[0], qb[1], qb[2], b);
    }
    if (k < m) {
      const float4 q0 = w.stage[3 * k], q1 = w.stage[3 * k + 1], q2 = w.stage[3 * k + 2];
      if (act) consider(r, q0, q1, q2, b);
    }
  }
  if (COUNT) {
    wc.tris += n;
    wc.cl_tris += n * (uint32_t)__popcll(__ballot(act));
  }
}

template <bool COUNT>
__device__ bool flat_any_w(const KParams& p, const Ray& r, bool act, WaveCtx& w, WorkCount& wc) {
  bool alive = act, hit = false;
  uint32_t risk = 0;
  const uint32_t n = p.nrec;
  if (__ballot(alive) == 0 || n == 0) return false;
  Fetch f = fetch_issue<kStageFlat>(p.tri, 3 * (int)chunk<kFlatRecs>(n, 0), w.lane);
  for (uint32_t base = 0; base < n; base += kFlatRecs) {
    uint32_t m = chunk<kFlatRecs>(n, base);
    fetch_commit<kStageFlat>(f, w);
    uint32_t nb = base + kFlatRecs;
    if (nb < n) f = fetch_issue<kStageFlat>(p.tri + 3 * (size_t)nb, 3 * (int)chunk<kFlatRecs>(n, nb), w.lane);
    if (COUNT) {
      wc.tris += m;
      wc.sh_tris += m * (uint32_t)__popcll(__ballot(alive));
    }
    // two records per step (mt_candidate2), as flat_closest_w
    uint32_t k = 0;
    for (; k + 1 < m; k += 2) {
      const float4 qa[3] = {w.stage[3 * k], w.stage[3 * k + 1], w.stage[3 * k + 2]};
      const float4 qb[3] = {w.stage[3 * k + 3], w.stage[3 * k + 4], w.stage[3 * k + 5]};
      bool ca = false, cb = false;
      if (alive) mt_candidate2(r.o, r.d, qa, qb, __builtin_inff(), ca, cb);
      if ((ca && any_hit_exact(r, qa[0], qa[1], qa[2], risk)) ||
          (cb && any_hit_exact(r, qb[0], qb[1], qb[2], risk))) {
        hit = true;
        alive = false;
      }
      if (__ballot(alive) == 0) break;
    }
    if (k < m && __ballot(alive) != 0) {
      const float4 q0 = w.stage[3 * k], q1 = w.stage[3 * k + 1], q2 = w.stage[3 * k + 2];
      if (alive && any_hit_rec(r, q0, q1, q2, risk)) {
        hit = true;
        alive = false;
      }
    }
    if (__ballot(alive) == 0) break;
  }
  wc.zero_risk += (uint32_t)__popcll(__ballot(risk != 0));
  return hit;
}

// Brute force, TRIANGLE-parallel: for a wave with few active lanes (deep
// reflection bounces, shadow rays of the lanes that hit, sky pixels), the
// lanes take turns: the active lane's ray is broadcast and the 64 lanes test
// 64 different triangles at a time, then the lexicographic (new_dist, prim)
// minimum is reduced across the wave -- the same decisions in another order
// (the key makes the winner order-independent).  Ray-parallel streaming pays
// the whole triangle list per wave however few lanes still query.
__device__ __forceinline__ Ray ray_of_lane(const Ray& r, int l) {
  Ray q;
  q.o = f3{__shfl(r.o.x, l), __shfl(r.o.y, l), __shfl(r.o.z, l)};
  q.d = f3{__shfl(r.d.x, l), __shfl(r.d.y, l), __shfl(r.d.z, l)};
  q.dlen = __shfl(r.dlen, l);
  q.eps = 0.0f;
  q.oh = q.o;
  q.ol = q.o;
  return q;
}

template <bool COUNT>
__device__ void flat_closest_tp(const KParams& p, const Ray& r, bool act, Best& b, WorkCount& wc) {
  const uint32_t n = p.nrec;
  const int lane = (int)(threadIdx.x & 63);
  uint64_t am = __ballot(act);
  if (COUNT) {
    wc.tris += n * (uint32_t)__popcll(am);
    wc.cl_tris += n * (uint32_t)__popcll(am);
  }
  while (am) {
    const int l = __ffsll((unsigned long long)am) - 1;
    am &= am - 1;
    const Ray q = ray_of_lane(r, l);
    Best mb = best_none();
    for (uint32_t base = 0; base < n; base += 64) {
      const uint32_t i = base + (uint32_t)lane;
      if (i < n) {
        const float4* t = p.tri + 3 * (size_t)i;
        consider(q, t[0], t[1], t[2], mb);
      }
    }
    // wave minimum of (dist, prim); the winner's obj, u, v, t travel with it
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float od = __shfl_xor(mb.dist, off);
      const uint32_t op = __shfl_xor(mb.prim, off), oo = __shfl_xor(mb.obj, off);
      const float ou = __shfl_xor(mb.u, off), ov = __shfl_xor(mb.v, off), ot = __shfl_xor(mb.t, off);
      if (od < mb.dist || (od == mb.dist && op < mb.prim)) {
        mb.dist = od;
        mb.prim = op;
        mb.obj = oo;
        mb.u = ou;
        mb.v = ov;
        mb.t = ot;
      }
    }
    if (lane == l) {
      b.dist = mb.dist;
      b.prim = mb.prim;
      b.obj = mb.obj;
      b.u = mb.u;
      b.v = mb.v;
      b.t = mb.t;
    }
  }
}

template <bool COUNT>
__device__ bool flat_any_tp(const KParams& p, const Ray& r, bool act, WorkCount& wc) {
  const uint32_t n = p.nrec;
  const int lane = (int)(threadIdx.x & 63);
  uint64_t am = __ballot(act);
  bool res = false;
  uint32_t risk = 0;  // per lane: any tested triangle's flag (conservative)
  while (am) {
    const int l = __ffsll((unsigned long long)am) - 1;
    am &= am - 1;
    const Ray q = ray_of_lane(r, l);
    bool hit = false;
    uint32_t base = 0;
    for (; base < n && !hit; base += 64) {  // hit is wave-uniform (ballot)
      const uint32_t i = base + (uint32_t)lane;
      bool h = false;
      if (i < n) {
        const float4* t = p.tri + 3 * (size_t)i;
        h = any_hit_rec(q, t[0], t[1], t[2], risk);
      }
      hit = __ballot(h) != 0;
    }
    if (COUNT) {
      const uint32_t tested = base < n ? base : n;
      wc.tris += tested;
      wc.sh_tris += tested;
    }
    if (lane == l) res = hit;
  }
  wc.zero_risk += (uint32_t)__popcll(__ballot(risk != 0));
  return res;
}

// Interior node whose child boxes are staged: test them, push the ones any
// lane wants (with the mask of the lanes that want each) far-to-near in
// octant order, so the nearest child ends on top of the stack.  The pushes
// are one vector step, not a loop over the octants: which slot each child
// takes is a function of the wave-uniform mask, dm and the children's
// ballots alone (csrc/rt_push_plan.h), and the stack ends up byte for byte
// what the serial loop left.
// rt_box_wants (rt_cull.h) of every lane as the wave's mask: one ballot per
// compare, ANDed in scalar registers.  (A ballot of the helper's own && is a
// ballot of no compare: the compiler selects 0 / 1 into a VGPR and compares
// that again, two VALU instructions per box.)
__device__ __forceinline__ uint64_t box_wants_w(bool hit, float tmin, float dlen, float limit) {
  return wave_ballot(hit) & wave_ballot(tmin != __builtin_inff()) & wave_ballot(rt_box_within(tmin, dlen, limit));
}

// wm: the lanes that want the node.
template <bool ANY>
__device__ __forceinline__ void stage_push_children(const Ray& r, f3 inv, uint32_t dm,
                                                    uint32_t info, uint64_t wm, float limit,
                                                    int& sp, WaveCtx& w, WorkCount& wc,
                                                    const float2* __restrict__ mu = nullptr) {
  const uint32_t mask = RT_NODE_MASK(info), cnt = RT_NODE_COUNT(info);
  // lane c keeps the mask of the lanes that want child c (v_writelane of the
  // compares' own scalar pairs): the ballots never sit in scalar registers
  // past their own child's test
  int wlo = 0, whi = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    if ((uint32_t)c < cnt) {
      float4 clo = w.stage[2 * c], chi = w.stage[2 * c + 1];
      uint64_t bc;
      if (ANY) {
        bc = wm & (mu ? wave_ballot(box_hit_sh(r, inv, clo, chi, mu[c]))  // exact-shadow mode's grown boxes
                      : wave_ballot(box_enter(r, inv, clo, chi) != __builtin_inff()));
      } else {
        float t0;
        const bool hit = box_hit(r, inv, clo, chi, t0);
        bc = wm & box_wants_w(hit, t0, r.dlen, limit);
      }
      wlo = wave_writelane((int)(uint32_t)bc, c, wlo);
      whi = wave_writelane((int)(uint32_t)(bc >> 32), c, whi);
    }
  }
  // One push step for the whole node (csrc/rt_push_plan.h): lane k < 8 takes
  // push-order key k, fetches its child's lane mask from lane `child` and the
  // child's record from the stage in one LDS round trip, and stores both at
  // its own slot.  The slots, sp and the overflow count are the serial
  // far-to-near loop's.
  const RtPushLane pl = rt_push_lane(mask, dm, (uint32_t)w.lane);
  const uint32_t mlo = (uint32_t)__shfl(wlo, (int)pl.child), mhi = (uint32_t)__shfl(whi, (int)pl.child);
  float4 rlo, rhi;
  if (w.lane < 8) {  // child <= 8: inside the stage whatever the key
    rlo = w.stage[2 * pl.child];
    rhi = w.stage[2 * pl.child + 1];
  }
  const bool push = w.lane < 8 && rt_push_wanted(pl, ((mlo | mhi) != 0 ? 1u : 0u) << pl.child);
  const uint32_t B = (uint32_t)wave_ballot(push);
  const int slot = sp + (int)rt_push_rank(B, (uint32_t)w.lane);
  if (push && slot < kStack2) {
    w.stk2[2 * slot] = rlo;
    w.stk2[2 * slot + 1] = rhi;
    w.stkm[slot] = (uint64_t)mhi << 32 | mlo;
  }
  uint32_t over;
  sp += (int)rt_push_commit(B, sp, kStack2, &over);
  wc.overflow += over;  // RT_EDEPTH, never silent
}

template <bool COUNT>
__device__ void staged_closest(const KParams& p, const Ray& r, bool act, Best& b, WaveCtx& w,
                               WorkCount& wc) {
  const float4* __restrict__ node = p.node;
  const float4* __restrict__ tri = p.tri;
  uint64_t am = __ballot(act);
  if (am == 0) return;
  f3 inv = inv_dir(r.d);
  uint32_t dm = wave_near_octant(act, r.d, am);
  int sp = 0;
  wave_sync();
  if (w.lane < 2) w.stk2[w.lane] = node[w.lane];
  if (w.lane == 0) w.stkm[0] = am;
  sp = 1;
  float limit = rt_prune_limit(b.dist, r.eps);
  bool pruning = wave_ballot(b.dist != __builtin_inff()) != 0;  // some lane has a best
  while (sp > 0) {
    --sp;
    wave_sync();
    float4 lo = w.stk2[2 * sp], hi = w.stk2[2 * sp + 1];
    uint64_t lm = w.stkm[sp];
    uint32_t first = uni(__float_as_uint(lo.w)), info = uni(__float_as_uint(hi.w));
    bool leaf = (info & RT_NODE_LEAF) != 0;
    uint32_t cnt = leaf ? RT_LEAF_COUNT(info) : RT_NODE_COUNT(info);
    // issue the node's payload fetch now; its latency overlaps the re-test
    Fetch f = leaf ? fetch_issue<kStageOct>(tri + 3 * (size_t)first, 3 * (int)chunk<kOctRecs>(cnt, 0), w.lane)
                   : fetch_issue<kStageKids>(node + 2 * (size_t)first, 2 * (int)cnt, w.lane);
    // Lanes that wanted it when pushed, re-tested against their best so far.
    // Such a lane passed rt_box_wants on these very floats when the node was
    // pushed, so its box is hit and the re-test is rt_box_within (rt_cull.h)
    // alone: the exit parameter is not computed.  A lane without a best has
    // limit = +inf and passes; the whole re-test is skipped while no lane has
    // one.  (The root is pushed untested, and popped before any leaf.)
    bool want = ((lm >> w.lane) & 1) != 0;
    uint64_t wm = wave_ballot(want);
    if (pruning) {
      float tn;
      box_hit(r, inv, lo, hi, tn);
      const bool within = rt_box_within(tn, r.dlen, limit);
      want = want && within;
      wm &= wave_ballot(within);
    }
    if (wm == 0) continue;
    if (COUNT) {
      wc.nodes++;
      wc.cl_nodes += (uint32_t)__popcll(__ballot(want));
    }
    fetch_commit<kStageOct>(f, w);
    if (leaf) {
      for (uint32_t base = 0; base < cnt; base += kOctRecs) {
        uint32_t m = chunk<kOctRecs>(cnt, base);
        if (base) stage_load<kStageOct>(tri + 3 * (size_t)(first + base), 3 * (int)m, w);
        stage_test(r, want, wm, m, b, w.stage);
      }
      limit = rt_prune_limit(b.dist, r.eps);
      pruning = wave_ballot(b.dist != __builtin_inff()) != 0;
      if (COUNT) {
        wc.tris += cnt;
        wc.cl_tris += cnt * (uint32_t)__popcll(__ballot(want));
      }
    } else {
      stage_push_children<false>(r, inv, dm, info, wm, limit, sp, w, wc);
    }
  }
}

template <bool COUNT>
__device__ bool staged_any(const KParams& p, const Ray& r, bool act, WaveCtx& w, WorkCount& wc) {
  const float4* __restrict__ node = p.node;
  const float4* __restrict__ tri = p.tri;
  bool alive = act, hit = false;
  uint32_t risk = 0;
  uint64_t am = __ballot(alive);
  if (am == 0) return false;
  f3 inv = inv_dir(r.d);
  uint32_t dm = wave_near_octant(act, r.d, am);
  int sp = 0;
  wave_sync();
  if (w.lane < 2) w.stk2[w.lane] = node[w.lane];
  if (w.lane == 0) w.stkm[0] = am;
  sp = 1;
  while (sp > 0) {
    --sp;
    wave_sync();
    float4 lo = w.stk2[2 * sp], hi = w.stk2[2 * sp + 1];
    uint64_t lm = w.stkm[sp];
    uint32_t first = uni(__float_as_uint(lo.w)), info = uni(__float_as_uint(hi.w));
    // any-hit has no pruning: the lanes that wanted the node when it was
    // pushed and still search want it now (no re-test)
    bool want = alive && ((lm >> w.lane) & 1) != 0;
    if (__ballot(want) == 0) continue;
    if (COUNT) {
      wc.nodes++;
      wc.sh_nodes += (uint32_t)__popcll(__ballot(want));
    }
    if (info & RT_NODE_LEAF) {
      uint32_t cnt = RT_LEAF_COUNT(info);
      for (uint32_t base = 0; base < cnt && __ballot(want) != 0; base += kOctRecs) {
        uint32_t m = chunk<kOctRecs>(cnt, base);
        stage_load<kStageOct>(tri + 3 * (size_t)(first + base), 3 * (int)m, w);
        if (COUNT) wc.tris += m;
        for (uint32_t k = 0; k < m; k++) {
          if (COUNT) wc.sh_tris += (uint32_t)__popcll(__ballot(want));
          float4 q0 = w.stage[3 * k], q1 = w.stage[3 * k + 1], q2 = w.stage[3 * k + 2];
          if (want && any_hit_rec(r, q0, q1, q2, risk)) {
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
      stage_push_children<true>(r, inv, dm, info, wave_ballot(want), 0.0f, sp, w, wc,
                                p.node_mu ? p.node_mu + first : nullptr);
    }
  }
  wc.zero_risk += (uint32_t)__popcll(__ballot(risk != 0));
  return hit;
}

}  // namespace rt
