// rt_query.h -- the queries the kernels ask: the traversal policy's choice
// of walk for a closest hit (closest_q), the shadow query through a light's
// buffer (LbRange, lbuf_range, lbuf_scan, lbuf_any; built by
// csrc/rt_lightbuf.hip, the cells a ray looks up: csrc/rt_lightbuf_cell.h) or
// a walk (shadow_q), and the camera rays' candidate lists (cand_range,
// cand_closest; built by csrc/rt_cand.hip).
// Part of rt_render.hip's one translation unit.  Needs rt_walk_lane.h and
// rt_walk_wave.h (included here).
#pragma once

#include "rt_lightbuf_cell.h"
#include "rt_shade_rows.h"
#include "rt_walk_lane.h"
#include "rt_walk_wave.h"

namespace rt {

// Traversal policy of an instantiation (RT_POLICY_*, rt_kernels.h).  The
// default: closest-hit queries walk as a staged packet while at least
// kPacketMin lanes query at a bounce depth <= kPacketMaxDepth (camera rays;
// reflections are incoherent), else per lane;
// shadow queries walk per lane, except directional-light shadows (parallel
// rays, cpu/light.c:53) under RT_POLICY_DIR_STAGED.
static constexpr int kPacketMin = 8;
// (The camera packet walk with the next node's payload copied global -> LDS
// while a leaf is tested measured slower -- round 5, profiles/r07_prefetch/:
// a second LDS stage costs occupancy, and at full occupancy the other waves
// already cover the payload latency -- and was removed.)
// Camera rays only (round 4): the reflection rays of a wave diverge, and a
// packet walks the union of their paths through cold nodes; per lane, the
// longest items of an 8-way split (reflection-heavy tiles, tools/tile_cost.py)
// finish sooner -- slowest of 8 ranks 3.13 -> 2.95 ms, C5 at N = 1 10.07 ->
// 10.04 ms (profiles/r05s_packet_depth/; round 2 measured 0 and 1 equal at N = 1)
#ifndef RT_PACKET_MAX_DEPTH
#define RT_PACKET_MAX_DEPTH 0
#endif
static constexpr int kPacketMaxDepth = RT_PACKET_MAX_DEPTH;

// Brute force: triangle-parallel when the list is long enough to fill the
// lanes and at most kTpMaxLanes lanes query (ray-parallel streaming costs the
// same list per wave whatever the active count; triangle-parallel costs it
// once per active lane, spread over 64 lanes).  Measured on C2 (spheres,
// 4,812 triangles, 1080p, flat): never 262 ms, <= 32 lanes 160, <= 48 160,
// <= 56 159, always 250; shadows always triangle-parallel 170
// (profiles/r02q_flat_tp/).
static constexpr int kTpMaxLanes = 48;
__device__ __forceinline__ bool use_tp(const KParams& p, bool act) {
  return p.nrec >= 256u && __popcll(__ballot(act)) <= kTpMaxLanes;
}

// Closest-hit query; converged call, act = lane has a query.
template <int ACCEL, bool COUNT, int POL>
__device__ __forceinline__ void closest_q(const KParams& p, const Ray& r, bool act, int depth, Best& b,
                                          Stack& s, WaveCtx& w, WorkCount& wc) {
  if (ACCEL == RT_ACCEL_FLAT_D) {
    if (use_tp(p, act))
      flat_closest_tp<COUNT>(p, r, act, b, wc);
    else
      flat_closest_w<COUNT>(p, r, act, b, w, wc);
    return;
  }
  if (POL == RT_POLICY_EXACT_REFL && depth > 0) {  // reflection rays: the proven walk
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) oct_closest_rf<COUNT>(p, r, b, s, lc);
    absorb<COUNT>(wc, lc, false);
    return;
  }
  bool staged = POL == RT_POLICY_STAGED ||
                (POL != RT_POLICY_LANE && __popcll(__ballot(act)) >= kPacketMin &&
                 depth <= kPacketMaxDepth);
  if (staged) {
    staged_closest<COUNT>(p, r, act, b, w, wc);
  } else {
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) oct_closest<COUNT>(p, r, b, s, lc);
    absorb<COUNT>(wc, lc, false);
    if (COUNT && depth > 0) {
      uint32_t mn = lc.lnodes, mt = lc.ltris;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        mn = max(mn, (uint32_t)__shfl_xor((int)mn, off));
        mt = max(mt, (uint32_t)__shfl_xor((int)mt, off));
      }
      wc.sec_lane_nodes = max(wc.sec_lane_nodes, uni(mn));
      wc.sec_lane_tris = max(wc.sec_lane_tris, uni(mt));
    }
  }
}

// Closest-hit query of a ray batch (RT_POLICY_RAYS*, csrc/rt_rays.h): what a
// reflection ray's query is on this context -- brute force on FLAT, the proven
// walk under RT_RAYS_WALK_EXACT, else the per-lane slack walk -- and, when the
// batch asks for it, the first query of a work item as one staged packet (the
// walk RT_POLICY_STAGED runs for arbitrary rays, at the same slack).  walk is
// wave-uniform (RayArgs::walk).  Converged call, act = lane has a query.
template <int ACCEL>
__device__ __forceinline__ void rays_closest(const KParams& p, const Ray& r, bool act, int depth, uint32_t walk,
                                             Best& b, Stack& s, WaveCtx& w, WorkCount& wc) {
  if (ACCEL == RT_ACCEL_FLAT_D) {
    closest_q<ACCEL, false, RT_POLICY_DEFAULT>(p, r, act, depth, b, s, w, wc);
    return;
  }
  if (walk & RT_RAYS_WALK_EXACT) {
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) oct_closest_rf<false>(p, r, b, s, lc);
    absorb<false>(wc, lc, false);
  } else if ((walk & RT_RAYS_WALK_PACKET) && depth == 0) {
    staged_closest<false>(p, r, act, b, w, wc);
  } else {
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) oct_closest<false>(p, r, b, s, lc);
    absorb<false>(wc, lc, false);
  }
}

// Shadow query through the light's buffer (built by csrc/rt_lightbuf.hip; the
// listing it relies on: csrc/rt_lightbuf_geom.h): the
// triangles listed in the cell the ray's origin projects to, in key order,
// up to the first any-hit -- for a point light also the opposite cell, whose
// triangles lie beyond the light (cpu/rt's shadow ray does not stop there,
// cpu/hit.c:93-109) -- then the light's global list.  Per lane.
// The cells a shadow ray's query scans and their entry ranges (the first
// memory round trip of a query; shade_record can issue it early).
struct LbRange {
  uint32_t rs[2], re[2];
  float lim;  // key limit of the first range (the second: none)
};

__device__ __forceinline__ LbRange lbuf_range(const RtLightBuf& L, const Ray& r) {
  uint32_t cell[2] = {0xffffffffu, 0xffffffffu};
  float lim = __builtin_inff();  // key limit of cell[0] (cell[1]: none)
  lbuf_cells(L, r.o, r.d, cell, lim);  // rt_lightbuf_cell.h
  // both cells' entry ranges (independent loads)
  LbRange g;
  g.lim = lim;
  for (int h = 0; h < 2; h++) {
    g.rs[h] = 0u;
    g.re[h] = 0u;
    if (cell[h] != 0xffffffffu) {
      g.rs[h] = L.start[cell[h]];
      g.re[h] = L.start[cell[h] + 1];
    }
  }
  return g;
}

// Each range's entries -- the record inline, its key in the prim slot: one
// contiguous load per test, no prim -> record indirection, the next record's
// load in flight.  Then the global list.
// The next entry's record in flight while an entry is tested (round 5):
// +12 VGPRs, so the shade kernel runs at 7 waves per SIMD (RT_SHADE_MIN_WAVES)
// instead of 8 -- C5 shade 1.96 -> 1.85 ms (profiles/r07_shade/; at 8 waves
// it spills: 1.92; at 6: 1.93).  Round 3 measured the lookahead at 8 waves
// only (spills, 2.72 ms).  (The loop without the lookahead was removed.)
// nd = unit_dir(r) (a directional light's: its row's).
template <bool COUNT>
__device__ bool lbuf_scan(const KParams& p, const RtLightBuf& L, const Ray& r, f3 nd, const LbRange& g,
                          LaneCount& lc) {
  for (int h = 0; h < 2; h++) {
    const float q = h == 0 ? g.lim : __builtin_inff();
    // the next entry's record in flight while this one is tested
    uint32_t k = g.rs[h];
    const uint32_t e = g.re[h];
    float4 n0, n1, n2;
    if (k < e) {
      const float4* t = L.rec + 3 * (size_t)k;
      n0 = t[0];
      n1 = t[1];
      n2 = t[2];
    }
    for (; k < e; k++) {
      const float4 a0 = n0, a1 = n1, a2 = n2;
      if (k + 1 < e) {
        const float4* t = L.rec + 3 * (size_t)(k + 1);
        n0 = t[0];
        n1 = t[1];
        n2 = t[2];
      }
      if (a2.y > q) break;
      if (COUNT) {
        lc.tris += lanes_distinct(k);
        lc.ltris++;
      }
      if (any_hit_rec(r, nd, a0, a1, a2, lc.risk)) return true;
    }
  }
  for (uint32_t k = 0; k < L.nglobal; k++) {
    const float4* t = p.tri_prim + 3 * (size_t)L.global[k];
    if (COUNT) {
      lc.tris += lanes_distinct(L.global[k]);
      lc.ltris++;
    }
    if (any_hit_rec(r, nd, t[0], t[1], t[2], lc.risk)) return true;
  }
  return false;
}

template <bool COUNT>
__device__ bool lbuf_any(const KParams& p, const RtLightBuf& L, const Ray& r, LaneCount& lc) {
  return lbuf_scan<COUNT>(p, L, r, unit_dir(r), lbuf_range(L, r), lc);
}

// The shadow ray (o, d) of light li and its unit direction.  A directional
// light's d is scale(v, -1) whatever the origin, so |d| and d / |d| come from
// the light's row (rt_shade_rows.h: the same operations, done once); a point
// light's are computed here.  li wave-uniform.
__device__ __forceinline__ Ray lbuf_ray(const KParams& p, f3 o, f3 d, uint32_t type, uint32_t li, f3& nd) {
  if (type == 1) {
    const LightShade S = LightRowsUniform{p.lshade}[li];
    nd = S.nd;
    return make_ray_len(p, o, d, S.dlen, p.eps_rel);
  }
  const Ray r = make_ray(p, o, d, p.eps_rel);
  nd = unit_dir(r);
  return r;
}

// Shadow query (collide_dist > 0.01, cpu/light.c:24-31) of a light of the
// given type; converged call.
template <int ACCEL, bool COUNT, int POL>
__device__ __forceinline__ bool shadow_q(const KParams& p, f3 o, f3 d, uint32_t type, uint32_t li,
                                         bool act, Stack& s, WaveCtx& w, WorkCount& wc, bool* defer = nullptr,
                                         const LbRange* pre = nullptr, bool can_defer = true) {
  uint64_t am = __ballot(act);
  wc.shadow += (uint32_t)__popcll(am);
  if (ACCEL == RT_ACCEL_FLAT_D) {
    const Ray r = make_ray(p, o, d, p.eps_rel);
    return use_tp(p, act) ? flat_any_tp<COUNT>(p, r, act, wc) : flat_any_w<COUNT>(p, r, act, w, wc);
  }
  if (POL == RT_POLICY_LBUF) {  // every such light has a buffer (rt_hip.cpp): no walk, no global prims
    const RtLightBuf L = lbuf_desc(p.lbuf, li);
    f3 nd;
    const Ray r = lbuf_ray(p, o, d, type, li, nd);
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    bool hit = act && lbuf_scan<COUNT>(p, L, r, nd, pre ? *pre : lbuf_range(L, r), lc);
    absorb<COUNT>(wc, lc, true);
    if (L.proven) {  // as below
      const bool out = act && !(o.x >= L.olo[0] && o.x <= L.ohi[0] && o.y >= L.olo[1] && o.y <= L.ohi[1] &&
                                o.z >= L.olo[2] && o.z <= L.ohi[2]);
      if (defer && can_defer && p.oob) {
        *defer = out;
        if (out) hit = false;
      } else {
        wc.sh_unproven += (uint32_t)__popcll(__ballot(out));
      }
    }
    return hit;
  }
  bool staged = POL == RT_POLICY_STAGED ||
                (POL == RT_POLICY_DIR_STAGED && type == 1 && __popcll(am) >= kPacketMin);
  bool hit, walked = true;
  f3 nd;
  const Ray r = lbuf_ray(p, o, d, type, li, nd);
  if (staged) {
    hit = staged_any<COUNT>(p, r, act, w, wc);
  } else if (p.lbuf && p.lbuf[li].kind != RT_LB_NONE) {
    walked = false;
    // (the descriptor by reference, through the vector cache: by value in
    // SGPRs, this kernel, which keeps the walk's state too, spilled more)
    const RtLightBuf& L = p.lbuf[li];
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    hit = act && lbuf_scan<COUNT>(p, L, r, nd, pre ? *pre : lbuf_range(L, r), lc);
    absorb<COUNT>(wc, lc, true);
    if (L.proven) {
      // the proof assumed origins in its box; the rare others (hit points of
      // float garbage hits far past a triangle, e.g. camera rays grazing a
      // ground plane at the horizon) are decided by brute force over every
      // record after the pass (cpu/hit.c:93-109)
      const bool out = act && !(o.x >= L.olo[0] && o.x <= L.ohi[0] && o.y >= L.olo[1] && o.y <= L.ohi[1] &&
                                o.z >= L.olo[2] && o.z <= L.ohi[2]);
      if (defer && can_defer && p.oob) {  // decided GPU-wide after the pass (rt_launch_shade_fixup)
        *defer = out;
        if (out) hit = false;
      } else {  // (lights past the 32nd) counted, never assumed: RT_EINEXACT
        wc.sh_unproven += (uint32_t)__popcll(__ballot(out));
      }
    }
  } else {
    LaneCount lc = {0, 0, 0, 0, 0, 0, 0, 0};
    hit = act && oct_any<COUNT>(p, r, s, lc);
    absorb<COUNT>(wc, lc, true);
  }
  // the prims whose float error region no slack multiplier bounds
  // (csrc/rt_shadow.hip): tested by every ray the walk found unshadowed (a
  // light buffer's proof covers its light's queries without them)
  if (walked && p.n_sh_global && __ballot(act && !hit)) {
    uint32_t risk = 0;
    for (uint32_t k = 0; k < p.n_sh_global; k++) {
      const float4* q = p.tri_prim + 3 * (size_t)uni(p.sh_global[k]);
      const float4 q0 = ldu(q, 0), q1 = ldu(q, 1), q2 = ldu(q, 2);
      if (act && !hit) hit = any_hit_rec(r, q0, q1, q2, risk);
      if (__ballot(act && !hit) == 0) break;
    }
    wc.zero_risk += (uint32_t)__popcll(__ballot(risk != 0));
  }
  // point lights (exact-shadow mode): the cosine bound assumed origins within
  // sh_omax of the scene centre
  if (walked && type == 2 && p.node_mu) {
    const float m = fmaxf(fabsf(o.x - p.scene_c.x), fmaxf(fabsf(o.y - p.scene_c.y), fabsf(o.z - p.scene_c.z)));
    wc.sh_unproven += (uint32_t)__popcll(__ballot(act && !(m <= p.sh_omax)));
  }
  return hit;
}

// Camera rays: the triangles of this tile's candidate list (csrc/rt_cand.hip)
// and of the global list, tested with the reference's exact arithmetic after
// the walk -- the ones whose float Moller-Trumbore error region reaches
// beyond the walk's culling slack.
// Entries [s, e) of the candidate list (kOctRecs per round: each lane loads
// one entry and its skip bound, the survivors' records are gathered in
// parallel -- one memory round trip -- into the LDS stage, compacted, then
// tested one after another as LDS broadcasts).  bmax: entries whose depth
// skip bound exceeds it cannot win any lane.  Returns the entries tested.
// (The next round's entries in flight while this round's records are gathered
// and tested measured no gain: trace 4.66 / 4.63 vs 4.64 / 4.61 ms on C5,
// profiles/r08_knob_resweep/; removed.)
template <bool COUNT>
__device__ __forceinline__ uint32_t cand_range(const KParams& p, const Ray& r, bool act, uint32_t s, uint32_t e,
                                               float bmax, Best& b, WaveCtx& w) {
  const int lane = w.lane;
  const uint64_t am = wave_ballot(act);
  uint32_t tested = 0;
  for (uint32_t base = s; base < e; base += kOctRecs) {
    uint32_t prim = 0;
    bool keep = false;
    if (lane < kOctRecs && base + lane < e) {
      prim = p.cand[base + lane];
      keep = !(p.cand_skip[base + lane] > bmax);
    }
    const uint64_t m = wave_ballot(keep);
    if (m == 0) continue;
    const uint32_t n = (uint32_t)__popcll(m);
    const uint32_t slot = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    float4 g0, g1, g2;
    if (keep) {
      const float4* q = p.tri_prim + 3 * (size_t)prim;
      g0 = q[0];
      g1 = q[1];
      g2 = q[2];
    }
    wave_sync();  // after the previous readers of stage
    if (keep) {
      w.stage[3 * slot] = g0;
      w.stage[3 * slot + 1] = g1;
      w.stage[3 * slot + 2] = g2;
    }
    wave_sync();
    // (two candidates per step as two scalar chains, as the brute-force loops
    // do, measured slower here: C5 frame 15.96 -> 16.10 ms,
    // profiles/r03f_bench/ab.log; two per packed-float instruction, RT_CAND_PK
    // of round 3, slower too: profiles/r04e_pk/ab.log)
    stage_test(r, act, am, n, b, w.stage);
    tested += n;
  }
  return tested;
}

template <bool COUNT>
__device__ __forceinline__ void cand_closest(const KParams& p, const Ray& r, bool act, uint32_t tile,
                                             Best& b, WaveCtx& w, WorkCount& wc) {
  if (!p.cand_start || __ballot(act) == 0) return;
    // Depth skip: a candidate's float new_dist is at least |pos - o| + its
    // entry's cand_skip (csrc/rt_cand_geom.h Footprint::skip), so one whose bound exceeds every
    // lane's best - |pos - o| (plus the float error of that difference)
    // cannot win here -- one compare instead of a test.  (A per-lane test of
    // the footprint's image-space band, measured: the bands of the long
    // footprints are 6-34 pixels wide, so nearly every listed tile has lanes
    // inside; it removed 1 % of the tests and cost 2.7 ms on C5.)
    float bl = -__builtin_inff();
    if (act)
      bl = b.dist == __builtin_inff() ? __builtin_inff()
                                      : (b.dist - length(sub(p.pos, r.o))) + (2e-3f + 4e-7f * b.dist);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bl = fmaxf(bl, __shfl_xor(bl, off));
    const float bmax = __uint_as_float(uni(__float_as_uint(bl)));
  const uint32_t tested =
      cand_range<COUNT>(p, r, act, uni(p.cand_start[tile]), uni(p.cand_start[tile + 1]), bmax, b, w);
  const uint32_t n_glob = p.n_cand_global_dev ? uni(*p.n_cand_global_dev) : p.n_cand_global;
  for (uint32_t k = 0; k < n_glob; k++) {
    const float4* q = p.tri_prim + 3 * (size_t)uni(p.cand_global[k]);
    float4 q0 = ldu(q, 0), q1 = ldu(q, 1), q2 = ldu(q, 2);
    if (act) consider(r, q0, q1, q2, b);
  }
  if (COUNT) {
    wc.tris += tested + n_glob;
    wc.cl_tris += (tested + n_glob) * (uint32_t)__popcll(__ballot(act));
  }
}

}  // namespace rt
