// rt_render.hip -- the MI355X (gfx950) render kernels.
//
// One lane renders one pixel: the 4 supersamples of cpu/raytracer.c:55-69 in
// the reference order, each a path of closest-hit queries (cpu/raytracer.c:19-34)
// with Phong + shadow-ray shading at every hit (cpu/light.c:33-100).  A wave
// owns an 8x8 pixel tile; waves are persistent and pull tiles from an atomic
// counter, so the irregular per-tile cost balances across the 256 CUs.
//
// Bit-parity with cpu/rt:
//   * -ffp-contract=off, IEEE div/sqrt, f64 sqrt/pow where the reference uses them;
//   * closest hit = lexicographic min of (new_dist, prim) over hits with
//     new_dist > 0.01 (prim = object-major, LIFO-triangle index);
//   * shadow = any hit with new_dist > 0.01 (early exit is exact);
//   * reflection terms are buffered and summed deepest-first.
//
// Acceleration: FLAT tests every triangle record (the reference's brute
// force, cpu/hit.c:72-109) streamed through LDS; OCTREE walks the octree
// (host/accel.c or csrc/rt_build.hip) front to back with conservative
// distance culling, as a wave-wide staged packet (coherent queries) or one
// stack per lane (incoherent ones), then tests the camera-ray candidate
// lists of csrc/rt_cand.hip.
//
// One translation unit in parts: the arithmetic, walks, queries and shading
// live in the headers included below (each says what it holds), the probes
// and the compatibility renderer in rt_probe.h and rt_compat.h, included where
// their kernels stand in the definition order.  This file keeps the tile and
// sample mapping, the trace, shade and fixup kernels, fold, assemble, the
// G-buffer and every launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cull.h"
#include "rt_device.h"
#include "rt_kernels.h"
#include "rt_reflect.h"
#include "rt_tiles.h"

// the parts of this translation unit, in their order of definition
#include "rt_isect.h"
#include "rt_walk_lane.h"
#include "rt_walk_wave.h"
#include "rt_query.h"
#include "rt_shading.h"

namespace rt {

// PPM (row, col) of pixel (row, col) of rank-local tile t (rt_hip.h "Image
// tiling", csrc/rt_tiles.h): 8 x 8 pixels.
__device__ __forceinline__ void tile_pixel(const KParams& p, uint32_t t, int row, int col, int& pr,
                                           int& pc) {
  int tx, ty;
  const int tb = rt_block_side(p.nranks);
  rt_tile_xy(t, (uint32_t)p.rank, (uint32_t)p.nranks, (uint32_t)rt_blocks_x(p.tiles_x, tb), (uint32_t)tb,
             &tx, &ty);
  pr = ty * 8 + row;
  pc = tx * 8 + col;
}

// The wave's counters are wave totals already: one atomic per counter per
// wave.  The wave-distinct record fetches (nodes, tris) of the shade kernel's
// shadow queries go to their own slots, so each kernel's algorithmic bytes
// can be priced on its own (bench.py roofline).
__device__ __forceinline__ void flush_counts(const KParams& p, const WorkCount& wc, int lane,
                                             bool shade = false) {
  uint32_t v[RT_NSTATS];
  v[RT_ST_CLOSEST] = wc.closest, v[RT_ST_SHADOW] = wc.shadow, v[RT_ST_PIXELS] = wc.pixels;
  v[RT_ST_NODE_VISITS] = shade ? 0u : wc.nodes, v[RT_ST_TRI_TESTS] = shade ? 0u : wc.tris;
  v[RT_ST_DEPTH_OVERFLOW] = wc.overflow, v[RT_ST_ZERO_NORMAL] = wc.zero_normal, v[RT_ST_HITS] = wc.hits;
  v[RT_ST_CLOSEST_NODE_LANES] = wc.cl_nodes, v[RT_ST_CLOSEST_TRI_LANES] = wc.cl_tris;
  v[RT_ST_SHADOW_NODE_LANES] = wc.sh_nodes, v[RT_ST_SHADOW_TRI_LANES] = wc.sh_tris;
  v[RT_ST_CYCLES_CAMERA] = wc.cy_cam, v[RT_ST_CYCLES_CAND] = wc.cy_cand, v[RT_ST_CYCLES_SECONDARY] = wc.cy_sec;
  v[RT_ST_CYCLES_SHADOW] = wc.cy_shadow, v[RT_ST_CYCLES_SHADOW_DIRECTIONAL] = wc.cy_shadow_dir;
  v[RT_ST_STACK_SPILLS] = wc.stack_spills, v[RT_ST_SHADOW_ZERO_RISK] = wc.zero_risk;
  v[RT_ST_SHADOW_NODE_VISITS] = shade ? wc.nodes : 0u, v[RT_ST_SHADOW_TRI_TESTS] = shade ? wc.tris : 0u;
  v[RT_ST_SHADOW_UNPROVEN] = wc.sh_unproven, v[RT_ST_CLOSEST_UNPROVEN] = wc.cl_unproven;
#pragma unroll
  for (int k = 0; k < RT_NSTATS; k++)
    if (lane == 0 && v[k])
      atomicAdd(p.stats + (size_t)(blockIdx.x % RT_STAT_SETS) * RT_STAT_STRIDE + k, (unsigned long long)v[k]);
}

// ---------------------------------------------------------- wavefront split
// A render is three launches.  trace_kernel follows every camera sample's
// path of closest hits (cpu/raytracer.c:19-34) and appends one hit record per
// hit -- the bounce never depends on the shading: ray_bounce takes only the
// hit (cpu/raytracer.c:28, cpu/ray.c:16-25) and the next coefficient only the
// material (cpu/raytracer.c:29).  shade_kernel then runs the shadow queries
// and Phong terms of every record (cpu/light.c:33-100) with the 64 lanes of a
// wave on 64 records -- no lane idles on a sky pixel or an ended path -- in a
// lean kernel that keeps more waves resident than the walk-heavy trace, and
// writes the record's term color_mul(local, coef) (cpu/raytracer.c:30).
// fold_kernel sums each path's terms deepest-first (color_add(reflection,
// term) from the deepest call outwards) and a pixel's four samples in the
// reference's order.  The same operations on the same values as the
// recursion, so the same bits; a path's length is bounded only by
// RT_MAX_BOUNCES (cpu/rt: by its stack).

// Hit record, 2 float4: P.xyz N.x | N.y N.z coef bits(obj); its path's
// previous record in hit_prev.  Record index = region | (slot << 3).
__device__ __forceinline__ size_t rec_addr(const KParams& p, uint32_t idx) {
  return (size_t)(idx & 7u) * p.hit_cap + (idx >> 3);
}

// Sample smp of the pixel at PPM (row pr, column pc): its ray (origin on the
// film, direction towards the eye) exactly as cpu/raytracer.c:55-60 computes
// it; false when the pixel lies outside the framebuffer's even-sized area (its
// ray is still defined).  The one place the camera's arithmetic is written:
// trace_kernel's samples and rt_hip_frame_rays' generator (rt_rays.h) call it.
__device__ __forceinline__ bool camera_ray(const KParams& p, int pr, int pc, int smp, f3& point, f3& dir) {
  // PPM (row, col) -> framebuffer slot (j, i) of cpu/raytracer.c:71,128-134
  const int ii = p.W - pc, jj = p.H - pr;
  const bool valid = pr < p.H && pc < p.W && ii >= 1 && ii <= 2 * (p.W / 2) && jj >= 1 && jj <= 2 * (p.H / 2);
  const int i = ii - p.W / 2, j = jj - p.H / 2;
  // for (float k = i; k < i + 1; k += 0.5) for (float l = j; ...)  (cpu/raytracer.c:55-58)
  const float k = (float)i + 0.5f * (float)(smp >> 1);
  const float l = (float)j + 0.5f * (float)(smp & 1);
  point = add(add(p.C, scale(p.u, k)), scale(p.v, l));
  dir = normalize(sub(p.pos, point));
  return valid;
}

// The camera sample of lane `lane` of item q of rank-local tile t (its pixel
// and sample smp by rt_item_pixel).
__device__ __forceinline__ bool camera_sample(const KParams& p, uint32_t t, uint32_t q, int lane, int& smp,
                                              f3& point, f3& dir) {
  int row, col, pr, pc;
  // (the lane's share of the map does not change from item to item: opaque,
  // or it is hoisted out of trace_kernel's item loop and holds registers
  // across every walk -- 8 B more scratch per lane)
  asm volatile("" : "+v"(lane));
  rt_item_pixel(q, (uint32_t)lane, &row, &col, &smp);
  tile_pixel(p, t, row, col, pr, pc);
  return camera_ray(p, pr, pc, smp, point, dir);
}

// A lane's G-buffer capture record (KParams::capture), as initialised: no
// winner, no record, no query.
struct Capture {
  uint32_t prim = 0xffffffffu;
  uint32_t dist = 0x7f800000u;  // +inf
  uint32_t first = RT_NO_REC;
  uint32_t queries = 0;
};

// One camera sample for every lane of the wave (trace_kernel): the
// recursion as a wave-uniform bounce loop, a hit record appended per hit (one
// atomic per wave and bounce, on the item stream's own counter x).  Returns
// the lane's deepest record (RT_NO_REC: none).  valid = the lane owns a pixel.
// RT_POLICY_GBUFFER and RT_POLICY_RAYS_GB only: cap = the lane's capture record
// (KParams::capture), filled at the first query (depth 0), its query count on
// every bounce.  RT_POLICY_RAYS*: a caller's rays (rt_rays.h) -- the first query
// takes a reflection ray's route too (rays_closest with the batch's `walk`, the
// secondary slack, no candidate lists), and a ray cast ends after it.
template <int ACCEL, bool COUNT, int POL>
__device__ __forceinline__ uint32_t trace_path(const KParams& p, bool valid, f3 o, f3 d,
                                               uint32_t x, Stack& s, WaveCtx& w, WorkCount& wc,
                                               uint32_t tile, Capture& cap, int depth = 0, float coef = 1.0f,
                                               uint32_t prev = RT_NO_REC, uint32_t walk = 0) {
  constexpr bool kRays = POL == RT_POLICY_RAYS || POL == RT_POLICY_RAYS_GB;
  constexpr bool kCapture = POL == RT_POLICY_GBUFFER || POL == RT_POLICY_RAYS_GB;
  // depth: wave-uniform, queries so far on this path
  bool alive = valid;
  for (;;) {
    alive = alive && !((double)coef < 0.01);  // checked before the query
    uint64_t am = __ballot(alive);
    if (am == 0) break;
    wc.closest += (uint32_t)__popcll(am);  // wave-uniform counters (SGPRs)
    if (kCapture && alive) cap.queries++;  // the lane's own share of wc.closest
    Ray r = make_ray(p, o, d, depth == 0 && !kRays ? p.eps_rel_cam : p.eps_rel);
    Best b = best_none();
    uint64_t c0 = COUNT ? __builtin_readcyclecounter() : 0ull;
    if constexpr (kRays)
      rays_closest<ACCEL>(p, r, alive, depth, walk, b, s, w, wc);
    else
      closest_q<ACCEL, COUNT, POL>(p, r, alive, depth, b, s, w, wc);
    if (COUNT) {
      const uint64_t c1 = __builtin_readcyclecounter();
      (depth == 0 ? wc.cy_cam : wc.cy_sec) += (uint32_t)(c1 - c0);
      c0 = c1;
    }
    if (!kRays && ACCEL != RT_ACCEL_FLAT_D && depth == 0) cand_closest<COUNT>(p, r, alive, tile, b, w, wc);
    if (COUNT) wc.cy_cand += (uint32_t)(__builtin_readcyclecounter() - c0);
    bool hit = alive && b.dist != __builtin_inff();
    if (kCapture && depth == 0 && hit) {  // the camera query's winner, a zero-normal one included
      cap.prim = b.prim;
      cap.dist = __float_as_uint(b.dist);
    }
    f3 N = f3{0.0f, 0.0f, 0.0f};
    wc.hits += (uint32_t)__popcll(__ballot(hit));
    bool zero = false;
    if (hit) {
      const float* nm = p.nrm + 9 * (size_t)b.prim;
      float w0 = 1.0f - b.u - b.v;
      N = add(add(scale(ld3(nm), w0), scale(ld3(nm + 3), b.u)), scale(ld3(nm + 6), b.v));
      zero = is_zero(N);  // cpu/hit.c:79 would skip this object; see DESIGN.md
    }
    wc.zero_normal += (uint32_t)__popcll(__ballot(zero));
    hit = hit && !zero;
    const uint64_t hm = __ballot(hit);
    if (hm == 0) break;
    uint32_t base = 0;
    if (w.lane == 0) base = atomicAdd(p.hit_count + RT_HIT_STRIDE * x, (uint32_t)__popcll(hm));
    base = uni(base);
    bool deep = false;
    if (hit) {
      const uint32_t slot = base + (uint32_t)__popcll(hm & ((1ull << w.lane) - 1ull));
      const f3 P = hit_point(r, b.t);  // the winner's hit point, same bits
      if (slot < p.hit_cap) {  // else: counted, and rt_hip_stats reports the overflow
        const size_t a = (size_t)x * p.hit_cap + slot;
        p.hit[2 * a] = make_float4(P.x, P.y, P.z, N.x);
        p.hit[2 * a + 1] = make_float4(N.y, N.z, coef, __uint_as_float(b.obj));
        p.hit_prev[a] = prev;
      }
      prev = x | (slot << 3);
      if (kCapture && depth == 0) cap.first = prev;
      const float ncoef = p.mat[RT_MAT_FLOATS_D * (size_t)b.obj + 10] * coef;  // obj.nr * coef
      if (depth + 1 >= RT_MAX_BOUNCES) {
        deep = !((double)ncoef < 0.01);  // cpu/rt would query again: never silent
      } else {
        d = bounce_dir(d, N);
        o = P;
        coef = ncoef;
      }
    }
    wc.overflow += (uint32_t)__popcll(__ballot(deep));
    alive = hit && depth + 1 < RT_MAX_BOUNCES;
    ++depth;
    if (POL == RT_POLICY_RAYS_GB && (walk & RT_RAYS_WALK_CAST)) break;  // a ray cast: its first query only
  }
  return prev;
}

template <int ACCEL, bool COUNT, int POL>
__global__ __launch_bounds__(64, RT_TRACE_MIN_WAVES) void trace_kernel(KParams p) {
  const int lane = threadIdx.x & 63;
  WorkCount wc = {};
  __shared__ float4 s_stack[ACCEL == RT_ACCEL_FLAT_D ? 1 : kStackArea];
  __shared__ float4 s_stage[ACCEL == RT_ACCEL_FLAT_D ? kStageFlat : kStageOct];
  Stack stk;
  WaveCtx w;
  wave_state(p, s_stack, s_stage, lane, stk, w);
  // Work item = (tile t, quarter q): a tile's 256 camera rays run on four
  // waves, so a tile of long mirror paths (C2: the worst tile cost 7.7x a
  // balanced schedule's whole frame, tools/tile_cost.py) is not one wave's
  // serial critical path.  A wave takes the four samples of a 4x4-pixel
  // quarter (rt_item_pixel, csrc/rt_tiles.h), not one sample of the 8x8
  // tile: the packet walk is wave-serial over the union of its lanes'
  // walks, and a quarter's cone crosses fewer leaves that most of its rays
  // never enter.  Items come in 8 streams, stream x = the
  // tiles t = x (mod 8) in scanline order, 4 items each: workgroup b (on XCD
  // b mod 8, the dispatcher's round robin) pulls from stream b mod 8, so a
  // tile's quarters share one XCD's L2, all XCDs work on the same few tile
  // rows (their geometry stays in the Infinity Cache), and the item counters'
  // atomic traffic is split 8 ways; a drained stream's waves move on to the
  // next.  Each item writes its lanes' deepest hit records.  With camera
  // candidate lists the tiles come longest-first (rt_cand_order): a tile's
  // list length predicts its cost, and the heavy tiles -- the horizon's
  // grazing rays, up to 20x the mean on C5 -- no longer finish the kernel.
  const uint32_t nt = (uint32_t)p.ntiles_local;
  const uint32_t home = (uint32_t)blockIdx.x & 7u;
  uint32_t probe = 0;
  bool first = true;
  unsigned long long wave_cost = 0;  // lane 0: this wave's item clocks (p.item_cost)
  // Items of the heavy tiles (the front of the work order) run at raised
  // wave priority: with 5 waves per SIMD a long mirror path otherwise shares
  // its SIMD's issue slots to the end and becomes the rank's critical path.
  const uint32_t n_heavy = p.n_heavy ? uni(*p.n_heavy) : 0u;
  for (;;) {
    const uint32_t x = (home + probe) & 7u;
    const uint32_t nx = nt > x ? (nt - x + 7u) / 8u : 0u;  // tiles of stream x
    // the first (gridDim.x - x + 7) / 8 items of stream x go one to each of
    // its home waves without an atomic (a small frame's few thousand waves
    // would otherwise queue on 8 counters), the rest through its counter
    uint32_t q = 0;
    if (first) {
      q = (uint32_t)blockIdx.x >> 3;
      first = false;
    } else {
      if (lane == 0) q = atomicAdd(p.tile_counter + 32u * x, 1u);
      q = uni(q) + (gridDim.x - x + 7u) / 8u;
    }
    if (q >= 4u * nx) {
      if (++probe == 8u) break;  // every stream drained: the wave exits
      continue;
    }
    const uint32_t pos = 8u * (q >> 2) + x;  // the tile's place in the work order
    const uint32_t u = 4u * (p.tile_order ? p.tile_order[pos] : pos) + (q & 3u);  // item 4t + quarter
    const bool prio = pos < n_heavy;
    if (prio) __builtin_amdgcn_s_setprio(3);
    const unsigned long long c0 = (COUNT || p.item_cost) ? __builtin_readcyclecounter() : 0ull;
    const uint32_t ph0[3] = {wc.cy_cam, wc.cy_cand, wc.cy_sec};
    wc.sec_lane_nodes = wc.sec_lane_tris = 0;
    const uint32_t t = u >> 2;
    int smp;
    f3 point, dir;
    const bool valid = camera_sample(p, t, u & 3u, lane, smp, point, dir);
    wc.pixels += (uint32_t)__popcll(__ballot(valid && smp == 0));
    Capture cap;
    p.last[(size_t)u * 64 + lane] =
        trace_path<ACCEL, COUNT, POL>(p, valid, point, dir, x, stk, w, wc, t, cap, 0, 1.0f, RT_NO_REC);
    if (POL == RT_POLICY_GBUFFER)  // one 16-byte vector store per lane
      p.capture[(size_t)u * 64 + lane] = make_uint4(cap.prim, cap.dist, cap.first, cap.queries);
    if (prio) __builtin_amdgcn_s_setprio(0);
    if (p.item_cost && lane == 0) {  // the next frame's work order (rt_cand_order)
      const unsigned long long cy = __builtin_readcyclecounter() - c0;
      p.item_cost[u] = cy < 0xffffffffull ? (uint32_t)cy : 0xffffffffu;
      wave_cost += cy;
    }
    if (COUNT && p.tile_cycles && lane == 0) {
      // [0] the item's clocks, [1..3] its phase clocks (camera walk, camera
      // candidates, secondary walks), planes of 4 * ntiles_local items
      const size_t items = 4 * (size_t)p.ntiles_local;
      const uint32_t ph1[3] = {wc.cy_cam, wc.cy_cand, wc.cy_sec};
      p.tile_cycles[u] = __builtin_readcyclecounter() - c0;
#pragma unroll
      for (int k2 = 0; k2 < 3; k2++) p.tile_cycles[u + (size_t)(k2 + 1) * items] = ph1[k2] - ph0[k2];
      p.tile_cycles[u + 4 * items] = wc.sec_lane_nodes;
      p.tile_cycles[u + 5 * items] = wc.sec_lane_tris;
    }
  }
  if (p.cost_sum && lane == 0 && wave_cost) atomicAdd(p.cost_sum, wave_cost);
  flush_counts(p, wc, lane);
}

// Per-lane LDS stack of the shadow walks only (shade_kernel, default
// policy): (first, info) entries, no staged wave stack.
static constexpr int kLaneStackArea = kLdsStack * 64 * 8 / 16;

// apply_light (cpu/light.c:33-100) of hit record a, in two phases per block
// of 32 lights: first the shadow queries (only the hit point is live across
// the walks), then the Phong terms of the unshadowed lights, summed in the
// file order of the lights as the reference does.
// RELIGHT (rt_hip_relight with some lights clean, csrc/rt_relight.h): only the
// lights of p.relight_dirty among 0..31 are queried, the others' bits come
// from the record's stored mask p.hit_lit; lights from index 32 up have no
// stored bit and are always queried.
template <int ACCEL, bool COUNT, int POL, bool RELIGHT = false>
__device__ __forceinline__ col shade_record(const KParams& p, bool valid, size_t a, Stack& s,
                                            WaveCtx& w, WorkCount& wc, uint32_t& lit0) {
  col acc = init_color(0.0f, 0.0f, 0.0f);
  uint32_t pend = 0;  // lights 0..31 whose query was deferred (p.oob)
  for (uint32_t l0 = 0; l0 < p.nlight; l0 += 32) {
    const uint32_t l1 = p.nlight - l0 < 32u ? p.nlight : l0 + 32u;
    uint32_t lit = 0;  // bit k: light l0 + k does not shadow the point
    if constexpr (RELIGHT)
      if (valid && l0 == 0) lit = p.hit_lit[a] & ~p.relight_dirty;  // the clean lights' decisions
    {
      f3 P{0.0f, 0.0f, 0.0f};
      if (valid) {
        const float4 r0 = p.hit[2 * a];
        P = f3{r0.x, r0.y, r0.z};
      }
      for (uint32_t li = l0; li < l1; li++) {
        const LightShade L = LightRowsUniform{p.lshade}[li];
        const uint32_t type = L.type;
        if (type != 1 && type != 2) continue;
        if constexpr (RELIGHT)
          if (l0 == 0 && !((p.relight_dirty >> li) & 1u)) continue;  // clean: no query (wave-uniform)
        const f3 lv = L.v;
        const uint64_t c0 = COUNT ? __builtin_readcyclecounter() : 0ull;
        bool df = false;
        // (issuing the first two lights' cell-range loads before either
        // query, through shadow_q's `pre`, measured slower: shade 1.92 ->
        // 2.16 ms on C5, profiles/r04b_shade_pre/)
        // (df by address, the block-0 condition a flag: a pointer chosen per
        // block kept df on the stack, a scratch store per query)
        // (round 5, with the entries one ahead: the next light's cell ranges
        // loaded while this light's entries are scanned, shade 1.85 -> 1.98
        // ms at 7 waves per SIMD, profiles/r07_shade/)
        const bool sh = shadow_q<ACCEL, COUNT, POL>(p, P, shadow_dir(type, lv, P), type, li, valid, s, w, wc,
                                                    &df, nullptr, l0 == 0);
        if (COUNT) {
          const uint32_t dc = (uint32_t)(__builtin_readcyclecounter() - c0);
          wc.cy_shadow += dc;
          if (type == 1) wc.cy_shadow_dir += dc;
        }
        if (df) pend |= 1u << li;
        if (!sh) lit |= 1u << (li - l0);
      }
    }
    if (l0 == 0) lit0 = lit;
    if (valid && pend && l0 == 0) {  // deferred: queued with the lit bits so far
      const uint32_t q = atomicAdd(p.oob_count, 1u);
      if (q < p.oob_cap) p.oob[q] = make_uint4((uint32_t)a, pend, lit & ~pend, 0u);
    }
    if (!valid) continue;
    const float4 r0 = p.hit[2 * a], r1 = p.hit[2 * a + 1];
    const f3 P{r0.x, r0.y, r0.z}, N{r0.w, r1.x, r1.y};
    const float* ms = p.mshade + RT_MAT_FLOATS_D * (size_t)__float_as_uint(r1.w);
    acc = lights_sum(LightRowsUniform{p.lshade}, acc, l0, l1, lit, ms, P, N);
  }
  return acc;
}

// shade_kernel: hit records in chunks of 64 from RT_HIT_REGIONS streams
// (workgroup b drains region b mod 8, then steals), every lane one record:
// cpu/light.c:33-100 with the shadow queries of cpu/light.c:24-31, then the
// term color_mul(local, coef) of cpu/raytracer.c:30.
template <int ACCEL, bool COUNT, int POL, bool RELIGHT = false>
__global__ __launch_bounds__(64, ACCEL == RT_ACCEL_FLAT_D ? RT_FLAT_SHADE_MIN_WAVES
                                : ((POL == RT_POLICY_STAGED || POL == RT_POLICY_DIR_STAGED) ? RT_STAGED_SHADE_MIN_WAVES
                                                                                              : RT_SHADE_MIN_WAVES)) void shade_kernel(KParams p) {
  const int lane = threadIdx.x & 63;
  WorkCount wc = {};
  constexpr bool kStaged = POL == RT_POLICY_STAGED || POL == RT_POLICY_DIR_STAGED;
  __shared__ float4 s_stack[ACCEL == RT_ACCEL_FLAT_D ? 1 : (kStaged ? kStackArea : kLaneStackArea)];
  __shared__ float4 s_stage[ACCEL == RT_ACCEL_FLAT_D ? kStageFlat : (kStaged ? kStageOct : 1)];
  Stack stk;
  WaveCtx w;
  wave_state(p, s_stack, s_stage, lane, stk, w);
  const uint32_t home = (uint32_t)blockIdx.x & 7u;
  uint32_t probe = 0;
  bool first_chunk = true;
  for (;;) {
    const uint32_t x = (home + probe) & 7u;
    const uint32_t hc = p.hit_count[RT_HIT_STRIDE * x];
    const uint32_t n = hc < p.hit_cap ? hc : p.hit_cap;
    const uint32_t stride = p.shade_stride > 1u ? p.shade_stride : 1u;  // verification only
    const uint32_t first = p.shade_first;
    const uint32_t ns = n > first ? (n - first + stride - 1u) / stride : 0u;  // records shaded
    // first chunk of each home wave without an atomic (as trace_kernel)
    uint32_t q = 0;
    if (first_chunk) {
      q = (uint32_t)blockIdx.x >> 3;
      first_chunk = false;
    } else {
      if (lane == 0) q = atomicAdd(p.shade_counter + RT_HIT_STRIDE * x, 1u);
      q = uni(q) + (gridDim.x - x + 7u) / 8u;
    }
    if (q >= (ns + 63u) / 64u) {
      if (++probe == 8u) break;
      continue;
    }
    const uint32_t k = q * 64u + (uint32_t)lane;
    const bool valid = k < ns;
    const size_t a = (size_t)x * p.hit_cap + (size_t)k * stride + first;
    uint32_t lit = 0;
    const col local = shade_record<ACCEL, COUNT, POL, RELIGHT>(p, valid, a, stk, w, wc, lit);
    if (valid) {
      const col tm = color_mul(local, p.hit[2 * a + 1].z);  // coef
      p.hit_term[a] = make_float4(tm.r, tm.g, tm.b, 0.0f);
      if (p.hit_lit) p.hit_lit[a] = lit;
    }
  }
  flush_counts(p, wc, lane, true);
}

// Exact-shadow mode, deferred queries (shade_kernel, p.oob): entry e's
// pending lights' shadow rays from its record's hit point by brute force over
// the nprim prim-order records (cpu/hit.c:93-109), a workgroup per
// (entry, chunk of kFixChunk records); hits ORed into the entry's w.
static constexpr uint32_t kFixChunk = 16384;
static constexpr uint32_t kFixBatch = 64;  // oob_fix_batch_kernel's queries
// (entry, pending light) queries of the deferred entries, kFixBatch + 1 when
// there are more than oob_fix_batch_kernel holds
__device__ __forceinline__ uint32_t oob_queries(const KParams& p, uint32_t n) {
  if (n > kFixBatch) return kFixBatch + 1;
  uint32_t m = 0;
  for (uint32_t e = 0; e < n; e++) m += (uint32_t)__popc(p.oob[e].y & (p.nlight >= 32 ? 0xffffffffu : (1u << p.nlight) - 1u));
  return m;
}
__global__ __launch_bounds__(256) void oob_fix_kernel(KParams p, uint32_t nprim) {
  __shared__ uint32_t bits, skip, nqs;
  const uint32_t n = min(*p.oob_count, p.oob_cap);
  if (threadIdx.x == 0) nqs = oob_queries(p, n);
  __syncthreads();
  if (nqs <= kFixBatch) return;  // oob_fix_batch_kernel decided them
  const uint32_t chunks = (nprim + kFixChunk - 1) / kFixChunk;
  for (uint64_t item = blockIdx.x; item < (uint64_t)n * chunks; item += gridDim.x) {
    const uint32_t e = (uint32_t)(item / chunks), c = (uint32_t)(item % chunks);
    const uint4 q = p.oob[e];
    if (threadIdx.x == 0) {  // one decision for the block: every lane reaches the barriers
      bits = 0;
      skip = (__atomic_load_n(&p.oob[e].w, __ATOMIC_RELAXED) & q.y) == q.y;  // all already shadowed
    }
    __syncthreads();
    if (skip) {
      __syncthreads();
      continue;
    }
    const float4 r0 = p.hit[2 * (size_t)q.x];
    const f3 P{r0.x, r0.y, r0.z};
    uint32_t mine = 0, risk = 0;
    for (uint32_t li = 0; li < 32 && li < p.nlight; li++) {
      if (!((q.y >> li) & 1u)) continue;
      const LightShade L = LightRowsUniform{p.lshade}[li];  // (li is the workgroup's)
      const Ray r = make_ray(p, P, shadow_dir(L.type, L.v, P), p.eps_rel);
      bool h = false;
      const uint32_t end = min(nprim, (c + 1) * kFixChunk);
      for (uint32_t k = c * kFixChunk + threadIdx.x; k < end && !h; k += blockDim.x) {
        const float4* t = p.tri_prim + 3 * (size_t)k;
        h = any_hit_rec(r, t[0], t[1], t[2], risk);
      }
      if (h) mine |= 1u << li;
    }
    if (mine) atomicOr(&bits, mine);
    if (risk) atomicAdd(p.stats + RT_ST_SHADOW_ZERO_RISK, 1ull);
    __syncthreads();
    if (threadIdx.x == 0 && bits) atomicOr(&p.oob[e].w, bits);
    __syncthreads();
  }
}

// The same decisions for the usual handful of deferred queries (C5: 4
// records, 8 queries per frame) in one pass over the records: every query
// -- (entry, pending light) -- is set up once per workgroup in LDS, and each
// thread streams its records once, testing each against every query.  The
// per-entry launch above reads all nprim records (480 MB on C5) once per
// query: 0.65 ms of HBM traffic for 8 queries.  At most kFixBatch queries.
struct FixQuery {
  Ray r;
  uint32_t e, li;
};
__global__ __launch_bounds__(256) void oob_fix_batch_kernel(KParams p, uint32_t nprim) {
  __shared__ FixQuery qs[kFixBatch];
  __shared__ uint32_t nq;
  const uint32_t n = min(*p.oob_count, p.oob_cap);
  if (threadIdx.x == 0) {
    uint32_t m = 0;
    const bool batch = oob_queries(p, n) <= kFixBatch;
    for (uint32_t e = 0; e < n && batch; e++) {
      const uint4 q = p.oob[e];
      const float4 r0 = p.hit[2 * (size_t)q.x];
      const f3 P{r0.x, r0.y, r0.z};
      for (uint32_t li = 0; li < 32 && li < p.nlight; li++) {
        if (!((q.y >> li) & 1u) || m >= kFixBatch) continue;
        const LightShade L = LightRowsUniform{p.lshade}[li];
        qs[m].r = make_ray(p, P, shadow_dir(L.type, L.v, P), p.eps_rel);
        qs[m].e = e;
        qs[m].li = li;
        m++;
      }
    }
    nq = m;
  }
  __syncthreads();
  const uint32_t m = nq;
  uint32_t risk = 0;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nprim; k += gridDim.x * blockDim.x) {
    const float4* t = p.tri_prim + 3 * (size_t)k;
    const float4 a0 = t[0], a1 = t[1], a2 = t[2];
    for (uint32_t j = 0; j < m; j++) {
      const FixQuery& q = qs[j];
      if (any_hit_rec(q.r, a0, a1, a2, risk)) atomicOr(&p.oob[q.e].w, 1u << q.li);
    }
  }
  if (risk) atomicAdd(p.stats + RT_ST_SHADOW_ZERO_RISK, 1ull);
}

// ... then each entry's record shaded again with the decided lights
// (cpu/light.c:33-100, cpu/raytracer.c:30), as shade_kernel would have.
__global__ __launch_bounds__(64) void oob_reshade_kernel(KParams p) {
  const uint32_t n = min(*p.oob_count, p.oob_cap);
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const uint4 q = p.oob[e];
    const size_t a = q.x;
    const uint32_t lit0 = q.z | (q.y & ~q.w);
    const float4 r0 = p.hit[2 * a], r1 = p.hit[2 * a + 1];
    const f3 P{r0.x, r0.y, r0.z}, N{r0.w, r1.x, r1.y};
    const float* ms = p.mshade + RT_MAT_FLOATS_D * (size_t)__float_as_uint(r1.w);
    const col acc = lights_sum(LightRowsUniform{p.lshade}, init_color(0.0f, 0.0f, 0.0f), 0,
                               p.nlight < 32u ? p.nlight : 32u, lit0, ms, P, N);
    const col tm = color_mul(acc, r1.z);  // coef
    p.hit_term[a] = make_float4(tm.r, tm.g, tm.b, 0.0f);
    if (p.hit_lit) p.hit_lit[a] = lit0;
  }
}

}  // namespace rt

#include "rt_probe.h"  // probe_shadow_kernel, probe_closest_kernel: here in the kernels' order

namespace rt {

// A pixel's four samples (four neighbouring lanes of one trace_kernel item,
// their deepest records one 16-byte load: rt_pixel_slots): each sample's path
// terms summed deepest-first, acc = color_add(reflected, term)
// (cpu/raytracer.c:29-30), then acc = color_add(acc, color_mul(s, 0.25)) over
// the samples (i,j), (i,j+.5), (i+.5,j), (i+.5,j+.5) (cpu/raytracer.c:55-68);
// pixels outside the framebuffer's even-sized area are 0.  One thread per
// pixel of the rank's tile buffer (slot = row * 8 + col).  (Neighbouring
// hit records are now a pixel's samples, so neighbouring threads' chain
// loads are four records apart: fold 0.127 -> 0.143 ms on C5, 0.061 -> 0.097
// on C3, beside shade's 1.84 -> 1.69 from the same order.  One thread per
// (item, lane) with the samples brought together by __shfl read them side by
// side but ran four times the threads: 0.245 and 0.076 ms)
// The frame check's bookkeeping (KParams::frame_check), by one thread of a
// frame's or a ray batch's last launch: every earlier launch has ended (same
// stream).
__device__ __forceinline__ void frame_check_account(const KParams& p) {
  uint32_t f = 0;
  for (int x = 0; x < RT_HIT_REGIONS; x++)
    if (p.hit_count[RT_HIT_STRIDE * x] > p.hit_cap) f |= RT_FRAME_HITBUF;
  unsigned long long s[RT_NSTATS] = {};
  for (int set = 0; set < RT_STAT_SETS; set++)
    for (int k = 0; k < RT_NSTATS; k++) s[k] += p.stats[set * RT_STAT_STRIDE + k];
  auto raised = [&s](uint32_t flag) {  // a slot that raises `flag` is not zero
    bool any = false;
    for (uint32_t k = 0; k < RT_NSTATS; k++) any = any || (rt_stat_frame_flag(k) == flag && s[k]);
    return any;
  };
  if (raised(RT_FRAME_DEPTH)) f |= RT_FRAME_DEPTH;
  if (raised(RT_FRAME_ZERO)) f |= RT_FRAME_ZERO;
  if (raised(RT_FRAME_UNPROVEN) || (p.oob_count && *p.oob_count > p.oob_cap)) f |= RT_FRAME_UNPROVEN;
  if (p.list_flag && *p.list_flag) f |= RT_FRAME_LISTS;
  atomicOr(p.frame_check, (unsigned long long)f);
  atomicAdd(p.frame_check + 1, 1ull);
  atomicAdd(p.frame_check + 2, s[RT_ST_CLOSEST]);
  atomicAdd(p.frame_check + 3, s[RT_ST_SHADOW]);
}

__global__ __launch_bounds__(256) void fold_kernel(KParams p) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx == 0 && p.frame_check) frame_check_account(p);
  if (idx >= (uint32_t)p.ntiles_local * 64u) return;
  const uint32_t t = idx >> 6, lane = idx & 63u;
  int pr, pc;
  const int row = (int)(lane >> 3), col_ = (int)(lane & 7u);
  tile_pixel(p, t, row, col_, pr, pc);
  const int ii = p.W - pc, jj = p.H - pr;
  const bool valid = pr < p.H && pc < p.W && ii >= 1 && ii <= 2 * (p.W / 2) && jj >= 1 &&
                     jj <= 2 * (p.H / 2);
  const uint4 l4 = *(const uint4*)(p.last + rt_pixel_slots(t, row, col_));
  const uint32_t last[4] = {l4.x, l4.y, l4.z, l4.w};
  col acc = init_color(0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int smp = 0; smp < 4; smp++) {
    col sc = init_color(0.0f, 0.0f, 0.0f);
    uint32_t r = last[smp];
    while (r != RT_NO_REC && (r >> 3) < p.hit_cap) {
      const size_t a = rec_addr(p, r);
      const float4 tm = p.hit_term[a];
      sc = color_add(sc, col{tm.x, tm.y, tm.z});
      r = p.hit_prev[a];
    }
    acc = color_add(acc, color_mul(sc, 0.25f));
  }
  if (!valid) acc = col{0.0f, 0.0f, 0.0f};
  float* o = p.out + (size_t)idx * 3;
  o[0] = acc.r;
  o[1] = acc.g;
  o[2] = acc.b;
}

}  // namespace rt

#include "rt_compat.h"  // compat_kernel, downscale_kernel

namespace rt {

// tiles of all ranks (rank-major, as gathered) -> PPM-order image
__global__ __launch_bounds__(256) void assemble_kernel(const float* __restrict__ tiles,
                                                       float* __restrict__ rgb, int W, int H,
                                                       int tiles_x, int ntiles, int nranks,
                                                       int tiles_per_rank) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t npx = (size_t)W * (size_t)H;
  if (idx >= npx) return;
  int row = (int)(idx / (size_t)W), col = (int)(idx % (size_t)W);
  uint32_t rank;
  const int tb = rt_block_side(nranks);
  const uint32_t local = rt_tile_local(col >> 3, row >> 3, (uint32_t)nranks,
                                       (uint32_t)rt_blocks_x(tiles_x, tb), (uint32_t)tb, &rank);
  int lane = ((row & 7) << 3) | (col & 7);
  const float* src = tiles + (((size_t)rank * tiles_per_rank + local) * 64 + lane) * 3;
  rgb[3 * idx + 0] = src[0];
  rgb[3 * idx + 1] = src[1];
  rgb[3 * idx + 2] = src[2];
  (void)ntiles;
}

// The same map for tile buffers of `words` 32-bit words per pixel slot (the
// G-buffer's 4 * RT_GB_WORDS_D): one thread per output word.
__global__ __launch_bounds__(256) void assemble_words_kernel(const uint32_t* __restrict__ tiles,
                                                             uint32_t* __restrict__ out, int W, int H,
                                                             int tiles_x, int nranks, int tiles_per_rank,
                                                             int words) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)W * (size_t)H * (size_t)words) return;
  const size_t px = idx / (size_t)words;
  const int k = (int)(idx % (size_t)words);
  const int row = (int)(px / (size_t)W), col = (int)(px % (size_t)W);
  uint32_t rank;
  const int tb = rt_block_side(nranks);
  const uint32_t local = rt_tile_local(col >> 3, row >> 3, (uint32_t)nranks,
                                       (uint32_t)rt_blocks_x(tiles_x, tb), (uint32_t)tb, &rank);
  const int lane = ((row & 7) << 3) | (col & 7);
  out[idx] = tiles[(((size_t)rank * tiles_per_rank + local) * 64 + lane) * (size_t)words + k];
}

// The public record (include/rt_hip.h rt_gsample: prim obj queries dist P N)
// of capture record `slot` (KParams::capture) and its path's first hit record,
// as five 8-byte stores at `out`; valid = false: a miss without a query.
__device__ __forceinline__ void gsample_store(const KParams& p, bool valid, size_t slot, uint32_t* out) {
  uint32_t prim = 0xffffffffu, obj = 0xffffffffu, queries = 0, dist = 0x7f800000u;
  float4 h0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), h1 = h0;
  if (valid) {
    const uint4 c = p.capture[slot];
    queries = c.w;
    if (c.x != 0xffffffffu) {
      prim = c.x;
      dist = c.y;
      obj = __float_as_uint(p.tri_prim[3 * (size_t)prim + 2].z);
      // no record: a zero-normal winner, or one past the buffer (RT_EHITBUF)
      if (c.z != RT_NO_REC && (c.z >> 3) < p.hit_cap) {
        const size_t a = rec_addr(p, c.z);
        h0 = p.hit[2 * a];
        h1 = p.hit[2 * a + 1];
      }
    }
  }
  uint2* o = (uint2*)out;
  o[0] = make_uint2(prim, obj);
  o[1] = make_uint2(queries, dist);
  o[2] = make_uint2(__float_as_uint(h0.x), __float_as_uint(h0.y));
  o[3] = make_uint2(__float_as_uint(h0.z), __float_as_uint(h0.w));
  o[4] = make_uint2(__float_as_uint(h1.x), __float_as_uint(h1.y));
}

// The G-buffer of a render traced with RT_POLICY_GBUFFER (p = its KParams):
// one thread per (pixel slot, sample) of the rank's tiles turns the sample's
// capture record and its path's first hit record into the public record at
// words [RT_GB_WORDS_D * (4 * slot + sample), ...) of `out` -- consecutive
// threads write consecutive records.  Padding slots and pixels outside the
// framebuffer's even-sized area (fold_kernel's test) are misses without a query.
__global__ __launch_bounds__(256) void gbuffer_kernel(KParams p, uint32_t* __restrict__ out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)p.ntiles_local * 256u) return;
  const uint32_t slot = (uint32_t)(g >> 2), smp = (uint32_t)g & 3u;
  const uint32_t t = slot >> 6, lane = slot & 63u;
  int pr, pc;
  const int row = (int)(lane >> 3), col_ = (int)(lane & 7u);
  tile_pixel(p, t, row, col_, pr, pc);
  const int ii = p.W - pc, jj = p.H - pr;
  const bool valid = pr < p.H && pc < p.W && ii >= 1 && ii <= 2 * (p.W / 2) && jj >= 1 &&
                     jj <= 2 * (p.H / 2);
  gsample_store(p, valid, rt_item_slot(t, row, col_, (int)smp), out + g * RT_GB_WORDS_D);
}

}  // namespace rt

#include "rt_recolour.h"  // relight_zero_kernel, recolour_kernel: after every render kernel
#include "rt_shade_tables.h"  // shade_tables_kernel: after those
#include "rt_rays.h"  // the ray batches' kernels: after those
#include "rt_occl.h"  // the occlusion batches' kernel: after those
#include "rt_ao.h"  // ambient occlusion from records: after those
#include "rt_gather.h"  // traced light gathered from records (ao_ray): after it
#include "rt_dlight.h"  // direct light for records: last

// ---------------------------------------------------------------- launchers
// One instantiation per (kernel, accel, work counting, policy); the default
// policy's kernels have no policy switch inside.  The work-counting pass and
// the test policies are separate kernels, so they cannot slow the default
// ones down.
// The instantiation of (kernel, accel, counting, policy).  Policies only
// differ in the walks they use: trace has no shadow queries (policy 3 =
// default there), shade has no closest-hit queries (policy 1 = default).
template <bool TRACE>
static const void* kernel_of(int accel, int count_work, int policy);

template <bool TRACE>
static const void* kernel_of(int accel, int count_work, int policy) {
  using namespace rt;
  // the capturing trace (no counting variant: the host refuses the pair)
  if (TRACE && policy == RT_POLICY_GBUFFER)
    return accel == RT_ACCEL_FLAT_D ? (const void*)trace_kernel<RT_ACCEL_FLAT_D, false, RT_POLICY_GBUFFER>
                                    : (const void*)trace_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_GBUFFER>;
  if (accel == RT_ACCEL_FLAT_D) {
    if (TRACE)
      return count_work ? (const void*)trace_kernel<RT_ACCEL_FLAT_D, true, 0>
                        : (const void*)trace_kernel<RT_ACCEL_FLAT_D, false, 0>;
    return count_work ? (const void*)shade_kernel<RT_ACCEL_FLAT_D, true, 0>
                      : (const void*)shade_kernel<RT_ACCEL_FLAT_D, false, 0>;
  }
  if (TRACE) {
    if (policy == RT_POLICY_EXACT_REFL)
      return count_work ? (const void*)trace_kernel<RT_ACCEL_OCTREE_D, true, RT_POLICY_EXACT_REFL>
                        : (const void*)trace_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_EXACT_REFL>;
    if (policy == RT_POLICY_LANE) return (const void*)trace_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_LANE>;
    if (policy == RT_POLICY_STAGED)
      return (const void*)trace_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_STAGED>;
    return count_work ? (const void*)trace_kernel<RT_ACCEL_OCTREE_D, true, RT_POLICY_DEFAULT>
                      : (const void*)trace_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_DEFAULT>;
  }
  if (policy == RT_POLICY_STAGED) return (const void*)shade_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_STAGED>;
  if (policy == RT_POLICY_LBUF)
    return count_work ? (const void*)shade_kernel<RT_ACCEL_OCTREE_D, true, RT_POLICY_LBUF>
                      : (const void*)shade_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_LBUF>;
  if (policy == RT_POLICY_DIR_STAGED)
    return (const void*)shade_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_DIR_STAGED>;
  return count_work ? (const void*)shade_kernel<RT_ACCEL_OCTREE_D, true, RT_POLICY_DEFAULT>
                    : (const void*)shade_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_DEFAULT>;
}

// Persistent grid of a kernel: as many one-wave workgroups as the kernel's
// registers and LDS let every CU hold (the occupancy API), so every SIMD is
// filled and no workgroup waits for a slot.
// The ray batches' trace instantiation (rt_rays.h): policy RT_POLICY_RAYS or
// RT_POLICY_RAYS_GB; no counting variant.
static const void* rays_kernel_of(int accel, int policy) {
  using namespace rt;
  if (policy == RT_POLICY_RAYS_GB)
    return accel == RT_ACCEL_FLAT_D ? (const void*)rays_trace_kernel<RT_ACCEL_FLAT_D, RT_POLICY_RAYS_GB>
                                    : (const void*)rays_trace_kernel<RT_ACCEL_OCTREE_D, RT_POLICY_RAYS_GB>;
  return accel == RT_ACCEL_FLAT_D ? (const void*)rays_trace_kernel<RT_ACCEL_FLAT_D, RT_POLICY_RAYS>
                                  : (const void*)rays_trace_kernel<RT_ACCEL_OCTREE_D, RT_POLICY_RAYS>;
}

extern "C" hipError_t rt_render_grid(int trace, int accel, int count_work, int policy, int cus,
                                     int* grid) {
  const bool rays = policy == RT_POLICY_RAYS || policy == RT_POLICY_RAYS_GB;
  const void* k = trace ? (rays ? rays_kernel_of(accel, policy) : kernel_of<true>(accel, count_work, policy))
                        : kernel_of<false>(accel, count_work, policy);
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, 64, 0);
  if (e != hipSuccess) return e;
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 32) per_cu = 32;
  *grid = per_cu * cus;
  return hipSuccess;
}

static hipError_t launch_kernel(const void* k, int grid, const KParams* p, hipStream_t stream) {
  void* args[] = {(void*)p};
  return hipLaunchKernel(k, dim3(grid), dim3(64), args, 0, stream);
}

extern "C" hipError_t rt_launch_trace(const KParams* p, int accel, int count_work, int policy,
                                      int grid, hipStream_t stream) {
  return launch_kernel(kernel_of<true>(accel, count_work, policy), grid, p, stream);
}

extern "C" hipError_t rt_launch_shade(const KParams* p, int accel, int count_work, int policy,
                                      int grid, hipStream_t stream) {
  return launch_kernel(kernel_of<false>(accel, count_work, policy), grid, p, stream);
}

extern "C" hipError_t rt_launch_shade_fixup(const KParams* p, uint32_t nprim, hipStream_t stream) {
  if (!p->oob) return hipGetLastError();
  // the batch pass holds kFixBatch queries; the per-entry pass any number
  // (the count is on the device: both are launched, each a no-op for the
  // other's case)
  hipLaunchKernelGGL(rt::oob_fix_batch_kernel, dim3(2048), dim3(256), 0, stream, *p, nprim);
  hipLaunchKernelGGL(rt::oob_fix_kernel, dim3(4096), dim3(256), 0, stream, *p, nprim);
  hipLaunchKernelGGL(rt::oob_reshade_kernel, dim3(64), dim3(64), 0, stream, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_probe_shadow(const KParams* p, const float* org, uint32_t n, uint32_t li,
                                             uint32_t nprim, int brute, uint32_t* out, hipStream_t stream) {
  if (n == 0) return hipGetLastError();
  hipLaunchKernelGGL(rt::probe_shadow_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *p, org, n, li, nprim,
                     brute, out);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_probe_closest(const KParams* p, const float* org, const float* dir, uint32_t n,
                                              uint32_t nprim, int brute, uint32_t* out, int grid, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t g = (n + 63) / 64;
  if (!brute && g > (uint32_t)grid) return hipErrorInvalidValue;  // the spill area holds `grid` waves
  hipLaunchKernelGGL(rt::probe_closest_kernel, dim3(g), dim3(64), 0, stream, *p, org, dir, n, nprim, brute, out);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_fold(const KParams* p, hipStream_t stream) {
  const uint32_t n = (uint32_t)p->ntiles_local * 64u;
  if (n == 0) return hipGetLastError();
  hipLaunchKernelGGL(rt::fold_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_assemble(const float* tiles, float* rgb, int W, int H, int tiles_x,
                                         int ntiles, int nranks, int tiles_per_rank,
                                         hipStream_t stream) {
  size_t npx = (size_t)W * (size_t)H;
  dim3 g((unsigned)((npx + 255) / 256)), b(256);
  hipLaunchKernelGGL(rt::assemble_kernel, g, b, 0, stream, tiles, rgb, W, H, tiles_x, ntiles,
                     nranks, tiles_per_rank);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_gbuffer(const KParams* p, uint32_t* out, hipStream_t stream) {
  const size_t n = (size_t)p->ntiles_local * 256u;
  if (n == 0) return hipGetLastError();
  hipLaunchKernelGGL(rt::gbuffer_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, *p, out);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_assemble_words(const uint32_t* tiles, uint32_t* out, int W, int H, int tiles_x,
                                               int nranks, int tiles_per_rank, int words,
                                               hipStream_t stream) {
  const size_t n = (size_t)W * (size_t)H * (size_t)words;
  if (n == 0) return hipGetLastError();
  if ((n + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rt::assemble_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tiles,
                     out, W, H, tiles_x, nranks, tiles_per_rank, words);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_compat(const KParams* p, int accel, int grid, hipStream_t stream) {
  dim3 g(grid), b(64);
  if (accel == RT_ACCEL_FLAT_D)
    hipLaunchKernelGGL((rt::compat_kernel<RT_ACCEL_FLAT_D, 0>), g, b, 0, stream, *p);
  else
    hipLaunchKernelGGL((rt::compat_kernel<RT_ACCEL_OCTREE_D, RT_POLICY_DEFAULT>), g, b, 0, stream, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_downscale(const uint32_t* hi, uint32_t* lo, int W, int H,
                                          hipStream_t stream) {
  const int n = W * H;
  hipLaunchKernelGGL(rt::downscale_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, hi, lo, W, H);
  return hipGetLastError();
}

// The relight's launches (rt_kernels.h).  shade_kernel's relight
// instantiations are separate kernels, like the counting and test ones: the
// default shade kernels have no switch for them.  Last in the file, and
// relight_zero_kernel / recolour_kernel templates, so that all of them are
// emitted after every other kernel: the render kernels keep their places in
// the code object.
extern "C" hipError_t rt_launch_relight_zero(const KParams* p, hipStream_t stream) {
  hipLaunchKernelGGL((rt::relight_zero_kernel<0>), dim3(1), dim3(256), 0, stream, *p);
  return hipGetLastError();
}

// A streaming kernel: one 256-lane workgroup per 256 records the buffers can
// hold, at most 8 workgroups per CU, the rest by grid stride.
extern "C" hipError_t rt_launch_recolour(const KParams* p, int cus, hipStream_t stream) {
  const unsigned long long blocks = ((unsigned long long)p->hit_cap * RT_HIT_REGIONS + 255) / 256;
  const unsigned long long most = 8ull * (cus > 0 ? cus : 1);
  hipLaunchKernelGGL((rt::recolour_kernel<0>), dim3((unsigned)(blocks < most ? (blocks ? blocks : 1) : most)), dim3(256), 0,
                     stream, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_reshade(const KParams* p, int accel, int policy, int grid, hipStream_t stream) {
  using namespace rt;
  const void* k = accel == RT_ACCEL_FLAT_D ? (const void*)shade_kernel<RT_ACCEL_FLAT_D, false, 0, true>
                  : policy == RT_POLICY_LBUF
                      ? (const void*)shade_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_LBUF, true>
                      : (const void*)shade_kernel<RT_ACCEL_OCTREE_D, false, RT_POLICY_DEFAULT, true>;
  return launch_kernel(k, grid, p, stream);
}

// The shading tables (rt_shade_tables.h): one thread per light or material row.
extern "C" hipError_t rt_launch_shade_tables(const float* light, uint32_t nlight, float* lshade, const float* mat,
                                             uint32_t nobj, float* mshade, hipStream_t stream) {
  const uint32_t n = nlight > nobj ? nlight : nobj;
  if (!n) return hipSuccess;
  hipLaunchKernelGGL((rt::shade_tables_kernel<0>), dim3((n + 255) / 256), dim3(256), 0, stream, light, nlight, lshade,
                     mat, nobj, mshade);
  return hipGetLastError();
}

// A ray batch's launches (rt_kernels.h, csrc/rt_rays.h).  After the relight's,
// for the same reason: every earlier kernel keeps its place.
extern "C" hipError_t rt_launch_rays_trace(const KParams* p, const RayArgs* a, int accel, int policy, int grid,
                                           hipStream_t stream) {
  if (grid <= 0) return hipErrorInvalidValue;
  void* args[] = {(void*)p, (void*)a};
  return hipLaunchKernel(rays_kernel_of(accel, policy), dim3(grid), dim3(64), args, 0, stream);
}

extern "C" hipError_t rt_launch_rays_fold(const KParams* p, const RayArgs* a, hipStream_t stream) {
  const unsigned long long blocks = a->rgb ? (a->n + 255) / 256 : 1;
  if (blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rt::rays_fold_kernel<0>), dim3((unsigned)blocks), dim3(256), 0, stream, *p, *a);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_rays_samples(const KParams* p, const RayArgs* a, hipStream_t stream) {
  const unsigned long long blocks = (a->n + 255) / 256;
  if (blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rt::rays_sample_kernel<0>), dim3((unsigned)blocks), dim3(256), 0, stream, *p, *a);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_frame_rays(const KParams* p, int order, float* org, float* dir, hipStream_t stream) {
  const unsigned long long blocks = (4ull * (unsigned long long)p->W * (unsigned long long)p->H + 255) / 256;
  if (blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rt::frame_rays_kernel<0>), dim3((unsigned)blocks), dim3(256), 0, stream, *p, order, org, dir);
  return hipGetLastError();
}

// The batches that count into the batch stats block (rt_kernels.h RT_BATCH_*;
// csrc/rt_occl.h, rt_ao.h, rt_dlight.h): one kernel per (kind, accel).  Last, for
// the same reason again.  The kernels are emitted in the order this file first
// names them, so the kinds' lookups stand in the order the kinds were added,
// ambient occlusion's generator between its fused kernel and direct light:
// every kernel keeps its place.
static const void* occl_kernel_of(int accel) {
  return accel == RT_ACCEL_FLAT_D ? (const void*)rt::rays_occl_kernel<RT_ACCEL_FLAT_D>
                                  : (const void*)rt::rays_occl_kernel<RT_ACCEL_OCTREE_D>;
}

static const void* ao_kernel_of(int accel, bool wide) {  // wide: k > 64
  if (accel == RT_ACCEL_FLAT_D)
    return wide ? (const void*)rt::ao_kernel<RT_ACCEL_FLAT_D, true> : (const void*)rt::ao_kernel<RT_ACCEL_FLAT_D, false>;
  return wide ? (const void*)rt::ao_kernel<RT_ACCEL_OCTREE_D, true> : (const void*)rt::ao_kernel<RT_ACCEL_OCTREE_D, false>;
}

// Ambient occlusion's generator alone (csrc/rt_ao.h), one thread per ray.
extern "C" hipError_t rt_launch_ao_rays(const AoArgs* a, hipStream_t stream) {
  const unsigned long long blocks = (a->n * a->k + 255) / 256;
  if (blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rt::ao_rays_kernel<0>), dim3((unsigned)blocks), dim3(256), 0, stream, *a);
  return hipGetLastError();
}

static const void* dlight_kernel_of(int accel) {
  return accel == RT_ACCEL_FLAT_D ? (const void*)rt::dlight_kernel<RT_ACCEL_FLAT_D>
                                  : (const void*)rt::dlight_kernel<RT_ACCEL_OCTREE_D>;
}

static const void* batch_kernel_of(int kind, int accel) {
  if (kind == RT_BATCH_OCCL) return occl_kernel_of(accel);
  if (kind == RT_BATCH_DLIGHT) return dlight_kernel_of(accel);
  return ao_kernel_of(accel, kind == RT_BATCH_AO_WIDE);
}

// Its persistent grid, as rt_render_grid's.
extern "C" hipError_t rt_batch_grid(int kind, int accel, int cus, int* grid) {
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, batch_kernel_of(kind, accel), 64, 0);
  if (e != hipSuccess) return e;
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 32) per_cu = 32;
  *grid = per_cu * cus;
  return hipSuccess;
}

// args: the kind's own block (OcclArgs, AoArgs, DlArgs)
extern "C" hipError_t rt_launch_batch(const KParams* p, const void* args, int kind, int accel, int grid,
                                      hipStream_t stream) {
  if (grid <= 0) return hipErrorInvalidValue;
  void* kargs[] = {(void*)p, (void*)args};
  return hipLaunchKernel(batch_kernel_of(kind, accel), dim3(grid), dim3(64), kargs, 0, stream);
}

// A gather's launches (rt_kernels.h, csrc/rt_gather.h): the ray batches' policy,
// k <= 64 and k > 64 two kernels.  Last, for the same reason once more: named
// here first, its kernels are emitted after every kernel that existed.
static const void* gather_kernel_of(int accel, bool wide) {  // wide: k > 64
  using namespace rt;
  if (accel == RT_ACCEL_FLAT_D)
    return wide ? (const void*)gather_trace_kernel<RT_ACCEL_FLAT_D, RT_POLICY_RAYS, true>
                : (const void*)gather_trace_kernel<RT_ACCEL_FLAT_D, RT_POLICY_RAYS, false>;
  return wide ? (const void*)gather_trace_kernel<RT_ACCEL_OCTREE_D, RT_POLICY_RAYS, true>
              : (const void*)gather_trace_kernel<RT_ACCEL_OCTREE_D, RT_POLICY_RAYS, false>;
}

// Its persistent grid, as rt_render_grid's.
extern "C" hipError_t rt_gather_grid(int accel, int wide, int cus, int* grid) {
  int per_cu = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gather_kernel_of(accel, wide != 0), 64, 0);
  if (e != hipSuccess) return e;
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 32) per_cu = 32;
  *grid = per_cu * cus;
  return hipSuccess;
}

extern "C" hipError_t rt_launch_gather_trace(const KParams* p, const GatherArgs* a, int accel, int grid,
                                             hipStream_t stream) {
  if (grid <= 0) return hipErrorInvalidValue;
  void* args[] = {(void*)p, (void*)a};
  return hipLaunchKernel(gather_kernel_of(accel, a->ao.k > 64u), dim3(grid), dim3(64), args, 0, stream);
}

extern "C" hipError_t rt_launch_gather_fold(const KParams* p, const GatherArgs* a, hipStream_t stream) {
  const unsigned long long blocks = (a->ao.n + 255) / 256;
  if (blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL((rt::gather_fold_kernel<0>), dim3((unsigned)blocks), dim3(256), 0, stream, *p, *a);
  return hipGetLastError();
}
