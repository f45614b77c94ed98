// rt_kernels.h -- parameter block shared by the render kernels and their
// host-side launcher (rt_hip.cpp).  Not part of the public C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_counters.h"
#include "rt_device.h"
#include "rt_lightbuf.h"

#define RT_ACCEL_FLAT_D 0
#define RT_ACCEL_OCTREE_D 1
#define RT_MAT_FLOATS_D 12
#define RT_LIGHT_FLOATS_D 8
// one row of the light shading table (KParams::lshade, csrc/rt_shade_rows.h):
// four float4, so a wave-uniform row is one 64-byte scalar load
#define RT_LSHADE_FLOATS_D 16
// closest-hit queries one path may make before the render reports RT_EDEPTH:
// cpu/rt recurses while coef >= 0.01 (cpu/raytracer.c:19-34), which is
// unbounded for mirrors of Nr >= 1; paths of Nr < 1 end long before this
#define RT_MAX_BOUNCES 16384
// per-lane global overflow area of the traversal stack (entries beyond LDS)
#define RT_SPILL_STACK 112
// hit records (the wavefront split, rt_render.hip): 8 regions, one per
// item stream, each with its own append counter; a record index is
// region | (slot << 3), RT_NO_REC = none.  The regions' counters (hit_count,
// shade_counter) lie RT_HIT_STRIDE words apart, each in its own cache line
#define RT_HIT_REGIONS 8
#define RT_HIT_STRIDE 32
#define RT_NO_REC 0xffffffffu
// occupancy target of the render kernels' launch bounds (waves per SIMD).
// The kernels need 123 VGPRs and 9.7 KB of LDS, so they still run 4 waves
// per SIMD; a target of 3 only changes the scheduler's trade-offs (measured,
// C5 render kernel: 13.86 ms at 4, 13.70 at 3 and at 2; profiles/r02m_waves/).
#ifndef RT_MIN_WAVES
#define RT_MIN_WAVES 3
#endif
// occupancy targets of the wavefront split's kernels (waves per SIMD):
// trace_kernel (closest-hit walks, candidate tests) needs 104 registers left
// alone, 96 at 5 waves (C5 trace 7.35 -> 6.34 ms, profiles/r03d/); shade_kernel
// (shadow queries + Phong per hit record) fits 64 at 8 (7.19 -> 6.89 ms).
// Re-measured with light buffers (profiles/r04c_validate/ab.log, C5): shade
// 1.92 ms at 8, 1.99 at 7, 2.01 at 6; trace 6.22 ms at 5, 7.12 at 4
#ifndef RT_TRACE_MIN_WAVES
#define RT_TRACE_MIN_WAVES 5
#endif
#ifndef RT_SHADE_MIN_WAVES
#define RT_SHADE_MIN_WAVES 7  // 72 VGPRs: the light-buffer scan's record one ahead (rt_query.h lbuf_scan)
#endif
// the staged test policies' shade kernels (packet any-hit walks, test / A/B
// only) need more registers than 8 waves allow: their own, reachable, target
#ifndef RT_STAGED_SHADE_MIN_WAVES
#define RT_STAGED_SHADE_MIN_WAVES 4
#endif
// the brute-force (FLAT) shade kernel streams records through LDS, two at a
// time (mt_candidate2): at 8 waves it spilled 96 B per lane
#ifndef RT_FLAT_SHADE_MIN_WAVES
#define RT_FLAT_SHADE_MIN_WAVES 5
#endif
// triangle record flag (q2.w bits, host/accel.c rt_flatten): the record's
// object has a triangle whose interpolated normal can be exactly zero, so
// cpu/hit.c:99 may skip the object in collide_dist (early any-hit exit is
// then not known to be exact)
#define RT_REC_ZERO_RISK 1u
// traversal policies (one kernel instantiation each, rt_render.hip); the
// others exist for tests and A/B measurements
#define RT_POLICY_DEFAULT 0     // staged packet closest hit for coherent queries, per-lane shadows
#define RT_POLICY_LANE 1        // every octree query per lane
#define RT_POLICY_STAGED 2      // every octree query as a staged packet
#define RT_POLICY_DIR_STAGED 3  // default + staged packet directional-light shadows
// shade kernel only, chosen by the host (never by rt_hip_set_policy): the
// default policy when every directional / point light has a light buffer --
// the shadow queries compile to the buffer scan alone, without the octree
// walk's registers and code (the default's fallback for lights without one)
#define RT_POLICY_LBUF 4
// trace kernel only, chosen by the host (rt_hip_set_exact_reflections with
// the default policy): the default plus reflection rays through the proven
// walk (csrc/rt_reflect.hip: per-node error-region growth)
#define RT_POLICY_EXACT_REFL 5
// trace kernel only, chosen by the host (rt_hip_set_gbuffer with the default
// policy, octree or FLAT): the default plus one capture record per camera
// sample (KParams::capture) -- the default kernel has no register to spare
// for it, so it has no switch either
#define RT_POLICY_GBUFFER 6
// ray-batch trace kernels only (rt_hip_trace_rays, csrc/rt_rays.h), chosen by
// the host: every query of a path, the first included, takes the route of a
// reflection ray -- no camera candidate lists, the secondary rays' slack, the
// walk the batch names (RayArgs::walk).  RAYS_GB also fills a capture record
// per ray (KParams::capture) and can stop after the first query (a ray cast)
#define RT_POLICY_RAYS 7
#define RT_POLICY_RAYS_GB 8
#define RT_NPOLICIES 9
// words of one public G-buffer sample record (include/rt_hip.h rt_gsample)
#define RT_GB_WORDS_D 10

// wave-total counters (wave-uniform, so they live in SGPRs; 32-bit per wave,
// widened to 64-bit by the final atomics)
struct WorkCount {
  uint32_t closest, shadow, pixels, nodes, tris, overflow, zero_normal, hits;
  // per-lane node visits / triangle tests of closest-hit and shadow queries
  // (COUNT pass): a record tested by k lanes counts k times
  uint32_t cl_nodes, cl_tris, sh_nodes, sh_tris;
  // COUNT pass: shader clocks a wave spent in the camera-ray walk, the
  // camera candidate tests, the secondary closest-hit walks and the shadow
  // queries (wall clock of the wave, so shares of its time)
  uint32_t cy_cam, cy_cand, cy_sec, cy_shadow;
  uint32_t cy_shadow_dir;  // the directional-light part of cy_shadow
  uint32_t stack_spills;   // per-lane stack pushes past the LDS entries (COUNT pass)
  uint32_t zero_risk;      // shadow hits on objects whose interpolated normal can vanish
  uint32_t sh_unproven;    // point-light shadow rays from beyond the proof's assumed extent
  uint32_t cl_unproven;    // exact reflection walk: queries with |d| past RT_RF_DLMAX
  // COUNT pass, per work item (rt_hip_tile_phase_cycles phases 4, 5): the
  // most node visits / triangle tests one lane made in per-lane secondary walks
  uint32_t sec_lane_nodes, sec_lane_tris;
};

struct KParams {
  const float4* tri;    // triangle records, 3 float4 each (host/rt_internal.h)
  const float* nrm;     // 9 floats per prim
  const float* mat;     // RT_MAT_FLOATS_D per object
  const float* light;   // RT_LIGHT_FLOATS_D per light
  const float4* node;   // 2 float4 per octree node (NULL for FLAT)
  uint32_t nrec, nlight;
  rt::f3 u, v, C, pos;  // camera frame (cpu/raytracer.c:82-86)
  int W, H;
  int tiles_x, ntiles_total, rank, nranks, ntiles_local;
  float* out;                   // rank's tile buffer (written by fold_kernel)
  // wavefront split (rt_render.hip): trace_kernel appends one hit record per
  // closest hit, shade_kernel turns each into its reflection term, fold_kernel
  // sums every path's terms deepest-first and a pixel's four samples
  float4* hit;                  // RT_HIT_REGIONS x hit_cap records: P.xyz N.x | N.yz coef obj
  uint32_t* hit_prev;           // per record: the path's previous record (RT_NO_REC)
  float4* hit_term;             // per record: color_mul(apply_light(...), coef), rgb
  uint32_t* hit_count;          // RT_HIT_REGIONS append counters, RT_HIT_STRIDE words apart
  uint32_t hit_cap;             // records per region
  uint32_t* last;               // per (item, lane), rt_tiles.h rt_item_slot: the path's deepest record (RT_NO_REC)
  uint32_t* shade_counter;      // RT_HIT_REGIONS chunk counters of shade_kernel, RT_HIT_STRIDE apart
  // shadow verification (rt_hip_verify_shadows; NULL / 0 in renders): the
  // shade pass writes each shaded record's unshadowed-light mask (lights
  // 0..31) and shades only every shade_stride-th record of each region
  uint32_t* hit_lit;
  uint32_t shade_stride;
  uint32_t shade_first;  // ... starting with the shade_first-th
  // exact shadow rays (csrc/rt_shadow.hip): per-node (mu, nu) multipliers of
  // the shadow walk's slack, and the prims every unshadowed shadow ray tests
  // light buffers (csrc/rt_lightbuf.hip), per light; NULL: every shadow query walks
  const RtLightBuf* lbuf;
  const float2* node_mu;
  // exact reflection rays (csrc/rt_reflect.hip, policy RT_POLICY_EXACT_REFL
  // and the closest-hit probe): 3 float4 of error-region bounds per node
  const float4* node_rf;
  const uint32_t* sh_global;
  uint32_t n_sh_global;
  float sh_omax;  // point-light shadow origins with |o - c|_max beyond this are counted unproven
  // exact-shadow mode (proven light buffers): shadow queries of lights 0..31
  // from origins off the proof box are deferred -- shade_kernel appends
  // (record, pending lights, lit lights, 0) and shades with them lit;
  // rt_launch_shade_fixup decides them by brute force and re-shades the record
  uint4* oob;
  uint32_t* oob_count;
  uint32_t oob_cap;
  uint32_t* tile_counter;       // 8 item-stream counters, 32 words apart; zeroed before launch
  unsigned long long* stats;    // RT_NSTATS counters (rt_counters.h RtStat), zeroed before launch
  uint2* spill;                 // grid*64 lanes x RT_SPILL_STACK stack entries
  rt::f3 scene_c;               // scene box centre
  float scene_cmag;             // max-norm of scene_c
  float scene_r;                // scene box half-extent (max-norm)
  float eps_rel;                // culling slack, rt_cull.h rt_cull_eps()
  float eps_rel_cam;            // the same for camera rays (bounce depth 0)
  unsigned long long* tile_cycles;  // COUNT pass: shader clocks of each work item (tile, quarter) (NULL: none)
  // camera-ray candidate lists (built by csrc/rt_cand.hip, ordered by rt_cand_entries.h); cand_start == NULL: none
  const uint32_t* cand_start;   // ntiles_local + 1 offsets into cand
  const uint32_t* cand;         // prims
  const uint32_t* cand_global;  // prims every camera ray tests
  uint32_t n_cand_global;
  const uint32_t* n_cand_global_dev;  // their count on the device (an asynchronous list build), or NULL
  const float4* tri_prim;       // prim-order triangle records
  const float* cand_skip;       // per cand entry: lower bound of new_dist - |pos - o| (depth skip)
  const uint32_t* tile_order;   // trace_kernel's work order: position -> rank-local tile (NULL: identity)
  // the trace's per-item cost (shader clocks of each (tile, quarter) item,
  // saturated to 32 bits) and their sum (zeroed before launch), for the next
  // frame's work order (rt_cand_order); NULL: not recorded
  uint32_t* item_cost;
  unsigned long long* cost_sum;
  // the heavy tiles at the front of tile_order (rt_cand_order's count, on
  // the device; NULL: none): their items run at raised wave priority
  const uint32_t* n_heavy;
  // per-frame completeness check (fold_kernel, the frame's last launch): the
  // conditions rt_hip_stats reports as errors, ORed into frame_check[0]
  // (RT_FRAME_*), frame_check[1] += 1 frame, [2] / [3] += its closest-hit /
  // shadow queries -- sticky across frames until rt_hip_frame_check reads
  // them, so a timed loop of many frames is checked and counted as a whole.
  // list_flag: the frame's asynchronous list build's overflow flag (the
  // snapshot's RT_CC_OVERFLOW), or NULL
  unsigned long long* frame_check;
  const uint32_t* list_flag;
  // G-buffer capture (RT_POLICY_GBUFFER; NULL otherwise), per (item, lane) like
  // `last`: the camera query's winner prim (~0: none) | bits of its new_dist |
  // the path's first hit record (RT_NO_REC: none) | the path's closest-hit
  // queries.  Appended: every other kernel's argument offsets stay put
  uint4* capture;
  // relight (rt_hip_relight, shade_kernel's relight instantiation only): the
  // lights 0..31 whose shadow queries run; the others' outcomes are the bits
  // of the record's stored mask hit_lit (csrc/rt_relight.h).  Appended too
  uint32_t relight_dirty;
  // shading tables (csrc/rt_shade_rows.h), derived on the device from mat and
  // light wherever those are uploaded: the constants of a material
  // (RT_MAT_FLOATS_D per object, as mat) and of a light (RT_LSHADE_FLOATS_D per
  // light) that the shade pass would otherwise compute again per record.  The
  // trace, the probes and the compatibility mode read mat and light.  Appended
  const float* mshade;
  const float* lshade;
};
// (the bits of frame_check[0], RT_FRAME_*: rt_counters.h)

// What a ray batch's kernels take beside the KParams (csrc/rt_rays.h): its own
// small block, so KParams -- passed by value to every kernel -- stays as it is.
#define RT_RAYS_WALK_PACKET 1u  // the first query of each work item as one staged packet
#define RT_RAYS_WALK_EXACT 2u   // every query through the proven reflection walk (KParams::node_rf)
#define RT_RAYS_WALK_CAST 4u    // stop after the first query (RT_POLICY_RAYS_GB)
struct RayArgs {
  const float* org;      // 3 floats per ray
  const float* dir;      // 3 floats per ray, used as given
  unsigned long long n;  // rays
  uint32_t nitems;       // rt_ray_item_count(n)
  uint32_t walk;         // RT_RAYS_WALK_*
  float* rgb;            // 3 floats per ray (NULL: a ray cast)
  uint32_t* samples;     // RT_GB_WORDS_D words per ray (NULL: none)
};

// What an occlusion batch's kernel takes beside the KParams (csrc/rt_occl.h).
// walk: RT_RAYS_WALK_PACKET (every aligned 64 rays as one packet) or
// RT_RAYS_WALK_EXACT (the proven closest walk), else the per-lane bounded walk.
struct OcclArgs {
  const float* org;      // 3 floats per ray
  const float* dir;      // 3 floats per ray, used as given
  const float* tmax;     // one per ray, world distance (NULL: +inf for every ray)
  unsigned long long n;  // rays
  uint32_t nitems;       // rt_ray_item_count(n)
  uint32_t walk;         // RT_RAYS_WALK_*
  unsigned char* out;    // one byte per ray
};

// What the ambient-occlusion kernels take beside the KParams (csrc/rt_ao.h):
// records in, the ray rule's inputs (csrc/rt_ao_items.h), one count per record
// out.  ao_rays_kernel reads the first block only and writes org, dir, shot.
struct AoArgs {
  const uint2* samples;     // n rt_gsample records as five 8-byte pairs each
  unsigned long long n;     // samples
  unsigned long long base;  // index offset of sample 0 (the hash's 64-bit g = base + i)
  const float* table;       // m local directions, 3 floats each
  uint32_t k, m, seed;      // rays per sample, table rows, hash seed
  uint32_t spi;             // rt_ao_spi(k): samples of a work item
  uint32_t kinv;            // rt_ao_kinv(k): a lane's sample without a division
  uint32_t nitems;          // rt_ao_item_count(n, k)
  uint32_t walk;            // RT_RAYS_WALK_*, as OcclArgs::walk
  float tmax;               // the batch's one distance bound (+inf: none)
  uint32_t* out;            // one count per sample
  float* org;               // ao_rays_kernel: 3 floats per ray
  float* dir;               // ao_rays_kernel: 3 floats per ray
  unsigned char* shot;      // ao_rays_kernel: one byte per sample, or NULL
};

// What the direct-light kernel takes beside the KParams (csrc/rt_dlight.h):
// records in, three colour words and (optionally) one mask word per record out.
struct DlArgs {
  const uint2* samples;  // n rt_gsample records as five 8-byte pairs each
  unsigned long long n;  // records
  uint32_t nitems;       // rt_ray_item_count(n)
  uint32_t walk;         // RT_RAYS_WALK_*, as OcclArgs::walk: the walk off a light buffer's proof box
  uint32_t nobj;         // objects of the context: rows of KParams::mshade
  float* rgb;            // 3 floats per record
  uint32_t* lit;         // one word per record, or NULL
};

// What a gather's kernels take beside the KParams (csrc/rt_gather.h): ambient
// occlusion's block for the records and the ray rule (out, tmax, org, dir and
// shot unused; nitems = rt_gather_item_count, walk as RayArgs::walk without
// the cast) and the sums out.
struct GatherArgs {
  AoArgs ao;
  float* rgb;  // 3 floats per record
};

// The three launches of one render (policy = RT_POLICY_*, octree only):
// trace (closest hits -> hit records), shade (shadow queries + Phong per
// record -> terms), fold (terms -> the rank's tile buffer)
extern "C" hipError_t rt_launch_trace(const KParams* p, int accel, int count_work, int policy,
                                      int grid, hipStream_t stream);
extern "C" hipError_t rt_launch_shade(const KParams* p, int accel, int count_work, int policy,
                                      int grid, hipStream_t stream);
// exact-shadow mode: the deferred queries of shade_kernel (p->oob), brute
// force over the nprim prim-order records, then their records re-shaded
extern "C" hipError_t rt_launch_shade_fixup(const KParams* p, uint32_t nprim, hipStream_t stream);
extern "C" hipError_t rt_launch_fold(const KParams* p, hipStream_t stream);
// relight (csrc/rt_recolour.h): the kept records of the last render shaded
// again.  rt_launch_relight_zero zeroes what a shade pass adds to -- the shade
// chunk counters, the shadow-side stat slots, the off-box queue's count --
// and leaves the trace's counters; rt_launch_recolour sums every record's
// lights from its stored mask p->hit_lit (no shadow query); rt_launch_reshade
// is shade_kernel querying only the lights of p->relight_dirty (default
// policy, RT_POLICY_LBUF or FLAT; no counting variant)
extern "C" hipError_t rt_launch_relight_zero(const KParams* p, hipStream_t stream);
extern "C" hipError_t rt_launch_recolour(const KParams* p, int cus, hipStream_t stream);
extern "C" hipError_t rt_launch_reshade(const KParams* p, int accel, int policy, int grid, hipStream_t stream);
// The shading tables of `nlight` light rows and `nobj` material rows (either
// count may be 0: that table is left alone)
extern "C" hipError_t rt_launch_shade_tables(const float* light, uint32_t nlight, float* lshade, const float* mat,
                                             uint32_t nobj, float* mshade, hipStream_t stream);
// shadow-query probe: light li's shadow ray from each of n origins through
// the light buffer p->lbuf[li] (brute = 0) or brute force over nprim
// prim-order records p->tri_prim (brute = 1); out[i] = shadowed
extern "C" hipError_t rt_launch_probe_shadow(const KParams* p, const float* org, uint32_t n, uint32_t li,
                                             uint32_t nprim, int brute, uint32_t* out, hipStream_t stream);
// closest-hit probe: ray i = (org[i], dir[i]) through the per-lane walk of a
// reflection ray (brute = 0) or brute force over nprim prim-order records
// (brute = 1); out[2 i] = winner prim (~0: none), out[2 i + 1] = new_dist bits.
// The walk's spill area p->spill holds `grid` waves: n <= 64 grid.
extern "C" hipError_t rt_launch_probe_closest(const KParams* p, const float* org, const float* dir, uint32_t n,
                                              uint32_t nprim, int brute, uint32_t* out, int grid, hipStream_t stream);
// A ray batch (csrc/rt_rays.h): its trace (policy = RT_POLICY_RAYS or
// RT_POLICY_RAYS_GB, one-wave workgroups pulling items of 64 rays), the fold of
// every ray's path into a->rgb with the frame check's bookkeeping (a->rgb NULL:
// the bookkeeping alone), and the capture records turned into a->samples
extern "C" hipError_t rt_launch_rays_trace(const KParams* p, const RayArgs* a, int accel, int policy, int grid,
                                           hipStream_t stream);
extern "C" hipError_t rt_launch_rays_fold(const KParams* p, const RayArgs* a, hipStream_t stream);
extern "C" hipError_t rt_launch_rays_samples(const KParams* p, const RayArgs* a, hipStream_t stream);
// rt_hip_frame_rays: the 4 W H camera rays of p's frame (p->u, v, C, pos, W, H)
// in pixel order (order 0) or quarter order (1), csrc/rt_ray_items.h
extern "C" hipError_t rt_launch_frame_rays(const KParams* p, int order, float* org, float* dir, hipStream_t stream);
// The batches that count into the batch stats block (csrc/rt_batch.h): an
// occlusion batch (csrc/rt_occl.h, args = OcclArgs), ambient occlusion from
// records (csrc/rt_ao.h, AoArgs; k <= 64 and k > 64 are two kernels) and direct
// light for records (csrc/rt_dlight.h, DlArgs).  Each kind is one kernel on
// one-wave workgroups pulling work items; rt_batch_grid is that kernel's
// persistent grid on `cus` CUs, rt_launch_batch its launch with `args`, the
// kind's own block.
#define RT_BATCH_OCCL 0
#define RT_BATCH_AO 1
#define RT_BATCH_AO_WIDE 2
#define RT_BATCH_DLIGHT 3
#define RT_NBATCH 4
extern "C" hipError_t rt_launch_batch(const KParams* p, const void* args, int kind, int accel, int grid,
                                      hipStream_t stream);
extern "C" hipError_t rt_batch_grid(int kind, int accel, int cus, int* grid);
// ambient occlusion's generator alone, one thread per ray
extern "C" hipError_t rt_launch_ao_rays(const AoArgs* a, hipStream_t stream);
// A gather (csrc/rt_gather.h): its trace (the ray batches' policy
// RT_POLICY_RAYS, one-wave workgroups pulling items of whole records; k <= 64
// and k > 64 are two kernels), that kernel's persistent grid on `cus` CUs, and
// the fold of every record's k paths into a->rgb with the frame check's
// bookkeeping.  The shade pass between them is rt_launch_shade and
// rt_launch_shade_fixup, as in a ray batch
extern "C" hipError_t rt_launch_gather_trace(const KParams* p, const GatherArgs* a, int accel, int grid,
                                             hipStream_t stream);
extern "C" hipError_t rt_gather_grid(int accel, int wide, int cus, int* grid);
extern "C" hipError_t rt_launch_gather_fold(const KParams* p, const GatherArgs* a, hipStream_t stream);
// The path export (rt_hip_path_records, csrc/rt_paths.hip, a translation unit
// of its own): the kept batch's hit-record buffers in, the caller's arrays
// out.  Three launches on 256-ray blocks (csrc/rt_path_items.h), none waiting
// for another workgroup: every ray's chain length into offsets[i] and every
// block's total into btot; one workgroup scanning btot in place and writing
// offsets[n]; the block-local scan that turns the lengths into offsets, and
// each chain walked again and stored first hit first below cap.
struct PathArgs {
  const float4* hit;         // the batch's KParams::hit, hit_prev, hit_term, last, hit_cap
  const uint32_t* hit_prev;
  const float4* hit_term;
  const uint32_t* last;
  uint32_t hit_cap;
  uint32_t nblocks;          // rt_path_blocks(n)
  unsigned long long n;      // rays
  unsigned long long cap;    // vertices the output arrays hold
  uint32_t* offsets;         // n + 1 words
  uint32_t* btot;            // rt_path_scratch_words(n): block totals, then block bases
  uint2* records;            // five 8-byte pairs per vertex (rt_gsample), or NULL
  float* coef;               // one per vertex, or NULL
  float* terms;              // three per vertex, or NULL
};
extern "C" hipError_t rt_launch_path_lengths(const PathArgs* a, hipStream_t stream);
extern "C" hipError_t rt_launch_path_totals(const PathArgs* a, hipStream_t stream);
extern "C" hipError_t rt_launch_path_write(const PathArgs* a, hipStream_t stream);
// persistent grid (one-wave workgroups) of trace (trace = 1) or shade on `cus` CUs
extern "C" hipError_t rt_render_grid(int trace, int accel, int count_work, int policy, int cus,
                                     int* grid);
// gpu/rt compatibility mode: p->W x p->H = the 3x upscaled frame, p->out =
// its packed RGBA8 image; then the 3x3 downscale to W x H (PNG row order)
extern "C" hipError_t rt_launch_compat(const KParams* p, int accel, int grid, hipStream_t stream);
extern "C" hipError_t rt_launch_downscale(const uint32_t* hi, uint32_t* lo, int W, int H,
                                          hipStream_t stream);
extern "C" hipError_t rt_launch_assemble(const float* tiles, float* rgb, int W, int H, int tiles_x,
                                         int ntiles, int nranks, int tiles_per_rank,
                                         hipStream_t stream);
// G-buffer of the last render with p->capture set (its KParams): the rank's
// tile buffer of 4 * RT_GB_WORDS_D words per pixel slot, one thread per
// (pixel, sample)
extern "C" hipError_t rt_launch_gbuffer(const KParams* p, uint32_t* out, hipStream_t stream);
// rt_launch_assemble for tile buffers of `words` 32-bit words per pixel slot
extern "C" hipError_t rt_launch_assemble_words(const uint32_t* tiles, uint32_t* out, int W, int H, int tiles_x,
                                               int nranks, int tiles_per_rank, int words,
                                               hipStream_t stream);
