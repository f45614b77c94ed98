/*
 * rt_hip.h -- C ABI of the MI355X (gfx950) render path.
 *
 * Plain pointers and sizes only.  This is the drop-in boundary for the
 * reference's hot path:
 *
 *   rt_raytrace()        replaces  void raytrace(const char *input, const char *output)
 *                                  (/root/reference/cpu/headers/raytracer.h:4,
 *                                   cpu/raytracer.c:79-136)
 *   rt_hip_create()      replaces  struct scene *to_cuda(const struct scene *)
 *                                  (/root/reference/gpu/headers/scene.h:52, gpu/scene.cu:224-352)
 *                                  + create_octree() (gpu/partitioning/octree.h:39, octree.cu:362-411)
 *   rt_hip_render()      replaces  render(...) (gpu/headers/raytracer.h:6, gpu/raytracer.cu:177-253)
 *                                  with cpu/rt semantics: 2x2 SSAA in cpu order, float
 *                                  channels, unbounded-by-design reflection recursion
 *                                  (cpu/raytracer.c:19-77), collide/collide_dist/apply_light
 *                                  (cpu/hit.c:72-109, cpu/light.c:33-100) on the device
 *   rt_hip_assemble()    (new)     tile buffers of all ranks -> PPM-order float image
 *   rt_hip_gbuffer()     (new)     opt-in per-sample passes of the last render: winning
 *                                  triangle, object, queries, depth, hit point, normal
 *   rt_hip_trace_rays()  (new)     trace(ray, 1.0) of cpu/raytracer.c:19-34 for a batch of the
 *                                  caller's rays: a colour and a hit record per ray
 *   rt_raytrace_multi()  (new)     in-process 1..8 GPU render + RCCL gather over xGMI
 *
 * Test, tuning and measurement hooks (probes, surveys, verification, A/B
 * knobs, phase timing) are declared in rt_hip_test.h.
 *
 * Threading: calls on distinct contexts may run concurrently on distinct host
 * threads; one context is not re-entrant.  rt_hip_render is asynchronous on
 * the given stream (NULL = the context's own stream); rt_hip_stats and
 * rt_hip_render_image synchronise.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include "rt_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Camera frame, cpu/raytracer.c:82-86: u = norm(cam.u), v = norm(cam.v),
 * C = pos + (u x v) * L with L = (float)(W / (2 tan(fov*pi/360))). */
typedef struct rt_frame {
  rt_vec3 u, v, C, position;
  int width, height;
} rt_frame;

/* Fails with RT_EINVAL for odd widths or heights: cpu/rt's output is
 * undefined there (cpu/raytracer.c:89-91,128-134 index the framebuffer two
 * different ways that agree only for even sizes). */
int rt_frame_from_camera(const rt_camera *cam, rt_frame *out);

/* Acceleration structure selection.  OCTREE: SAH octree built on the host
 * (host/accel.c); OCTREE_GPU: octree built on the device by rt_hip_create
 * (csrc/rt_build.hip, Morton keys + radix sort).  Both
 * render the same image; they differ in build time and traversal cost. */
enum { RT_ACCEL_FLAT = 0, RT_ACCEL_OCTREE = 1, RT_ACCEL_OCTREE_GPU = 2 };

/* Per-render counters.  closest = closest-hit queries
 * (collide() calls: camera + reflection rays), shadow = shadow queries
 * (collide_dist() calls), camera = 4*pixels rendered.  node_visits and
 * tri_tests (closest-hit queries) and shadow_node_visits / shadow_tri_tests
 * are only filled by the instrumented kernels (rt_hip_set_count_work) and
 * give the algorithmic bytes of the roofline. */
typedef struct rt_stats {
  unsigned long long closest, shadow, camera;
  unsigned long long node_visits, tri_tests;
  unsigned long long depth_overflow;   /* paths past RT_MAX_BOUNCES or a stack overflow (must be 0) */
  unsigned long long zero_normal;      /* winners with an exactly-zero interpolated normal */
  unsigned long long pixels;
  unsigned long long hits;             /* closest-hit queries that hit geometry */
  /* camera-ray exactness: triangles whose float test the
   * octree slack cannot guarantee, their tile-list entries (each tested by
   * the 64 pixels x 4 samples of the tile), and those every camera ray tests */
  unsigned long long cand_prims, cand_entries, cand_global;
  /* per-lane work of the instrumented pass (rt_hip_set_count_work): node
   * visits and triangle tests summed over the lanes that made them (a record
   * tested by k lanes of a wave counts k times; node_visits / tri_tests count
   * it once), for closest-hit and for shadow queries */
  unsigned long long closest_node_lanes, closest_tri_lanes;
  unsigned long long shadow_node_lanes, shadow_tri_lanes;
  /* instrumented pass: shader clocks the waves spent in the camera-ray walk,
   * the camera candidate tests, the secondary closest-hit walks and the
   * shadow queries (summed over waves) */
  unsigned long long cycles_camera, cycles_cand, cycles_secondary, cycles_shadow;
  unsigned long long cycles_shadow_directional;  /* the directional-light share of cycles_shadow */
  unsigned long long stack_spills;  /* per-lane stack pushes beyond the LDS entries (instrumented pass) */
  unsigned long long shadow_zero_risk;  /* shadow rays whose first hit lies on an object that can
                                         * interpolate a zero normal (must be 0, RT_EZERONORMAL) */
  unsigned long long hit_records;   /* closest hits recorded for shading (trace -> shade) */
  /* instrumented pass: wave-distinct node / triangle record fetches of the
   * shadow queries (shade kernel); node_visits / tri_tests are then those of
   * the closest-hit queries (trace kernel) */
  unsigned long long shadow_node_visits, shadow_tri_tests;
  /* point-light shadow rays whose origin lies beyond the extent the exact
   * shadow walk assumes (csrc/rt_shadow.hip; must be 0, RT_EINEXACT) */
  unsigned long long shadow_unproven;
  /* exact-shadow mode: shadow queries from origins off the proof box (float
   * garbage hits far past a triangle), decided by brute force after the
   * shade pass (rt_hip_set_exact_shadows) */
  unsigned long long shadow_deferred;
  /* exact reflection rays (rt_hip_set_exact_reflections): queries outside the
   * proven walk's assumption |d| <= RT_RF_DLMAX (must be 0, RT_EINEXACT) */
  unsigned long long closest_unproven;
} rt_stats;

/* Sizes of the device-side scene image, for the roofline accounting. */
typedef struct rt_accel_info {
  unsigned long long triangles;        /* scene triangles                        */
  unsigned long long tri_refs;         /* triangle records in traversal order    */
  unsigned long long nodes;            /* octree nodes (0 for FLAT)              */
  unsigned long long leaves;
  unsigned long long max_depth;
  unsigned long long tri_record_bytes; /* bytes per triangle record             */
  unsigned long long node_record_bytes;
  unsigned long long device_bytes;     /* total device memory of the scene image */
  double build_seconds;                /* build time (flatten + octree, host or device) */
  unsigned long long max_leaf;         /* largest leaf (triangle records)        */
  /* exact shadow rays (octree, csrc/rt_shadow.hip): triangles every
   * unshadowed shadow ray tests outside the walk, and the largest per-node
   * multiplier of the shadow walk's culling slack */
  unsigned long long shadow_global;
  double shadow_mu_max;
  /* light buffers of the default shadow queries (csrc/rt_lightbuf.hip):
   * cell entries over all lights, and triangles every query of their light
   * tests (footprint unbounded) */
  unsigned long long lightbuf_entries;
  unsigned long long lightbuf_global;
  double lightbuf_seconds;             /* their build time (device, at rt_hip_create) */
  /* proven light buffers (rt_hip_set_exact_shadows): triangles no shadow ray
   * of a light can make the float test accept (listed nowhere), and
   * triangles listed along a band of a point light's cube map */
  unsigned long long lightbuf_never;
  unsigned long long lightbuf_band;
  /* lights whose buffer could not be built (too many entries or cells, out
   * of device memory, a directional light with a zero vector): their shadow
   * queries walk the octree instead (the proven walk in the exact-shadow
   * mode).  Any other build failure fails the call (RT_EHIP). */
  unsigned long long lightbuf_failed;
  char lightbuf_fail_reason[96]; /* the last such fallback's cause ("" if none) */
  int trace_grid, shade_grid;    /* persistent one-wave workgroups of the default
                                    trace / shade kernels (occupancy-derived) */
  float scene_center[3], scene_radius;  /* the scene's box centre and half-extent (max-norm) */
} rt_accel_info;

typedef struct rt_hip_ctx rt_hip_ctx;

int rt_hip_device_count(int *n);

/* Deep-copies the scene into device memory of `device` (flattened SoA
 * triangle records, pre-normalised vertex normals, materials, lights) and
 * builds the acceleration structure.  The caller keeps ownership of scene. */
int rt_hip_create(int device, const rt_scene *scene, int accel, rt_hip_ctx **out);
int rt_hip_accel_info(const rt_hip_ctx *ctx, rt_accel_info *out);
void rt_hip_destroy(rt_hip_ctx *ctx);

/* Image tiling (csrc/rt_tiles.h): 8x8-pixel tiles grouped in blocks of tb x
 * tb tiles, tb = 4 (32x32 pixels) when nranks > 1 and 1 (scanline tile order)
 * for one rank; blocks b (scanline order over ceil(tiles_x/tb) x
 * ceil(tiles_y/tb) blocks) come in runs of nranks, run g = b / nranks holding
 * one block of every rank: block b belongs to rank (b % nranks + g) % nranks
 * as that rank's g-th block.  A rank's tile buffer holds its blocks in order,
 * tb*tb tiles each in row-major order, each tile 64 pixels x 3 floats (pixel
 * p of a tile = row p/8, col p%8 inside the tile); slots past the frame's
 * edge are padding (0).  rt_hip_tiles_per_rank() = the largest rank's tile
 * count, the size of every rank's buffer in a gather. */
int rt_hip_tiles_per_rank(int width, int height, int nranks);
size_t rt_hip_tile_buffer_floats(int width, int height, int nranks);

/* Renders every tile of `rank` into d_tiles (device memory of the context's
 * device, rt_hip_tile_buffer_floats() floats).  Asynchronous on `stream`
 * (a hipStream_t; NULL = the context's stream). */
int rt_hip_render(rt_hip_ctx *ctx, const rt_frame *frame, int rank, int nranks, float *d_tiles,
                  void *stream);
/* A caller that streams frames (enqueues the next rt_hip_render while the
 * last one runs) gets the next frame's candidate lists built on a second
 * stream of the context, beside the last frame's shade pass: the build waits
 * for that frame's trace kernel by an event, and `stream` waits for the
 * build before the trace, so every call stays ordered on `stream` as before
 * (default 1; the first frame of a size, a frame whose buffers grow, consumed
 * lists and rt_hip_render_compat build on `stream`).  Images and counters
 * are the same either way.  0 turns it off (A/B runs).  With it on, a timed
 * frame's list span and render span (include/rt_hip_test.h
 * rt_hip_frame_times) overlap the previous frame's and no longer add up to
 * the frame.  rt_hip_overlap_builds: the context's builds that ran on the
 * second stream so far. */
int rt_hip_set_overlap_lists(rt_hip_ctx *ctx, int enable);
int rt_hip_overlap_builds(const rt_hip_ctx *ctx, unsigned long long *n);
/* Waits for the last render and returns its counters.  The counters are
 * filled in whatever the return code: RT_EHITBUF (render again),
 * RT_EDEPTH / RT_EZERONORMAL (the image may differ from cpu/rt's there),
 * RT_EINEXACT (a parity-breaking tuning knob below was active, or a
 * point-light shadow ray left from beyond the proven extent). */
int rt_hip_stats(rt_hip_ctx *ctx, rt_stats *out);

/* Shadow rays exact by proof (default 1; rt_hip_set_exact_shadows rebuilds
 * the buffers now).  Each light buffer lists a triangle in every cell from
 * which some shadow ray can make the float Moller-Trumbore test accept it
 * (proven footprints, csrc/rt_lightbuf.hip); a query whose origin lies off the
 * proof's box (a float garbage hit far past a triangle) is deferred and
 * decided by brute force over every record after the shade pass (lights
 * 0..31; with more lights it is counted -> RT_EINEXACT).  Queries that walk
 * the octree (staged policies, light buffers off, a failed buffer, the
 * compatibility mode) use the proven walk: each node's box grown by a
 * per-node multiple of the culling slack covering every triangle below it,
 * plus a global list (csrc/rt_shadow.hip).  0: slack-grown
 * buffers and the plain-slack walk, whose decisions are measured against
 * brute force (rt_hip_verify_shadows), not proven; ~0.26 ms faster on C5. */
int rt_hip_set_exact_shadows(rt_hip_ctx *ctx, int enable);
/* Reflection rays exact by proof (default 0; builds the per-node bounds now).
 * The reflection walk grows each node's box by the reach of the reference
 * float Moller-Trumbore test's error region for that ray -- bounded through
 * the node's normal cone (the ray's cosine with every plane below it) and the
 * 1e-7f accept threshold -- and prunes with the matching distance error, so
 * every triangle the float test could accept is tested (csrc/rt_reflect.hip,
 * DESIGN.md §2).  0: the culling slack, whose reflection decisions are
 * tested (rt_hip_probe_closest), not proven.  Default traversal policy only
 * (rt_hip_render fails with RT_EINVAL otherwise); the closest-hit probe uses
 * the same walk. */
int rt_hip_set_exact_reflections(rt_hip_ctx *ctx, int enable);

/* Triangle-parallel camera candidate lists of an nranks-way frame (new; the
 * per-rank build of rt_hip_render runs the float fast path, classification
 * and emission over every triangle on every rank).  Each rank:
 *   1. rt_hip_cand_produce: the whole frame's list entries of triangles
 *      [rank P / nranks, (rank + 1) P / nranks), routed to the ranks that own
 *      their tiles; counts[d] = entries for rank d (global triangles included,
 *      one entry per rank each), *nglobal = this slice's global triangles.
 *      Synchronises its stream (the entry total).
 *   2. rt_hip_cand_send_buffer: the routed entries (device memory of the
 *      context, 3 x 32-bit words each, destination-rank order: counts[0]
 *      entries for rank 0, then rank 1's, ...), valid until the next produce.
 *   3. an all-to-all of those blocks (e.g. RCCL / torch.distributed
 *      all_to_all_single), every rank receiving its blocks from every rank,
 *      and the sum of the producers' *nglobal;
 *   4. rt_hip_cand_consume: this rank's lists from the n received entries
 *      (any source order); the next rt_hip_render of the same frame, rank and
 *      nranks uses them instead of building its own (once).
 * The lists equal the per-rank build's, tile by tile, as multisets (the
 * render is order-independent: the lexicographic (new_dist, prim) key).
 * Octree contexts with exact camera rays only (else RT_EINVAL).  stream:
 * as rt_hip_render. */
int rt_hip_cand_produce(rt_hip_ctx *ctx, const rt_frame *frame, int rank, int nranks, unsigned *counts,
                        unsigned *nglobal, void *stream);
int rt_hip_cand_send_buffer(const rt_hip_ctx *ctx, const void **d_entries, size_t *n);
int rt_hip_cand_consume(rt_hip_ctx *ctx, const rt_frame *frame, int rank, int nranks, const void *d_entries,
                        size_t n, unsigned nglobal, void *stream);
/* Steps 1-4 for n contexts of this process at once (ctx[r] = rank r, any
 * devices, e.g. all on one GPU): produce on every rank, the blocks moved by
 * device memcpys, consume on every rank; synchronous.  rt_raytrace_multi
 * makes the same exchange over RCCL (grouped ncclSend / ncclRecv) from 4
 * GPUs up. */
int rt_hip_cand_exchange_local(rt_hip_ctx **ctx, int n, const rt_frame *frame);

/* d_gathered = nranks consecutive tile buffers (rank-major, as an RCCL gather
 * delivers them); writes the PPM-order image (W*H*3 floats) to d_rgb. */
int rt_hip_assemble(rt_hip_ctx *ctx, const rt_frame *frame, const float *d_gathered, int nranks,
                    float *d_rgb, void *stream);

/* Convenience: single-GPU render of the whole frame into host memory
 * h_rgb (W*H*3 floats, PPM order); synchronous. */
int rt_hip_render_image(rt_hip_ctx *ctx, const rt_frame *frame, float *h_rgb, rt_stats *stats);

/* Relighting (new): the last rt_hip_render's image under edited lights and
 * materials without tracing it again.  A path's hit records (P, N, coef,
 * object) do not depend on the lights -- trace() recurses on obj.nr * coef
 * only (cpu/raytracer.c:19-34) and apply_light takes the hit, the object's
 * ka/kd/ks/ns and the lights (cpu/light.c:33-100) -- and a shadow decision
 * does not depend on a light's colour (cpu/light.c:24-31).  The context keeps
 * the records of its last render, and per record the unshadowed-light mask
 * of lights 0..31; a relight shades the records again, asking shadow queries
 * only for lights whose stored decision is not current, and the result is
 * bit for bit what a new context on the edited scene renders.
 * rt_raytrace_multi*, the CLIs and rt_hip_render_compat do not relight.
 *
 * rt_hip_set_lights replaces the light table (n may differ from the old
 * count; n = 0 is legal).  Synchronous setup, like rt_hip_set_exact_shadows:
 * it waits for the last render's stream, uploads the table, and rebuilds the
 * light buffer of exactly those lights whose (type, v) differs bitwise from
 * the old light at the same index, and of new indices; unchanged lights keep
 * their buffers, removed ones free theirs, a colour-only change builds
 * nothing.  A build past the entry cap or out of memory makes that light's
 * queries walk, as at rt_hip_create (rt_accel_info: lightbuf_failed,
 * lightbuf_fail_reason); the light-buffer totals of rt_accel_info are
 * recomputed.  Renders after it use the new table.
 *
 * rt_hip_set_materials takes ka, kd, ks, ns of objects[i] for every object
 * (`triangles` is ignored); n must equal the context's object count, and nr
 * -- all the trace reads of a material -- must equal the context's value
 * bitwise, else RT_EINVAL and nothing changes: reflectivity changes the
 * paths, which needs a new context.
 *
 * rt_hip_relight re-shades the kept records of the last rt_hip_render under
 * the current lights and materials and folds them into d_tiles; asynchronous
 * on `stream`.  RT_EINVAL, with nothing changed: no render yet; the last
 * render was of another frame (compared bytewise), rank or nranks; it ran on
 * another stream; it was rt_hip_render_compat; a non-default traversal policy
 * is set; rt_hip_set_count_work is on.  A rank without tiles writes nothing
 * and returns RT_OK.  A frame that overflowed its hit buffer relights what
 * it holds and rt_hip_stats reports RT_EHITBUF again.  The G-buffer of that
 * render stays valid (P, N and the winners do not depend on lights).  Which
 * lights are queried: a directional or point light's stored decision is
 * current iff its index is below 32, a shade pass of the kept records wrote
 * it (a render with keep-visibility on, or an earlier relight) and its
 * (type, v) has not changed since; lights from index 32 up are always
 * queried; ambient and other lights never.  A render without
 * keep-visibility, rt_hip_set_exact_shadows, rt_hip_set_light_buffers,
 * rt_hip_set_lightbuf_entry_cap, rt_hip_set_cull_slack (and
 * rt_hip_set_policy) and a reallocation of the hit buffers make every stored
 * decision stale; colours and materials never do.
 *
 * rt_hip_stats after a relight: the trace-side counters (closest, camera,
 * pixels, hits, zero_normal, depth_overflow, hit_records, cand_*) are the
 * traced frame's, the shadow-side ones (shadow, shadow_*, shadow_zero_risk,
 * shadow_unproven, shadow_deferred) the relight's: a relight that asked no
 * query reads shadow == 0.  rt_hip_frame_check counts renders only.
 *
 * rt_hip_set_keep_visibility (default 0): with 1, renders also write the
 * masks (4 B per record, allocated with the hit buffers), so the first relight
 * after a render can already skip queries.  With 0 renders are exactly what
 * they were, and the first relight of a frame allocates the buffer, asks every
 * query and writes the masks.
 *
 * rt_hip_relight_image: rt_hip_relight of the whole frame (one rank, the
 * context's stream: after rt_hip_render_image) into host memory; synchronous. */
int rt_hip_set_lights(rt_hip_ctx *ctx, const rt_light *lights, size_t n);
int rt_hip_set_materials(rt_hip_ctx *ctx, const rt_object *objects, size_t n);
int rt_hip_set_keep_visibility(rt_hip_ctx *ctx, int enable);   /* default 0 */
int rt_hip_relight(rt_hip_ctx *ctx, const rt_frame *frame, int rank, int nranks,
                   float *d_tiles, void *stream);
int rt_hip_relight_image(rt_hip_ctx *ctx, const rt_frame *frame, float *h_rgb, rt_stats *stats);

/* Moving geometry (new): new triangles in a live context, everything that
 * depends on them rebuilt on the device.  An animated object, a simulated
 * cloth or a skinned mesh needs no new rt_hip_create per frame: the caller's
 * vertices -- a device tensor already, with PyTorch-ROCm as the plumbing --
 * replace a range of the scene's triangles, and the device derives what
 * rt_hip_create's host flatten derives (host/accel.c rt_flatten): the records'
 * v0, e1 = v1 - v0, e2 = v2 - v0, the normalised vertex normals (the same IEEE
 * sqrt and quotients as the host's), the scene's bounding box over every
 * triangle (a partial update can shrink it) and each touched object's
 * zero-normal risk flag from all of its triangles (csrc/rt_geom.hip).
 *
 * rt_hip_set_triangles replaces the triangles [first, first + count) of the
 * scene, in prim order (object, then the object's triangle index: the order of
 * rt_gsample.prim), by `count` records of rt_triangle layout (18 floats:
 * vertex[3], normal[3]) read from d_triangles, device memory of the context's
 * device, on the context's stream.  rt_hip_set_triangles_host uploads them
 * first.  The topology stays as created: the objects, their triangle counts
 * and the prim numbering do not change.  Values are taken as rt_hip_create
 * takes the scene's: no validation, a non-finite vertex is as undefined as it
 * is there.
 *
 * Synchronous setup, like rt_hip_set_lights: it waits for the context's last
 * stream and for the side stream, and returns when everything is rebuilt, in
 * rt_hip_create's order -- the octree (RT_ACCEL_OCTREE_GPU; a FLAT context's
 * records are its scene image), the light buffers with create's fallbacks,
 * the proven shadow walk's multipliers and the exact-reflection bounds where
 * the context had built them.  rt_accel_info's build_seconds and
 * lightbuf_seconds become those of the update.
 *
 * After RT_OK every later call on the context gives what the same call gives
 * on a fresh context made by rt_hip_create on the edited scene with the same
 * accel and brought to the same settings, bit for bit: images, G-buffer
 * records, ray-batch colours and hit records, occlusion bytes, every rt_stats
 * counter, every non-timing field of rt_accel_info, rt_hip_accel_validate.
 * Buffer capacities are the only exceptions: the hit-record buffers keep
 * their size and the list forecast starts over, so either side may answer a
 * first frame with RT_EHITBUF where the other does not (render again, as
 * rt_hip_render_image does).  The settings (exact shadows, exact reflections,
 * G-buffer, keep-visibility, slacks, policy, overlap) and the lights and
 * materials as last edited persist.  What described the old geometry is
 * forgotten: the kept frame (rt_hip_relight and rt_hip_gbuffer return
 * RT_EINVAL until the next rt_hip_render), consumed candidate lists, the list
 * forecast, the item clocks, the last batch.
 *
 * RT_EINVAL, with nothing changed: a NULL context; a NULL pointer with
 * count > 0; first + count past the context's triangle count; a context whose
 * octree was built on the host (RT_ACCEL_OCTREE: its tree comes from the
 * rt_scene -- make a new context or use RT_ACCEL_OCTREE_GPU).  count == 0 is
 * RT_OK and a true no-op: nothing is invalidated, a kept frame still relights.
 * A failure after the records were touched (RT_EHIP, out of memory in the tree
 * or a buffer) leaves the context broken: every entry point that takes it,
 * but rt_hip_set_triangles*, rt_hip_geometry_updates, rt_hip_accel_info and
 * rt_hip_destroy, then returns RT_EINVAL with a message that says so; a later
 * successful update heals it.
 *
 * Not here: refitting the tree without a rebuild, changing triangle counts,
 * host-tree contexts, a transform API (the caller's tensor library does
 * that), rt_raytrace_multi (it owns its contexts). */
int rt_hip_set_triangles(rt_hip_ctx *ctx, const void *d_triangles, size_t first, size_t count);
int rt_hip_set_triangles_host(rt_hip_ctx *ctx, const rt_triangle *h_triangles, size_t first, size_t count);
int rt_hip_geometry_updates(const rt_hip_ctx *ctx, unsigned long long *n);   /* successful updates so far */

/* Per-sample G-buffer (new; opt-in, default off): what the renderer knows
 * about each of a pixel's four camera samples beside its colour.  One record
 * of RT_GB_WORDS 32-bit words per sample, 4 per pixel in cpu sample order:
 * sample s has k = i + 0.5 (s >> 1), l = j + 0.5 (s & 1) (cpu/raytracer.c:55-58).
 *   prim     winner of collide() for the camera ray: the global triangle index
 *            in (object, LIFO triangle) order = the triangle counts of the
 *            earlier objects + the index into objects[obj].triangles; -1: miss
 *   obj      the winner's object index; -1: miss
 *   queries  closest-hit queries of the sample's path: the camera ray, every
 *            reflection and the final miss (the coef < 0.01 cut-off makes none)
 *   dist     the winner's new_dist (cpu/hit.c); +inf: miss
 *   P, N     hit point and interpolated normal, the bits the shading used;
 *            0 for a miss and for a winner whose interpolated normal is
 *            exactly zero (counted in rt_stats.zero_normal)
 * With the G-buffer on, rt_hip_render runs the default trace kernel's
 * capturing instantiation (16 B more per sample); lists, shading and the
 * image are unchanged.  It fails with RT_EINVAL together with a non-default
 * traversal policy, rt_hip_set_count_work or rt_hip_set_exact_reflections;
 * rt_hip_render_compat captures nothing.  The G-buffer is valid whenever the
 * image is (after RT_EHITBUF: render again). */
#define RT_GB_WORDS 10
typedef struct rt_gsample { int prim, obj, queries; float dist, P[3], N[3]; } rt_gsample;
int rt_hip_set_gbuffer(rt_hip_ctx *ctx, int enable);
/* Words of a rank's G-buffer tile buffer: the layout of the colour tile
 * buffer ("Image tiling" above) with 4 * RT_GB_WORDS words per pixel slot
 * (sample-major) in place of 3 floats; padding slots are misses of 0 queries. */
size_t rt_hip_gbuffer_tile_words(int width, int height, int nranks);
/* The G-buffer tiles of the last rt_hip_render, which must have been of the
 * same frame, rank and nranks with the G-buffer on, on the same stream (else
 * RT_EINVAL).  Asynchronous.  A rank without tiles writes nothing. */
int rt_hip_gbuffer(rt_hip_ctx *ctx, const rt_frame *frame, int rank, int nranks, void *d_tiles,
                   void *stream);
/* rt_hip_assemble for G-buffer tile buffers: d_samples receives H*W*4
 * rt_gsample in PPM pixel order. */
int rt_hip_assemble_gbuffer(rt_hip_ctx *ctx, const rt_frame *frame, const void *d_gathered, int nranks,
                            void *d_samples, void *stream);
/* rt_hip_render_image plus the G-buffer (on for this call only);
 * h_samples = H*W*4 records, PPM order. */
int rt_hip_render_image_gbuffer(rt_hip_ctx *ctx, const rt_frame *frame, float *h_rgb,
                                rt_gsample *h_samples, rt_stats *stats);

/* Ray batches (new): trace rays the caller supplies instead of the pinhole
 * camera's -- a panorama, an orthographic view, a light probe's faces, a pick
 * ray, a line-of-sight query.  Ray i is (d_origins[3i..], d_dirs[3i..]),
 * device memory of the context's device; the direction is used as given, not
 * normalised (the reference's bounce directions are not either).
 *
 * rt_hip_trace_rays writes to d_rgb[3i..] the float channels of the
 * reference's trace(ray_i, 1.0) (cpu/raytracer.c:19-34): its recursion, the
 * coef < 0.01 cut-off, the bounce limit (rt_stats.depth_overflow, never
 * silent) and the zero-normal rule, exactly as a camera sample's path; and to
 * d_samples, if not NULL, n rt_gsample records (8-byte aligned) of the rays'
 * first hits, the fields as above.  d_rgb == NULL with d_samples != NULL is a
 * pure ray cast: one closest-hit query per ray, no bounce, no shade pass,
 * queries == 1.  Both NULL: RT_EINVAL.  A ray with a non-finite component or
 * an all-zero direction is not traced: colour 0, a miss of 0 queries.  n == 0
 * returns RT_OK and writes nothing; n > RT_RAYS_MAX (what a hit record's index
 * addresses) is RT_EINVAL.  Asynchronous on `stream`, with rt_hip_render's
 * threading rules.  RT_EINVAL with a non-default traversal policy or
 * rt_hip_set_count_work.
 *
 * Every query of a batch, the first included, is what a reflection ray's
 * query is on this context: the per-lane octree walk at the culling slack
 * (tested against brute force, not proven), the proven walk under
 * rt_hip_set_exact_reflections, brute force on a FLAT context; no camera
 * candidate lists.  The proven walk assumes |d| <= 1.0625: proven mode wants
 * normalised directions, and a batch with a longer one still traces but
 * rt_hip_stats returns RT_EINEXACT with closest_unproven counted.  With
 * RT_RAYS_PACKET the first query of each aligned group of 64 rays walks the
 * octree as one packet: a promise about the caller's ray order (coherent
 * groups, e.g. rt_hip_frame_rays order 1) that only buys speed -- the results
 * are the same bits with and without it; ignored under exact reflections and
 * on FLAT.  Shadow rays start on scene triangles as always, so the light
 * buffers and their proof apply unchanged.
 *
 * A batch uses the context's hit-record buffers (first sized for two records
 * per ray): on overflow rt_hip_stats returns RT_EHITBUF, the buffers grow and
 * the batch must be traced again, as a render.  rt_hip_stats after a batch:
 * camera = rays traced, pixels = 0, cand_* = 0, every other counter as for a
 * render; rt_hip_frame_check accounts a batch like a render.  A batch
 * overwrites the last render's hit records: rt_hip_relight and rt_hip_gbuffer
 * return RT_EINVAL after it until the next rt_hip_render.  It touches no
 * candidate list, so a batch between two frames of a streaming caller leaves
 * both frames as they are. */
#define RT_RAYS_PACKET 1u   /* each aligned group of 64 rays walks its first query as one packet */
#define RT_RAYS_MAX 0xfffffff8ull  /* 8 regions x (2^29 - 1) record slots */
int rt_hip_trace_rays(rt_hip_ctx *ctx, const float *d_origins, const float *d_dirs, size_t n,
                      unsigned flags, float *d_rgb, void *d_samples, void *stream);
/* Upload, rt_hip_trace_rays on the context's stream, download, rt_hip_stats;
 * synchronous.  Traces again once after RT_EHITBUF, as rt_hip_render_image. */
int rt_hip_trace_rays_host(rt_hip_ctx *ctx, const float *h_origins, const float *h_dirs, size_t n,
                           unsigned flags, float *h_rgb, rt_gsample *h_samples, rt_stats *stats);
/* The 4 W H camera rays of `frame` (3 floats each), computed on the device by
 * the arithmetic of the render's camera samples (cpu/raytracer.c:55-60).
 * order 0: PPM pixel order, ray 4 (row W + col) + s, s in cpu sample order
 * (rt_gsample above).  order 1: by 4x4-pixel quarter, quarters in scanline
 * order, each aligned 64 rays one quarter's 16 pixels (row-major) x 4 samples,
 * ray 64 quarter + 4 pixel + s -- the groups a render's trace walks as packets;
 * width and height must be multiples of 4.  Odd sizes are RT_EINVAL. */
int rt_hip_frame_rays(rt_hip_ctx *ctx, const rt_frame *frame, int order,
                      float *d_origins, float *d_dirs, void *stream);
/* rt_hip_frame_rays on the context's stream into host memory; synchronous. */
int rt_hip_frame_rays_host(rt_hip_ctx *ctx, const rt_frame *frame, int order,
                           float *h_origins, float *h_dirs);

/* Occlusion batches (new): "is anything in the way, up to this far?" for rays
 * the caller supplies -- ambient occlusion, visibility between two points,
 * light baking, line of sight.  The any-hit query behind the reference's
 * has_direct_hit (cpu/light.c:24-31), with a distance bound.  Ray i is
 * (d_origins[3i..], d_dirs[3i..]) as for rt_hip_trace_rays, the direction used
 * as given; with D = collide_dist(scene, ray_i) of cpu/hit.c:93-109 (the least
 * new_dist > 0.01 over the triangles ray_intersect accepts, 0 if none),
 *
 *     d_occluded[i] = (D != 0 && D <= d_tmax[i])     float compare
 *
 * d_tmax[i] is a world distance |hit point - origin| in the units of new_dist,
 * not the Moller-Trumbore parameter: it does not scale with |d|.  d_tmax ==
 * NULL means +inf for every ray, i.e. has_direct_hit.  A ray rt_hip_trace_rays
 * would not trace (a non-finite component, an all-zero direction) and a ray
 * whose tmax is NaN are not traced: byte 0.  A traced ray with tmax <= 0
 * answers 0 without a query.  One byte per ray; bytes past n are never
 * written.  n == 0 returns RT_OK and writes nothing; n > RT_RAYS_MAX, a NULL
 * ray or output pointer, a non-default traversal policy or
 * rt_hip_set_count_work: RT_EINVAL with nothing changed.  Asynchronous on
 * `stream`, with rt_hip_render's threading rules.
 *
 * The answer is the same on every path: brute force over every record on a
 * FLAT context; on octree contexts a per-lane any-hit walk at the culling slack
 * that skips a node only when the ray misses its slack-grown box or the
 * closest walk's prune rule puts it beyond tmax (tested against brute force,
 * not proven, as a reflection ray's query; the plain slack boxes, not the
 * shadow rays' proof, which is about the scene's lights); under
 * rt_hip_set_exact_reflections the proven closest walk, answering dist <= tmax
 * -- proven for |d| <= 1.0625, a longer direction is counted in
 * closest_unproven and rt_hip_stats returns RT_EINEXACT, as for a ray batch.
 * With RT_RAYS_PACKET each aligned group of 64 rays walks as one packet: the
 * same bytes, faster for coherent groups; ignored on FLAT and under exact
 * reflections.  A hit on an object whose interpolated normal can vanish is
 * counted in shadow_zero_risk (RT_EZERONORMAL), never silent.
 *
 * A batch writes no hit record, so the kept frame survives it: rt_hip_relight,
 * rt_hip_gbuffer and a streaming caller's next frame behave as if the batch had
 * not happened.  rt_hip_stats directly after a batch describes the batch --
 * camera = rays traced, shadow = traced rays with tmax > 0 (the queries),
 * depth_overflow, shadow_zero_risk and closest_unproven as counted, every other
 * counter 0 -- and after a later relight what it would have read without the
 * batch.  rt_hip_frame_check counts renders only, as for a relight. */
int rt_hip_occluded(rt_hip_ctx *ctx, const float *d_origins, const float *d_dirs, const float *d_tmax,
                    size_t n, unsigned flags, unsigned char *d_occluded, void *stream);
/* Upload, rt_hip_occluded on the context's stream, download, rt_hip_stats;
 * synchronous. */
int rt_hip_occluded_host(rt_hip_ctx *ctx, const float *h_origins, const float *h_dirs, const float *h_tmax,
                         size_t n, unsigned flags, unsigned char *h_occluded, rt_stats *stats);

/* Ambient occlusion from G-buffer records (new): for each of n rt_gsample
 * records in device memory -- a rank's tile buffer straight from
 * rt_hip_gbuffer, the assembled samples, the records of a ray batch -- the
 * number of its k hemisphere rays that are occluded within tmax.  The rays are
 * made in the kernel; no ray array exists.  d_occluded[i] (one 32-bit word per
 * record, 0..k) is written exactly once for every i < n, nothing past n; the
 * output needs no clearing.
 *
 * The ray rule (csrc/rt_ao_items.h is its one statement, rtgpu.ao_rays_host
 * its numpy float32 twin; every step is a correctly rounded float operation in
 * the written order, no FMA, so host and device agree in every bit):
 *   shoots   s = (N.x N.x + N.y N.y) + N.z N.z in float, l = (float)sqrt((double)s);
 *            record i shoots iff prim >= 0 and 0 < l < +inf.  A miss and a NaN,
 *            zero, underflowing or overflowing normal do not: count 0.
 *   frame    n = N / l;  sg = copysignf(1, n.z);  a = -1 / (sg + n.z);
 *            b = n.x n.y a;  T = (1 + sg n.x n.x a, sg b, -sg n.x);
 *            B = (b, sg + n.y n.y a, -n.y), each product left to right.  No
 *            sine or cosine anywhere.
 *   hash     g = base + i (64-bit);  h = mix32((uint32)g ^ mix32((uint32)(g >> 32) + seed)),
 *            mix32(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16.
 *   ray r    (0 <= r < k) takes row ((h >> 3) % m + r) % m of d_table (m rows of
 *            3 floats, local directions with z > 0 about +z, e.g. cosine
 *            weighted unit vectors); bit 0 of h swaps the row's x and y, then
 *            bit 1 negates x and bit 2 negates y;  d = (x T + y B) + z n per
 *            component, not normalised afterwards; the origin is P.
 * `base` is the index of record 0 in the caller's whole set: a set cut into
 * pieces, each with its base, gives the whole set's words.
 *
 * Each generated ray is then exactly ray j of an occlusion batch with
 * d_tmax[j] = tmax (rt_hip_occluded above): the same traced / query rules (a
 * non-finite P, a NaN tmax: not traced; tmax <= 0: no query), the same walks,
 * RT_RAYS_PACKET with the same meaning (each work item's rays as one packet:
 * the same counts), the same answer on FLAT, octree and proven contexts.
 * tmax = +inf is has_direct_hit.  A record's count is the number of its k rays
 * whose byte would be 1.  rt_hip_ao_rays writes the rays themselves, in ray
 * order j = i k + r, 3 floats each for origin and direction -- zeros for a
 * record that does not shoot, a ray no batch traces -- and, if d_shot is not
 * NULL, one byte per record saying whether it shot.
 *
 * To the context the call is an occlusion batch: the kept frame survives it,
 * rt_hip_stats directly after reads camera = rays traced, shadow = queries,
 * depth_overflow, shadow_zero_risk and closest_unproven as counted and every
 * other counter 0; a streaming caller's frames are unchanged.  Asynchronous on
 * `stream`.  RT_EINVAL with nothing changed: a NULL context; NULL samples,
 * table or output with n > 0; samples not 8-byte aligned; k == 0 or k >
 * RT_AO_KMAX; m == 0; n k > RT_RAYS_MAX; flags other than RT_RAYS_PACKET; a
 * non-default traversal policy; rt_hip_set_count_work.  n == 0 returns RT_OK
 * and writes nothing. */
#define RT_AO_KMAX 1024
int rt_hip_ambient_occlusion(rt_hip_ctx *ctx, const void *d_samples, size_t n, unsigned long long base,
                             unsigned k, const float *d_table, unsigned m, unsigned seed, float tmax,
                             unsigned flags, unsigned *d_occluded, void *stream);
/* Upload, rt_hip_ambient_occlusion on the context's stream, download,
 * rt_hip_stats; synchronous. */
int rt_hip_ambient_occlusion_host(rt_hip_ctx *ctx, const rt_gsample *h_samples, size_t n,
                                  unsigned long long base, unsigned k, const float *h_table, unsigned m,
                                  unsigned seed, float tmax, unsigned flags, unsigned *h_occluded,
                                  rt_stats *stats);
int rt_hip_ao_rays(rt_hip_ctx *ctx, const void *d_samples, size_t n, unsigned long long base, unsigned k,
                   const float *d_table, unsigned m, unsigned seed, float *d_origins, float *d_dirs,
                   unsigned char *d_shot /* may be NULL */, void *stream);
/* Upload, rt_hip_ao_rays on the context's stream, download; synchronous. */
int rt_hip_ao_rays_host(rt_hip_ctx *ctx, const rt_gsample *h_samples, size_t n, unsigned long long base,
                        unsigned k, const float *h_table, unsigned m, unsigned seed, float *h_origins,
                        float *h_dirs, unsigned char *h_shot /* may be NULL */);

/* Traced light gathered over a record's hemisphere (new): what a lightmap
 * bake, a probe bake or a one-bounce final gather needs -- for each of n
 * rt_gsample records in device memory, k rays over its hemisphere, the
 * reference's trace(ray, 1.0) on each, and the colours added up.  The records,
 * n, base, k, d_table, m and seed are rt_hip_ambient_occlusion's, and so are
 * the rays; they are made in the trace kernel and exist in no array.  There is
 * no tmax.
 *
 * The contract is a composition of calls above.  Let (o_j, d_j), j = i k + r,
 * be the rays rt_hip_ao_rays writes for the same records, k, table, m, seed
 * and base, and c_j the colour rt_hip_trace_rays writes for ray j on this
 * context in its current settings (an untraced ray has colour 0: that covers a
 * record that does not shoot, whose directions are all zero).  Then
 *     d_rgb[3i .. 3i+2] = acc_k,  acc_0 = (+0, +0, +0),
 *     acc_{r+1} = color_add(acc_r, c_{i k + r})        (cpu/colors.c: a float
 *                 add per channel, then the clamp `if (x > 255) x = 255`)
 * in ray order, in float, one add per channel per ray.  That order is the
 * rule: no tree or wave reduction replaces it.  The sum is not divided by k
 * and carries no cosine or weight: the caller's table is the distribution.
 * rtgpu.gather_sum is the rule's numpy float32 twin.  Every word of [0, 3 n)
 * is written exactly once, with plain stores, nothing past it; the output
 * needs no clearing.  k ranges over 1 .. RT_AO_KMAX.
 *
 * The queries are a reflection ray's, as a ray batch's: tested against brute
 * force by default, proven under rt_hip_set_exact_reflections, brute force on
 * a FLAT context; no candidate list.  Table directions are near unit length; a
 * longer one (|d| > 1.0625) counts in closest_unproven under the proven walk,
 * as for a batch.  RT_RAYS_PACKET means what it means for a ray batch: each
 * work item's rays (whole records side by side, 64 / k of them; one record's
 * rounds of 64 for k > 64) walk their first query as one packet -- the same
 * bits, only faster for coherent groups; ignored on FLAT and under exact
 * reflections.
 *
 * To the context a gather is a ray batch.  It uses and overwrites the
 * hit-record buffers (first sized for two records per path): rt_hip_relight
 * and rt_hip_gbuffer return RT_EINVAL after it until the next rt_hip_render.
 * rt_hip_stats after it reads as after rt_hip_trace_rays on those rays: camera
 * = rays traced, pixels = 0, cand_* = 0, every other counter as for a render;
 * on RT_EHITBUF the buffers grow and the call must be made again.
 * rt_hip_frame_check accounts it like a batch.  It touches no candidate list:
 * a gather between two frames of a streaming caller leaves both as they are.
 * Asynchronous on `stream`, with rt_hip_render's threading rules.
 *
 * RT_EINVAL with nothing changed: a NULL context; NULL samples, table or d_rgb
 * with n > 0; samples not 8-byte aligned; k == 0 or k > RT_AO_KMAX; m == 0;
 * n k > RT_RAYS_MAX; flags other than RT_RAYS_PACKET; a non-default traversal
 * policy; rt_hip_set_count_work; a context left broken by a failed geometry
 * update.  n == 0 returns RT_OK and writes nothing. */
int rt_hip_gather(rt_hip_ctx *ctx, const void *d_samples, size_t n, unsigned long long base, unsigned k,
                  const float *d_table, unsigned m, unsigned seed, unsigned flags, float *d_rgb,
                  void *stream);
/* Upload, rt_hip_gather on the context's stream, download, rt_hip_stats;
 * synchronous.  Gathers again once after RT_EHITBUF, as rt_hip_trace_rays_host. */
int rt_hip_gather_host(rt_hip_ctx *ctx, const rt_gsample *h_samples, size_t n, unsigned long long base,
                       unsigned k, const float *h_table, unsigned m, unsigned seed, unsigned flags,
                       float *h_rgb, rt_stats *stats);

/* Direct light for caller's surface records (new): for each of n rt_gsample
 * records in device memory (8-byte aligned; a rank's tile buffer straight from
 * rt_hip_gbuffer, the assembled samples, a ray batch's records, or points of
 * the caller's own: lightmap texels, probes in free space), d_rgb[3 i ..]
 * receives the three float channels of
 *     apply_light(scene, objects[obj_i], (P_i, N_i))      (cpu/light.c:33-100)
 * under the context's current lights and materials (rt_hip_set_lights,
 * rt_hip_set_materials): the lights summed in file order with the reference's
 * colour algebra, N used as given (not normalised), no coef, no reflection.
 * The specular term needs no view direction (cpu/light.c:7-22).  d_lit[i], if
 * d_lit is not NULL, receives the unshadowed mask in the sense of a relight:
 * bit li (li < 32) is set iff light li is directional or point and
 * collide_dist of its shadow ray from P_i (cpu/light.c:51-54, 76-80) is 0.
 * Lights from index 32 up count in the colour and have no bit.
 *
 * A record shades iff prim >= 0, 0 <= obj < the context's object count, every
 * component of P and N is finite and N is not zero by vector3_is_zero
 * (csrc/rt_dlight_items.h is the one statement, rtgpu.direct_light_shades its
 * numpy twin).  Every other record -- a miss, the G-buffer's zero-normal
 * winner, a non-finite point -- gets colour 0 0 0 and mask 0.  Every output
 * word of [0, n) is written exactly once, nothing past it; the outputs need no
 * clearing.
 *
 * Every shadow decision is has_direct_hit (cpu/light.c:24-31); the route only
 * decides how it is found.  FLAT: brute force.  Octree: through the light's
 * buffer when it has one and P lies in the buffer's proof box (proven in the
 * default exact-shadow mode); otherwise -- P off the box, the build failed,
 * rt_hip_set_light_buffers off -- by the walk of an occlusion batch without a
 * distance bound (tested at the default culling slack; proven under
 * rt_hip_set_exact_reflections for directions within that walk's bound, a
 * longer walked ray -- most point lights' -- is counted in closest_unproven
 * and rt_hip_stats reports RT_EINEXACT, as for an occlusion batch).  Nothing
 * is deferred.  Unlike a batch, a
 * shadow ray with a zero or huge direction (a light at P, a zero light vector,
 * a light 3e38 away) is asked like any other, as the reference asks it.
 * RT_RAYS_PACKET: the 64 records of a work item walk one light's rays as a
 * packet; the same bytes.
 *
 * To the context the call is an occlusion batch: it writes no hit record, the
 * kept frame survives it, rt_hip_frame_check counts renders only, and
 * rt_hip_stats directly after reads camera = records that shaded, shadow =
 * queries asked, shadow_deferred = queries of lights with a buffer that left
 * its proof box and walked, shadow_zero_risk, closest_unproven and
 * depth_overflow as counted, shadow_unproven and every other counter 0.
 * Asynchronous on `stream`.  RT_EINVAL with nothing changed: a NULL context;
 * NULL samples or d_rgb with n > 0; samples not 8-byte aligned; n >
 * RT_RAYS_MAX; flags other than RT_RAYS_PACKET; a non-default traversal
 * policy; rt_hip_set_count_work; a context left broken by a failed geometry
 * update.  n == 0 returns RT_OK and writes nothing. */
int rt_hip_direct_light(rt_hip_ctx *ctx, const void *d_samples, size_t n, unsigned flags,
                        float *d_rgb, unsigned *d_lit /* may be NULL */, void *stream);
/* Upload, rt_hip_direct_light on the context's stream, download, rt_hip_stats;
 * synchronous. */
int rt_hip_direct_light_host(rt_hip_ctx *ctx, const rt_gsample *h_samples, size_t n, unsigned flags,
                             float *h_rgb, unsigned *h_lit /* may be NULL */, rt_stats *stats);

/* A ray batch's paths written out (new): every bounce as a surface record.
 * The tracer keeps a hit record per bounce of every ray (P, N, coef, obj, the
 * link to the bounce before it and, after the shade pass, its term
 * color_mul(apply_light(...), coef)); the fold sums each ray's chain
 * deepest-first.  This call hands the chains to the caller: a CSR offset per
 * ray and, per path vertex, an rt_gsample that rt_hip_ambient_occlusion,
 * rt_hip_direct_light, rt_hip_gather and rt_hip_ao_rays take as it is, the
 * vertex's coef and its term.  What a mirror shows can then be given ambient
 * occlusion or gathered light (a frame with indirect light is the sum over
 * every vertex k of coef_k (direct_k + gathered_k)), and bounces can be shaded
 * by the caller without tracing them again ray by ray.
 *
 * Which batch: the paths are those of the context's last rt_hip_trace_rays
 * that traced (n > 0) with d_rgb != NULL, with or without d_samples or
 * RT_RAYS_PACKET; n must be that batch's n.
 *
 * What a path is: the chain the batch's fold walked for ray i -- from the
 * ray's deepest record, while the index names a record the buffers hold, along
 * the links -- written out in reverse: vertex 0 is the ray's first hit, the
 * last vertex the deepest.  len_i is the chain's length; a miss, an untraced
 * ray (rt_hip_trace_rays) and a first-hit winner with a zero normal have
 * len_i = 0.  The walk is bounded by the tracer's bounce limit.
 *
 * d_offsets: n + 1 words, the exclusive scan of len; d_offsets[n] is the true
 * total even when it exceeds cap (it fits 32 bits: RT_RAYS_MAX bounds the
 * records).  All n + 1 words hold their values when the call completes,
 * nothing past them is written; no clearing needed.  d_records, d_coef and
 * d_terms may each be NULL.  Vertex v of ray i has index j = d_offsets[i] + v
 * and is written iff j < cap: nothing at or past cap is written.  With all
 * three NULL the call only counts and cap is ignored.  Per written vertex:
 *     d_records[j]      an rt_gsample (8-byte aligned): P, N and obj are the
 *                       hit record's bits; prim = RT_PATH_PRIM (the hit records
 *                       do not keep the triangle; the consumers read the sign
 *                       only); queries = v; dist = +0
 *     d_coef[j]         the record's coef: 1 for vertex 0, then the product of
 *                       the nr of the objects before it (cpu/raytracer.c:29)
 *     d_terms[3j..3j+2] the record's shaded term, under the lights and
 *                       materials of the batch
 * The terms fold to the batch's colours: color_add from (+0, +0, +0) over a
 * ray's terms, deepest first, is d_rgb of that ray, word for word
 * (rtgpu.path_fold).  The records chain hop by hop: a ray cast from P_v along
 * ray_bounce(d_v, N_v) (cpu/ray.c:16-25) has vertex v + 1 as its first hit.
 * Without an overflow rt_stats.hit_records of the batch is the total: a
 * caller sizes cap from it without a second call.
 *
 * To the context: the call reads only (calling it again gives the same
 * words), asynchronous on `stream`, which must be the batch's stream.  The
 * paths survive what the kept frame survives (rt_hip_occluded,
 * rt_hip_ambient_occlusion, rt_hip_ao_rays, rt_hip_direct_light,
 * rt_hip_frame_rays, rt_hip_stats) and also rt_hip_set_lights and
 * rt_hip_set_materials (the terms stay the batch's own).  They are gone after
 * anything that writes or moves hit records: rt_hip_render,
 * rt_hip_render_compat, a ray cast or a newer batch (which replaces them),
 * rt_hip_gather, rt_hip_set_triangles, any reallocation of the hit buffers.
 * After RT_EHITBUF the call exports what the fold saw -- its terms still fold
 * to what that batch wrote to d_rgb -- and the caller traces again as before.
 *
 * RT_EINVAL with nothing written and nothing changed: a NULL context; a
 * context left broken by a failed geometry update; no such batch kept (the
 * message names the call that took it); n other than the batch's; NULL
 * d_offsets; d_records not 8-byte aligned; another stream. */
#define RT_PATH_PRIM 0x7fffffff   /* a hit whose triangle the hit records do not keep */
int rt_hip_path_records(rt_hip_ctx *ctx, size_t n, unsigned *d_offsets, size_t cap,
                        void *d_records, float *d_coef, float *d_terms, void *stream);
/* Allocate, rt_hip_path_records on the batch's stream, download (offsets
 * whole, the arrays up to min(total, cap) vertices), synchronise. */
int rt_hip_path_records_host(rt_hip_ctx *ctx, size_t n, unsigned *h_offsets, size_t cap,
                             rt_gsample *h_records, float *h_coef, float *h_terms);

/* gpu/rt compatibility mode (gpu/raytracer.cu:31-129,
 * gpu/light.cu, gpu/colors.cu): the camera's frame rendered at 3x width and
 * height with one ray per high-resolution pixel, uint8 saturating colours,
 * reflections summed front to back over at most 11 closest-hit queries, then
 * a 3x3 box downscale.  h_rgba receives width x height RGBA8 pixels (alpha
 * 255) in gpu/rt's PNG row order.  stats as rt_hip_stats (camera = pixels =
 * high-resolution rays).  Camera rays keep the exactness of cpu mode: the
 * per-frame candidate lists of the 3x frame's one-ray-per-pixel camera
 * (csrc/rt_cand.h CandParams::compat, csrc/rt_cand_geom.h pixel_range). */
int rt_hip_render_compat(rt_hip_ctx *ctx, const rt_camera *cam, unsigned char *h_rgba,
                         rt_stats *stats);
/* Drop-in for gpu/rt's main (gpu/rt.cpp:56-97): load, render in
 * compatibility mode on GPU 0, write an 8-bit RGBA PNG.  accel < 0: choose. */
int rt_raytrace_gpu(const char *input, const char *output, int accel);

/* Device memory helpers so C callers need no HIP headers. */
int rt_hip_malloc(int device, size_t bytes, void **d_ptr);
int rt_hip_free(void *d_ptr);
int rt_hip_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);
int rt_hip_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
/* device -> device, asynchronous on stream (NULL: the null stream) */
int rt_hip_memcpy_d2d(void *d_dst, const void *d_src, size_t bytes, void *stream);

/* Drop-in for raytrace() (cpu/raytracer.c:79-136): parse, render on GPU 0,
 * write the P3 PPM.  Returns an RT_E* code instead of exiting. */
int rt_raytrace(const char *input, const char *output);

/* Same with the frame tiled over `ngpus` devices of this node and gathered
 * to device 0 with one RCCL gather over xGMI.  accel = RT_ACCEL_*.
 * stats (optional) receives the summed counters; render_ms the wall time of
 * render + gather. */
int rt_raytrace_multi(const char *input, const char *output, int ngpus, int accel,
                      rt_stats *stats, double *render_ms);

/* rt_raytrace_multi with rank g on device devices[g].  Distinct devices: as
 * rt_raytrace_multi (RCCL).  A device shared by several ranks (tests running
 * N ranks on one GPU): the same frame with device memcpys in place of the
 * RCCL calls (the candidate lists' exchange from 4 ranks up, the gather). */
int rt_raytrace_multi_dev(const char *input, const char *output, int ngpus, const int *devices, int accel,
                          rt_stats *stats, double *render_ms);

#ifdef __cplusplus
}
#endif
#endif
