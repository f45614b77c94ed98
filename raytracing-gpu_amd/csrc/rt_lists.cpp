// rt_lists.cpp -- the camera rays' candidate lists on the context's side
// (DESIGN.md §2 "Exact camera rays", §4 "Candidate-list kernels"): the
// per-rank build (cand_prepare: fast path -> classification -> emission ->
// refinement -> compaction -> sort -> offsets -> work order), the
// triangle-parallel produce / consume of an N-rank frame, and the entry
// points that hand a scene or the last frame's device-built lists to the host
// mirrors.  The frame constants (cand_params) and the mirrors themselves need
// no context and live in rt_cand_host.cpp.
#include "rt_ctx.h"

extern "C" int rt_cand_refine_sample(const rt_scene* scene, float eps_ulps, double bound_scale, unsigned stride,
                                     int compat, unsigned* out, size_t cap, size_t* n, size_t* total) {
  if (!scene || (!out && cap) || !n || !total) return rt_set_error(RT_EINVAL, "null argument");
  rt_frame f;
  rt_camera cam = scene->camera;
  if (compat) {  // gpu/rt's frame: the camera's width and height times 3 (gpu/rt.cpp:72-83)
    cam.width *= 3;
    cam.height *= 3;
  }
  int rc = compat ? rt_frame_from_camera_any(&cam, &f) : rt_frame_from_camera(&cam, &f);
  if (rc) return rc;
  rt_flat_scene fs;
  rc = rt_flatten(scene, RT_ACCEL_FLAT, &fs);
  if (rc) return rc;
  float sc[3], sr;
  scene_extent(fs, sc, &sr);  // as rt_hip_create
  CandParams cp;
  rc = cand_params(&f, sc, sr, eps_ulps, bound_scale, 0, 1, &cp, compat ? 1 : 0);
  if (!rc) {
    cp.nprim = (uint32_t)fs.ntri;
    *n = rt_cand_refine_sample_host(&cp, fs.tri, stride, out, cap, total);
  }
  rt_flat_free(&fs);
  return rc;
}

extern "C" int rt_cand_survey(const rt_scene* scene, float eps_ulps, double bound_scale, int threads,
                              int use_leaves, unsigned long long out[88]) {
  if (!scene || !out) return rt_set_error(RT_EINVAL, "null argument");
  rt_frame f;
  int rc = rt_frame_from_camera(&scene->camera, &f);
  if (rc) return rc;
  rt_flat_scene fs;
  rc = rt_flatten(scene, RT_ACCEL_FLAT, &fs);
  if (rc) return rc;
  float sc[3], sr;
  scene_extent(fs, sc, &sr);  // as rt_hip_create
  CandParams cp;
  rc = cand_params(&f, sc, sr, eps_ulps, bound_scale, 0, 1, &cp);
  rt_flat_scene ft;  // the host octree's leaves (use_leaves)
  std::memset(&ft, 0, sizeof ft);
  std::vector<uint32_t> pl;
  if (!rc && use_leaves) {
    rc = rt_flatten(scene, RT_ACCEL_OCTREE, &ft);
    if (!rc) {
      pl.assign(fs.ntri + 1, 0);
      for (size_t ni = 0; ni < ft.nnode; ni++) {
        uint32_t first, info;
        std::memcpy(&first, &ft.node[RT_NODE_FLOATS * ni + 3], 4);
        std::memcpy(&info, &ft.node[RT_NODE_FLOATS * ni + 7], 4);
        if (!(info & RT_NODE_LEAF)) continue;
        for (uint32_t k = 0; k < RT_LEAF_COUNT(info); k++) {
          uint32_t prim;
          std::memcpy(&prim, &ft.tri[RT_TRI_FLOATS * (size_t)(first + k) + 9], 4);
          pl[prim] = (uint32_t)ni;
        }
      }
    }
  }
  if (!rc) {
    cp.nprim = (uint32_t)fs.ntri;
    if (rt_cand_survey_host(&cp, fs.tri, use_leaves ? ft.node : nullptr,
                            use_leaves ? pl.data() : nullptr, threads, out))
      rc = rt_set_error(RT_EINVAL, "candidate survey: per-row tile count != rasterised tiles");
  }
  if (use_leaves) rt_flat_free(&ft);
  rt_flat_free(&fs);
  return rc;
}


static int cand_verify(rt_hip_ctx* c, const rt_frame* f, KParams kp, int compat, unsigned long long out[7]);

extern "C" int rt_hip_cand_verify(rt_hip_ctx* c, const rt_frame* f, int rank, int nranks,
                                  unsigned long long out[7]) {
  if (!c || !f || !out) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (!c->d_cand_start || !c->d_cand || !c->d_cand_list)
    return rt_set_error(RT_EINVAL, "no candidate lists (render a frame with exact camera rays first)");
  if (c->last_p.rank != rank || c->last_p.nranks != nranks)
    return rt_set_error(RT_EINVAL, "the last render was rank %d of %d", c->last_p.rank, c->last_p.nranks);
  return cand_verify(c, f, c->last_p, 0, out);
}

// The same for the compatibility mode's lists (rt_hip_render_compat): the
// camera's 3x frame, one sample per pixel (CandParams::compat), one rank.
extern "C" int rt_hip_cand_verify_compat(rt_hip_ctx* c, const rt_camera* cam, unsigned long long out[7]) {
  if (!c || !cam || !out) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (!c->d_cand_start || !c->d_cand || !c->d_cand_list)
    return rt_set_error(RT_EINVAL, "no candidate lists (render a frame with exact camera rays first)");
  rt_camera big = *cam;
  big.width = 3 * cam->width;
  big.height = 3 * cam->height;
  rt_frame f;
  int rc = rt_frame_from_camera_any(&big, &f);
  if (rc) return rc;
  KParams kp;
  std::memset(&kp, 0, sizeof kp);
  kp.rank = 0;
  kp.nranks = 1;
  kp.ntiles_local = tiles_x_of(big.width) * tiles_y_of(big.height);
  return cand_verify(c, &f, kp, 1, out);
}

static int cand_verify(rt_hip_ctx* c, const rt_frame* f, KParams kp, int compat, unsigned long long out[7]) {
  const int rank = kp.rank, nranks = kp.nranks;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->last_stream ? c->last_stream : c->stream;
  HIP_TRY(hipStreamSynchronize(s));
  // the render keeps only the big footprints: build the frame's lists again
  // (deterministic: the same entries at the same places) keeping every one
  {
    c->cand_store_fp = 1;
    const int rp = cand_prepare(c, f, &kp, s, compat);
    c->cand_store_fp = 0;
    if (rp) return rp;
    HIP_TRY(hipStreamSynchronize(s));
  }
  CandParams cp;
  int rc = cand_params(f, c->scene_c, c->scene_r, c->cam_eps_ulps, c->bound_scale, rank, nranks, &cp, compat);
  if (rc) return rc;
  cp.nprim = c->nprim;
  const uint32_t nt = (uint32_t)cp.ntiles_local;
  cp.refine = c->cand_refine ? 1u : 0u;
  cp.drop_key = nt;
  uint32_t nlist = 0;
  HIP_TRY(hipMemcpy(&nlist, c->d_cand_ctr + RT_CC_LIST, sizeof nlist, hipMemcpyDeviceToHost));
  std::vector<uint32_t> start(nt + 1), list(nlist + 1), pl;
  HIP_TRY(hipMemcpy(start.data(), c->d_cand_start, (nt + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<uint32_t> cand(start[nt] + 1);
  if (start[nt])
    HIP_TRY(hipMemcpy(cand.data(), c->d_cand, start[nt] * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (nlist) HIP_TRY(hipMemcpy(list.data(), c->d_cand_list, nlist * sizeof(uint32_t), hipMemcpyDeviceToHost));
  const size_t fpb = rt_cand_footprint_bytes();
  std::vector<unsigned char> fp((size_t)nlist * fpb + 1);
  if (nlist) HIP_TRY(hipMemcpy(fp.data(), c->d_cand_fp, (size_t)nlist * fpb, hipMemcpyDeviceToHost));
  std::vector<float> tri((size_t)c->nprim * RT_TRI_FLOATS + 1), node;
  HIP_TRY(hipMemcpy(tri.data(), c->d_tri_prim, (size_t)c->nprim * RT_TRI_FLOATS * sizeof(float),
                    hipMemcpyDeviceToHost));
  if (c->d_prim_leaf) {
    pl.resize(c->nprim + 1);
    HIP_TRY(hipMemcpy(pl.data(), c->d_prim_leaf, c->nprim * sizeof(uint32_t), hipMemcpyDeviceToHost));
    node.resize((size_t)c->info.nodes * RT_NODE_FLOATS + 1);
    HIP_TRY(hipMemcpy(node.data(), c->d_node, (size_t)c->info.nodes * RT_NODE_FLOATS * sizeof(float),
                      hipMemcpyDeviceToHost));
  }
  rt_cand_verify_host(&cp, tri.data(), c->d_prim_leaf ? node.data() : nullptr,
                      c->d_prim_leaf ? pl.data() : nullptr, list.data(), nlist, fp.data(),
                      start.data(), cand.data(), nt, out);
  return RT_OK;
}

extern "C" int rt_hip_cand_tile_entries(rt_hip_ctx* c, unsigned int* out, size_t n) {
  if (!c || !out) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (!c->d_cand_start) return rt_set_error(RT_EINVAL, "no candidate lists (render a frame first)");
  if (n > (size_t)c->last_p.ntiles_local)
    return rt_set_error(RT_EINVAL, "%zu tiles asked, the last render had %d", n, c->last_p.ntiles_local);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->last_stream ? c->last_stream : c->stream;
  HIP_TRY(hipStreamSynchronize(s));
  std::vector<uint32_t> st(n + 1);
  HIP_TRY(hipMemcpy(st.data(), c->d_cand_start, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  for (size_t t = 0; t < n; t++) out[t] = st[t + 1] - st[t];
  return RT_OK;
}

// ---------------------------------------------------- exact camera rays
// The builds of the candidate lists (launchers: csrc/rt_cand.h): count ->
// scan -> (one small read-back for the list sizes) -> fill.
// the headroom of the lists' entry and offset buffers (rt_mem.h half_more)
static size_t list_room(size_t need) { return half_more(need, 8192); }

// big footprints whose per-lane row counts big_count_kernel keeps for
// big_kernel (C5: ~5e4 per frame; beyond this big_kernel recounts)
static constexpr uint32_t kBigLaneCap = 1u << 17;
// (big footprint, chunk) work items of the entry-parallel big emission (C5:
// ~5e4 per frame; beyond this the frame's big footprints go to big_kernel)
#ifndef RT_CAND_ITEM_CAP
#define RT_CAND_ITEM_CAP (1u << 20)
#endif
static constexpr uint32_t kItemCap = RT_CAND_ITEM_CAP;
// (The lists' two prim-length scans are the device-length scan of rt_scan.h:
// the classification's over the listed prims only, no zeroing pass.  rocPRIM's
// scan over every prim with a separate scatter launch was removed.)

extern "C" int rt_hip_set_cand_item_cap(rt_hip_ctx* c, unsigned cap) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->cand_item_cap = cap;
  lists_changed(c);  // the lists change
  return RT_OK;
}

// the trace's item-clock sum in the frame counters (KParams::cost_sum)
unsigned long long* cost_sum_of(rt_hip_ctx* c) {
  return (unsigned long long*)((char*)c->d_counter.get() + kItemCounterBytes + kStatBytes + kHitCounterBytes);
}

// The last render's kept-entry count (rt_hip_stats reads it) outlives a list
// build that overwrites the offsets it points into: saved in stream order to
// a word no build writes (d_cand_ctr[RT_CAND_CTR_SAVED_VALID]).
static int save_valid(rt_hip_ctx* c, hipStream_t s) {
  if (!c->d_cand_valid || !c->d_cand_ctr) return RT_OK;
  uint32_t* const saved = c->d_cand_ctr + RT_CAND_CTR_SAVED_VALID;
  if (c->d_cand_valid == saved) return RT_OK;
  HIP_TRY(hipMemcpyAsync(saved, c->d_cand_valid, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
  c->d_cand_valid = saved;
  return RT_OK;
}

// The entry buffers (keys, vals, keys2, cand) for n entries: all four or
// none (a failure leaves the later ones empty, so the next call starts over).
static int cand_entry_buffers(rt_hip_ctx* c, size_t n) {
  DevBuf<uint32_t>* const all[] = {&c->d_cand_keys, &c->d_cand_vals, &c->d_cand_keys2, &c->d_cand};
  if (std::all_of(std::begin(all), std::end(all), [&](const DevBuf<uint32_t>* b) { return b->holds(n + 1); }))
    return RT_OK;
  c->ext_ready = 0;  // consumed lists (ext) point into these
  for (DevBuf<uint32_t>* b : all) b->reset();
  HIP_TRY(c->d_cand_keys.grow(n + 1, list_room(n + 1)));
  for (DevBuf<uint32_t>* b : {&c->d_cand_vals, &c->d_cand_keys2, &c->d_cand})
    HIP_TRY(b->alloc(c->d_cand_keys.cap()));
  return RT_OK;
}

// The per-tile offsets and work-order buffers for nt tiles.
static int cand_tile_buffers(rt_hip_ctx* c, size_t nt) {
  if (!c->d_cand_start.holds(nt + 1) || !c->d_order.holds(3 * (nt + 1))) {
    c->ext_ready = 0;  // the consumed lists' offsets and work order live here
    if (c->d_cand_valid && c->d_cand_valid != c->d_cand_ctr + RT_CAND_CTR_SAVED_VALID) c->d_cand_valid = nullptr;
  }
  HIP_TRY(c->d_cand_start.grow(nt + 1, list_room(nt + 1)));
  HIP_TRY(c->d_order.grow(3 * (nt + 1), 3 * (nt + 1)));
  return RT_OK;
}

// The longest-first work order of the nt tiles from their offsets, and the
// lists' kernel parameters common to both builds.
static int cand_order(rt_hip_ctx* c, KParams* kp, size_t nt, hipStream_t s, const rt_frame* f, int rank,
                      int nranks) {
  // the item clocks of this frame's last trace on this context (its counters
  // are zeroed only by the render that follows this order)
  // -- or of the last frame of the same size and rank split: a new camera
  // (an animation's next frame) moves the costly tiles little, and the order
  // is a schedule only (any order renders the same image)
  const bool hist = c->cost_hist.same_grid(f, rank, nranks) && c->d_item_cost.holds(4 * nt);
  const uint32_t* ic = hist ? c->d_item_cost : nullptr;
  const unsigned long long* cs = hist ? cost_sum_of(c) : nullptr;
  const auto order = [&](void* tmp, size_t* tb) {
    return rt_cand_order(c->d_cand_start, (uint32_t)nt, c->d_order, c->d_order + nt + 1,
                         c->d_order + 2 * (nt + 1), ic, cs, c->cost_waves, tmp, tb, s);
  };
  HIP_TRY(with_tmp(c->d_scan_tmp, order));
  kp->tile_order = c->d_order + 2 * (nt + 1);
  kp->n_heavy = c->d_order + (nt + 1) + nt;  // the scan of the heavy flags: its total
  kp->cand_start = c->d_cand_start;
  kp->tri_prim = c->d_tri_prim;
  return RT_OK;
}

// Radix sort bits of keys below n_keys.
static int key_bits(size_t n_keys) {
  int bits = 1;
  while ((1ull << bits) < n_keys) bits++;
  return bits;
}

// Passes 0-2 of the lists of cp (the prims [cp.prim0, cp.prim1)): the
// unsorted (tile, prim) entries in d_cand_keys / d_cand_vals, each listed
// prim's depth-skip bound in d_cand_skip and the global prims in
// d_cand_global; count -> scan -> (read back the entry total: the build's
// only host sync) -> emit.  The entry buffers are sized for total +
// glob_copies x globals (the triangle-parallel build routes each global to
// every rank).  No contended atomics; deterministic.
// Entries per big emission item for a build of 1/split of a frame's work (a
// rank's lists of an N-rank frame, a producer's slice of N): 1024 for a whole
// frame, halved per doubling of split down to 128, so the items stay many
// enough to overlap (rt_cand_passes.h).  RT_CAND_CHUNK_SHIFT: A/B knob.
static uint32_t cand_chunk_shift(uint32_t split) {
  if (const char* e = std::getenv("RT_CAND_CHUNK_SHIFT")) {
    const int v = std::atoi(e);
    if (v >= 6 && v <= 14) return (uint32_t)v;
  }
  uint32_t sh = 10;
  for (uint32_t q = split; q > 1 && sh > 7; q >>= 1) sh--;
  return sh;
}

// The buffers every build of a scene uses, with their sizes: fn(buffer, n)
// for each until one returns false.  They exist together: a partial set left
// by a failure is freed, never allocated over.
template <class Fn>
static bool cand_scene_buffers(rt_hip_ctx* c, Fn&& fn) {
  const size_t np1 = (size_t)c->nprim + 1, nw = (size_t)rt_cand_big_waves() + 1;
  return fn(c->d_cand_list, np1) && fn(c->d_cand_fp, np1 * rt_cand_footprint_bytes()) &&
         fn(c->d_cand_sfp, 2 * np1) && fn(c->d_cand_visits, np1) && fn(c->d_cand_off, np1) &&
         fn(c->d_cand_global, np1) && fn(c->d_cand_big, np1) && fn(c->d_cand_ctr, RT_CAND_CTR_BLOCK) &&
         fn(c->d_cand_skip, np1) && fn(c->d_cand_big_lane, (size_t)kBigLaneCap * 64) &&
         fn(c->d_cand_items, (size_t)kItemCap + 1) && fn(c->d_cand_wave_items, nw) &&
         fn(c->d_cand_wave_base, nw) && fn(c->d_scan_bsum, (size_t)rt_cand_scan_dev_tiles(c->nprim));
}

static int cand_build(rt_hip_ctx* c, CandParams& cp, hipStream_t s, uint32_t glob_copies, uint32_t* total_out,
                      uint32_t* nglobal_out, const ListShape* known = nullptr, ListShape* shape = nullptr) {
  int rc = RT_OK;
  // every build overwrites the entry, offset and order buffers: lists that
  // rt_hip_cand_consume left for a render (ext) are gone from here on, so
  // that render builds its own (produce -> consume -> produce ->
  // render must not render from clobbered buffers)
  c->ext_ready = 0;
  rc = save_valid(c, s);
  if (rc) return rc;
  cp.tri = c->d_tri_prim;
  cp.nprim = c->nprim;
  const size_t np = c->nprim;
  if (!c->d_prim_leaf && c->d_node) {  // once per scene: which leaf holds each prim
    HIP_TRY(c->d_prim_leaf.alloc(np + 1));
    HIP_TRY(hipMemsetAsync(c->d_prim_leaf, 0xff, (np + 1) * sizeof(uint32_t), s));  // atomicMin's start
    HIP_TRY(rt_cand_prim_leaf(c->d_node, (uint32_t)c->info.nodes, c->d_tri, c->d_prim_leaf, s));
  }
  cp.node = c->d_node;
  cp.prim_leaf = c->d_prim_leaf;
  if (!cand_scene_buffers(c, [](auto& b, size_t n) { return b.holds(n); }) || !c->h_cand.holds(RT_CC_BUILD_WORDS)) {
    cand_scene_buffers(c, [](auto& b, size_t) { return b.reset(), true; });
    hipError_t he = hipSuccess;
    cand_scene_buffers(c, [&](auto& b, size_t n) { return (he = b.alloc(n)) == hipSuccess; });
    HIP_TRY(he);
    HIP_TRY(hipMemset(c->d_cand_wave_items, 0, c->d_cand_wave_items.cap() * sizeof(uint32_t)));  // [last] stays 0
    HIP_TRY(c->h_cand.grow(RT_CC_BUILD_WORDS, RT_CC_BUILD_WORDS));
  }
  cp.list = c->d_cand_list;
  cp.fp = (rtc::Footprint*)c->d_cand_fp.get();
  // compact small footprints while tile columns fit their 16-bit intervals
  cp.sfp = cp.tiles_x < 32767 ? c->d_cand_sfp : nullptr;
  cp.store_fp = (c->cand_store_fp || !cp.sfp) ? 1u : 0u;
  cp.visits = c->d_cand_visits;
  cp.off = c->d_cand_off;
  cp.global = c->d_cand_global;
  cp.big = c->d_cand_big;
  cp.ctr = c->d_cand_ctr;
  cp.skip = c->d_cand_skip;
  cp.big_lane = c->d_cand_big_lane;
  cp.big_cap = kBigLaneCap;
  cp.items = c->d_cand_items;
  cp.item_cap = c->cand_item_cap < kItemCap ? c->cand_item_cap : kItemCap;
  cp.chunk_shift = cand_chunk_shift(glob_copies ? glob_copies : (uint32_t)cp.nranks);
  cp.wave_items = c->d_cand_wave_items;
  cp.wave_base = c->d_cand_wave_base;
  cp.refine = c->cand_refine ? 1u : 0u;
  cp.drop_key = (uint32_t)cp.ntiles_local;  // sorts after the tiles (their keys are < ntiles_local)
  // (the build's counters and visits[np] are zeroed by quick_kernel)
  // (temporary storage for both scans, before the launches)
  const auto prim_scan = [&](void* tmp, size_t* tb) {
    return rt_cand_scan(c->d_cand_visits, c->d_cand_off, (uint32_t)np, tmp, tb, s);
  };
  HIP_TRY(with_tmp(c->d_scan_tmp, prim_scan, false));
  const auto wave_scan = [&](void* tmp, size_t* tb) {
    return rt_cand_scan(c->d_cand_wave_items, c->d_cand_wave_base, rt_cand_big_waves(), tmp, tb, s);
  };
  HIP_TRY(with_tmp(c->d_scan_tmp, wave_scan, false));
  // pass 0: flags -> compact list of the prims the float fast path leaves
  // (over this build's slice of the prims only)
  if (cp.prim1 > cp.nprim || cp.prim0 > cp.prim1) return rt_set_error(RT_EINVAL, "prim slice");
  HIP_TRY(rt_cand_quick(&cp, s));
  HIP_TRY(rt_cand_scan_scatter(&cp, c->d_scan_bsum, s));
  // pass 1: footprints and tile counts of the listed prims
  HIP_TRY(rt_cand_count(&cp, s));
  HIP_TRY(rt_cand_big_count(&cp, s));
  // the big footprints' emission items (a scan over the big_count waves)
  size_t tb = c->d_scan_tmp.cap();
  HIP_TRY(wave_scan(c->d_scan_tmp, &tb));
  HIP_TRY(rt_cand_items(&cp, s));
  // over the list's length only (on the device); the entry total -> its counter
  HIP_TRY(rt_cand_scan_dev(c->d_cand_visits, c->d_cand_off, (uint32_t)np, c->d_cand_ctr + RT_CC_LIST,
                           c->d_cand_ctr + RT_CC_TOTAL, c->d_scan_bsum, s));
  if (known) {
    // no read-back: the frame's lists were built before with a read-back of
    // their sizes (deterministic for the same frame), so the buffers hold
    // them; an entry past known->total would not be written and would set
    // ctr[RT_CC_OVERFLOW] (rt_hip_stats then reports the frame, rt_hip_cand_produce
    // builds again: never silent).  The emission kernels read the item
    // count and the over-cap flag on the device and the render reads the
    // global prims' count there
    rc = cand_entry_buffers(c, (size_t)known->total + (size_t)glob_copies * known->nglobal);
    if (rc) return rc;
    cp.keys = c->d_cand_keys;
    cp.vals = c->d_cand_vals;
    cp.key_cap = known->total;
    HIP_TRY(rt_cand_emit(&cp, s));
    // the same launch shape as the read-back build (the kernels read the
    // counts on the device and loop over whatever they find)
    if (known->over)
      HIP_TRY(rt_cand_big(&cp, known->nbig, s));
    else
      HIP_TRY(rt_cand_big_items(&cp, known->nitems, 1, s));
    // (entries past the build's own total, ctr[RT_CC_TOTAL] -- never expected -- are
    // left to the caller: cand_prepare drops them before the sort, a
    // produce's partition routes them as dropped; and cand_prepare's
    // bounds_kernel snapshots the counters for rt_hip_stats)
    *total_out = known->total;  // the sort's length
    *nglobal_out = known->nglobal;  // (the render reads the count on the device, ctr[RT_CC_GLOBAL])
    return RT_OK;
  }
  // one read-back of the build's sizes
  HIP_TRY(hipMemcpyAsync(c->h_cand, c->d_cand_ctr, RT_CC_BUILD_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint32_t total = c->h_cand[RT_CC_TOTAL], nglobal = c->h_cand[RT_CC_GLOBAL], nbig = c->h_cand[RT_CC_BIG];
  const uint32_t nitems = c->h_cand[RT_CC_ITEMS], items_over = c->h_cand[RT_CC_ITEMS_OVER];
  rc = cand_entry_buffers(c, (size_t)total + (size_t)glob_copies * nglobal);
  if (rc) return rc;
  cp.key_cap = 0;
  cp.keys = c->d_cand_keys;
  cp.vals = c->d_cand_vals;
  HIP_TRY(rt_cand_emit(&cp, s));
  if (items_over)
    HIP_TRY(rt_cand_big(&cp, nbig, s));
  else
    HIP_TRY(rt_cand_big_items(&cp, nitems, 0, s));
  if (shape) shape->set_sizes(c->h_cand);
  *total_out = total;
  *nglobal_out = nglobal;
  return RT_OK;
}

// Sorts n (key < n_keys, value) pairs keys/vals -> keys2/vals2 on the key
// bits from begin_bit up (rocPRIM radix sort, stable, temporary storage in
// d_scan_tmp).
static int cand_sort(rt_hip_ctx* c, uint32_t* keys, uint32_t* keys2, uint32_t* vals, uint32_t* vals2, uint32_t n,
                     size_t n_keys, hipStream_t s, int begin_bit = 0) {
  const int bits = key_bits(n_keys);
  const auto sort = [&](void* tmp, size_t* tb) {
    return rt_cand_sort(keys, keys2, vals, vals2, n, begin_bit, bits, tmp, tb, s);
  };
  HIP_TRY(with_tmp(c->d_scan_tmp, sort, n != 0));
  return RT_OK;
}

// This rank's lists, built on this rank: cand_build for the rank's tiles
// (every prim) -> radix sort by tile -> per-tile offsets -> per-entry skip
// bounds -> work order.
// A build of plan's shape for nt tiles allocates and frees nothing: every
// buffer cand_build and cand_prepare size up front holds already (the
// scans' temporaries and the partition counts grow by themselves, behind a
// device-wide wait).
static bool cand_buffers_fit(rt_hip_ctx* c, const ListPlan& plan, size_t nt) {
  const size_t n = (size_t)plan.shape.total + 1;
  return cand_scene_buffers(c, [](auto& b, size_t need) { return b.holds(need); }) &&
         c->h_cand.holds(RT_CC_BUILD_WORDS) && (c->d_prim_leaf || !c->d_node) && c->d_cand_keys.holds(n) &&
         c->d_cand_vals.holds(n) && c->d_cand_keys2.holds(n) && c->d_cand.holds(n) &&
         c->d_cand_start.holds(nt + 1) && c->d_order.holds(3 * (nt + 1));
}

// Ends a side-stream build that did not reach its join (an error return in
// the middle of cand_prepare): nothing stays in flight there.
struct SideBuild {
  rt_hip_ctx* c;
  bool open = false;
  ~SideBuild() {
    if (!open) return;
    (void)hipStreamSynchronize(c->side_stream);
    c->overlap.joined();
    c->overlap.lists_touched();
  }
};

int cand_prepare(rt_hip_ctx* c, const rt_frame* f, KParams* kp, hipStream_t cs, int compat, bool from_render) {
  hipStream_t s = cs;  // the build's stream: the caller's, or the context's side stream (csrc/rt_overlap.h)
  CandParams cp;
  int rc = cand_params(f, c->scene_c, c->scene_r, c->cam_eps_ulps, c->bound_scale, kp->rank, kp->nranks,
                       &cp, compat);
  if (rc) return rc;
  cp.prim0 = 0;
  cp.prim1 = c->nprim;
  const size_t nt = (size_t)kp->ntiles_local;
  uint32_t total = 0, nglobal = 0;
  ListForecast& fc = c->forecast;
  const int rank = kp->rank, nranks = kp->nranks;
  // the last estimated-shape build's counters, once their read-back is done
  const auto arrived = [&] { return c->ev_kept && hipEventQuery(c->ev_kept) == hipSuccess; };
  if (fc.snap_pending && arrived()) fc.absorb_snapshot(c->h_kept + RT_KEPT_CTR);
  const ListPlan plan = fc.plan(f, rank, nranks, c->async_lists, c->cand_store_fp, compat);
  const bool async = plan.async;
  ListOverlap& ov = c->overlap;
  SideBuild side{c};
  if (ov.side(from_render, async, compat != 0, cand_buffers_fit(c, plan, nt)) && c->side_stream.s &&
      c->ev_lists_free && c->ev_lists_done) {
    s = c->side_stream;
    HIP_TRY(hipStreamWaitEvent(s, c->ev_lists_free, 0));
    side.open = true;
    ov.forked();
    if (c->timing) {  // the lists' own span, on their stream
      HIP_TRY(hipEventRecord(c->ev[c->frames % RT_TIMED_FRAMES][0], s));
      c->ev_side[c->frames % RT_TIMED_FRAMES] = 1;
    }
  } else if (!from_render) {
    ov.lists_touched();
  }
  ListShape built;
  rc = cand_build(c, cp, s, 0, &total, &nglobal, async ? &plan.shape : nullptr, async ? nullptr : &built);
  if (rc) return rc;
  c->last_async = async ? 1 : 0;
  if (async)
    nglobal = 0;  // on the device (ctr[RT_CC_GLOBAL])
  else
    fc.record_build(built, f, rank, nranks, compat);
  rc = cand_tile_buffers(c, nt);
  if (rc) return rc;
  // the kept count of the last build of this size and split, once its
  // read-back is done
  if (fc.kept_pending && arrived()) fc.absorb_kept(c->h_kept[RT_KEPT_COUNT]);
  const ListCompaction compact = fc.compaction(plan, f, rank, nranks, total, c->cand_refine, c->cand_store_fp, compat);
  bool kept_now = false;
  if (compact) {
    // the kept entries (stable) -> keys2 / d_cand, sorted back into keys /
    // vals, and the buffer pairs swapped so that the sorted ones are where
    // the uncompacted path leaves them
    const uint32_t nw = rt_cand_part_waves(total);
    HIP_TRY(c->d_part.grow((size_t)2 * nw + 4, 2 * ((size_t)nw + nw / 2) + 1024));  // headroom (as list_room)
    uint32_t* cnt = c->d_part;
    uint32_t* off = c->d_part + nw + 1;
    const auto compaction = [&](void* tmp, size_t* tb) {
      return rt_cand_compact(c->d_cand_keys, c->d_cand_vals, total, c->d_cand_ctr + RT_CC_TOTAL, (uint32_t)nt,
                             compact.cap, cnt, off, tmp, tb, c->d_cand_keys2, c->d_cand,
                             c->d_cand_ctr + RT_CC_OVERFLOW, s);
    };
    HIP_TRY(with_tmp(c->d_scan_tmp, compaction));
    uint32_t kept = compact.cap;
    if (compact.fresh) {  // off[nw] = the kept entries
      HIP_TRY(c->h_kept.grow(RT_KEPT_WORDS, RT_KEPT_WORDS));
      HIP_TRY(hipMemcpyAsync(c->h_kept + RT_KEPT_COUNT, off + nw, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      kept = c->h_kept[RT_KEPT_COUNT];
      if (kept > total) return rt_set_error(RT_EHIP, "compaction kept %u of %u entries", kept, total);
      fc.record_kept(kept, f, rank, nranks);
      kept_now = true;
    }
    rc = cand_sort(c, c->d_cand_keys2, c->d_cand_keys, c->d_cand, c->d_cand_vals, kept, nt + 1, s);
    if (rc) return rc;
    swap(c->d_cand_keys, c->d_cand_keys2);
    swap(c->d_cand_vals, c->d_cand);
    total = kept;
  } else {
    // an asynchronous build's entries past its own total (never expected): dropped
    if (async) HIP_TRY(rt_cand_fill_tail(c->d_cand_keys, c->d_cand_ctr + RT_CC_TOTAL, total, (uint32_t)nt, s));
    // keys are tiles < nt, or nt for an entry the refinement dropped: nt + 1 keys
    rc = cand_sort(c, c->d_cand_keys, c->d_cand_keys2, c->d_cand_vals, c->d_cand, total, nt + 1, s);
    if (rc) return rc;
  }
  // start[nt] = the entries with a tile (the dropped ones sort after them)
  // (an asynchronous build's counters snapshot for rt_hip_stats, where no build writes)
  HIP_TRY(rt_cand_bounds(c->d_cand_keys2, total, c->d_cand_start, (uint32_t)nt, async ? c->d_cand_ctr : nullptr, s));
  if (fc.wants_late_readback(plan, f, rank, nranks, c->cand_refine, compat, kept_now)) {
    HIP_TRY(c->h_kept.grow(RT_KEPT_WORDS, RT_KEPT_WORDS));
    if (!c->ev_kept) HIP_TRY(hipEventCreateWithFlags(&c->ev_kept, hipEventDisableTiming));
    HIP_TRY(hipMemcpyAsync(c->h_kept + RT_KEPT_COUNT, c->d_cand_start + nt, sizeof(uint32_t), hipMemcpyDeviceToHost,
                           s));
    if (plan.estimated)  // bounds_kernel's snapshot of its counters
      HIP_TRY(hipMemcpyAsync(c->h_kept + RT_KEPT_CTR, c->d_cand_ctr + RT_CAND_CTR_SNAPSHOT,
                             RT_CC_BUILD_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(c->ev_kept, s));
    fc.late_readback_requested(plan, f, rank, nranks);
  }
  // the sorted keys are spent: their buffer takes the per-entry skip bounds
  float* entry_skip = (float*)c->d_cand_keys2.get();
  HIP_TRY(rt_cand_entry_skip(c->d_cand, c->d_cand_skip, entry_skip, total, c->d_cand_start + nt, s));
  // longest-first work order of the rank's tiles (heavy lists first)
  rc = cand_order(c, kp, nt, s, f, rank, nranks);
  if (rc) return rc;
  kp->cand = c->d_cand;
  kp->cand_global = c->d_cand_global;
  kp->n_cand_global = nglobal;
  kp->n_cand_global_dev = async ? c->d_cand_ctr + RT_CC_GLOBAL : nullptr;
  kp->cand_skip = entry_skip;
  c->cand_entries = total;  // until rt_hip_stats reads start[nt]
  c->d_cand_valid = (c->cand_refine || async) ? c->d_cand_start + nt : nullptr;
  c->cand_global = nglobal;
  c->cand_prims = 0;  // not counted separately (entries and globals are)
  // the build's overflow flag for its frame's fold (bounds_kernel's snapshot
  // of the counters): with the overlap on, in a word the next build -- which
  // may run beside that fold -- does not write
  c->list_flag = async ? c->d_cand_ctr + RT_CAND_CTR_SNAPSHOT + RT_CC_OVERFLOW : nullptr;
  if (async && ov.enabled && !compat) {
    if (!c->d_list_flag) HIP_TRY(c->d_list_flag.alloc(2));
    uint32_t* const word = c->d_list_flag + ov.flag_slot();
    HIP_TRY(hipMemcpyAsync(word, c->list_flag, sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    c->list_flag = word;
  }
  if (side.open) {  // the join: the caller's stream goes on behind the build
    if (c->timing) HIP_TRY(hipEventRecord(c->ev[c->frames % RT_TIMED_FRAMES][5], s));
    HIP_TRY(hipEventRecord(c->ev_lists_done, s));
    HIP_TRY(hipStreamWaitEvent(cs, c->ev_lists_done, 0));
    side.open = false;
    ov.joined();
  }
  return RT_OK;
}

// Triangle-parallel lists of an N-rank frame:
// rank r builds the whole frame's entries of prims [r P / N, (r + 1) P / N)
// -- the float fast path, classification and emission each run once per
// prim over the N GPUs instead of once per prim on every GPU -- and routes
// them to the ranks owning their tiles; one all-to-all exchange gives each
// rank its own lists (rt_hip_cand_consume).
extern "C" int rt_hip_cand_produce(rt_hip_ctx* c, const rt_frame* f, int rank, int nranks, unsigned* counts,
                                   unsigned* nglobal_out, void* stream) {
  if (!c || !f || !counts || !nglobal_out) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (nranks <= 0 || rank < 0 || rank >= nranks) return rt_set_error(RT_EINVAL, "rank %d of %d", rank, nranks);
  if (c->accel != RT_ACCEL_OCTREE || !c->d_node || !c->exact_camera)
    return rt_set_error(RT_EINVAL, "no camera candidate lists in this configuration (octree, exact camera rays)");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  c->overlap.lists_touched();
  CandParams cp;
  int rc = cand_params(f, c->scene_c, c->scene_r, c->cam_eps_ulps, c->bound_scale, 0, 1, &cp, 0);
  if (rc) return rc;
  const uint64_t np = c->nprim;
  // this producer's slice: the blocks of RT_SLICE_BLOCK prims b = rank mod
  // nranks (prims near each other in the scene -- one sphere, one region --
  // are near each other in prim order: contiguous slices loaded the producer
  // of the nearest objects ~20 % above the mean on C5, blocks spread it)
  const uint64_t nb = (np + RT_SLICE_BLOCK - 1) / RT_SLICE_BLOCK;
  uint64_t len = 0;
  for (uint64_t b = (uint64_t)rank; b < nb; b += (uint64_t)nranks)
    len += std::min<uint64_t>(RT_SLICE_BLOCK, np - b * RT_SLICE_BLOCK);
  cp.prim0 = 0;
  cp.prim1 = (uint32_t)len;
  cp.sl_stride = (uint32_t)nranks;
  cp.sl_rank = (uint32_t)rank;
  // a slice produced before for this frame is built without the mid-build
  // read-back (its sizes are deterministic); the read-back of the counts at
  // the end checks them, and a mismatch -- never expected -- builds again
  const bool async = c->async_lists && !c->cand_store_fp && c->pknown.same(f, rank, nranks);
  uint32_t total = 0, nglobal = 0;
  rc = cand_build(c, cp, s, (uint32_t)nranks, &total, &nglobal, async ? &c->pknown : nullptr,
                  async ? nullptr : &c->pknown);
  if (rc) return rc;
  if (!async) c->pknown.set(f, rank, nranks);
  const uint32_t tpr = (uint32_t)rt_hip_tiles_per_rank(f->width, f->height, nranks);
  const int tb = rt_block_side(nranks);
  // key = rank << tbits | local tile (tpr: a global), rank nranks for an
  // entry the refinement dropped (or, in an asynchronous build, past the
  // build's own total); then a stable partition by rank.  The consumer's
  // stable sort by tile gives each tile the same entries as the rank's own
  // build -- in the producers' interleaved slice order, not necessarily the
  // same order within a tile, which the render does not depend on (the
  // winner is the lexicographic (new_dist, prim) minimum, rt_isect.h
  // consider_exact)
  const int tbits = key_bits((size_t)tpr + 1);
  if (nranks > 256 || tbits + key_bits((size_t)nranks + 1) > 32)
    return rt_set_error(RT_EINVAL, "%d ranks x %u tiles per rank: routed keys exceed 32 bits", nranks, tpr);
  // (the entries' routing is fused into the partition's count pass)
  HIP_TRY(rt_cand_route_globals(c->d_cand_global, nglobal, nranks, tpr, (uint32_t)tbits, c->d_cand_keys + total,
                                c->d_cand_vals + total, s));
  const uint32_t n = total + nglobal * (uint32_t)nranks;
  // the starts, then the build's counters
  const size_t nstart = rt_rstart_words(nranks);
  HIP_TRY(c->d_rstart.grow(nstart, nstart));
  HIP_TRY(c->h_rstart.grow(nstart, nstart));
  HIP_TRY(c->d_send.grow(3 * (size_t)n + 1, 3 * ((size_t)n + n / 4 + 1024)));
  // per-wave rank counts (rank-major) -> exclusive scan -> stable scatter
  const size_t nh = ((size_t)nranks + 1) * rt_cand_part_waves(n);
  HIP_TRY(c->d_part.grow(2 * nh + 2, 2 * (nh + nh / 4) + 1024));
  uint32_t* hist = c->d_part;
  uint32_t* hoff = c->d_part + nh + 1;
  if (nh) {
    HIP_TRY(rt_cand_part_count(c->d_cand_keys, n, (uint32_t)tbits, nranks, hist, total, cp.tiles_x,
                               rt_blocks_x(cp.tiles_x, tb), tb, cp.drop_key,
                               async ? c->d_cand_ctr + RT_CC_TOTAL : nullptr, s));
    const auto scan = [&](void* tmp, size_t* bytes) { return rt_cand_scan(hist, hoff, (uint32_t)(nh - 1), tmp, bytes, s); };
    HIP_TRY(with_tmp(c->d_scan_tmp, scan));
  }
  HIP_TRY(rt_cand_part_scatter(c->d_cand_keys, c->d_cand_vals, c->d_cand_skip, n, (uint32_t)tbits, nranks, hoff,
                               c->d_rstart, c->d_send, c->d_cand_ctr, s));
  // the per-rank starts and the build's counters in one read-back
  HIP_TRY(hipMemcpyAsync(c->h_rstart, c->d_rstart, nstart * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint32_t* hc = c->h_rstart + rt_rstart_ctr(nranks);  // the build's counters
  if (async && !c->pknown.same_sizes(hc)) {
    c->pknown.valid = 0;  // not this slice's sizes after all: build it with the read-back
    return rt_hip_cand_produce(c, f, rank, nranks, counts, nglobal_out, stream);
  }
  for (int d = 0; d < nranks; d++) counts[d] = c->h_rstart[d + 1] - c->h_rstart[d];
  *nglobal_out = nglobal;
  c->send_n = c->h_rstart[nranks];  // the routed entries (the refinement's dropped ones sort after them)
  return RT_OK;
}

extern "C" int rt_hip_cand_send_buffer(const rt_hip_ctx* c, const void** d_entries, size_t* n) {
  if (!c || !d_entries || !n) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  *d_entries = c->d_send;
  *n = c->send_n;
  return RT_OK;
}

// This rank's lists from the entries the producers routed to it (any order
// of sources; 3 words each: rank-local tile or tpr for a global, prim, skip
// bits): sort by tile -> gather prims and skip bounds -> offsets -> work
// order.  The next rt_hip_render of (frame, rank, nranks) uses them.
extern "C" int rt_hip_cand_consume(rt_hip_ctx* c, const rt_frame* f, int rank, int nranks, const void* d_entries,
                                   size_t n, unsigned nglobal, void* stream) {
  if (!c || !f || (!d_entries && n)) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (nranks <= 0 || rank < 0 || rank >= nranks) return rt_set_error(RT_EINVAL, "rank %d of %d", rank, nranks);
  if (n >= (1ull << 31) || nglobal > n) return rt_set_error(RT_EINVAL, "%zu entries, %u globals", n, nglobal);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const size_t nt = (size_t)rank_tile_count(f->width, f->height, rank, nranks);
  const uint32_t tpr = (uint32_t)rt_hip_tiles_per_rank(f->width, f->height, nranks);
  c->ext_ready = 0;  // set again once this consume's lists are complete
  c->overlap.lists_touched();
  int rc = save_valid(c, s);
  if (rc) return rc;
  rc = cand_entry_buffers(c, n);
  if (rc) return rc;
  rc = cand_tile_buffers(c, nt);
  if (rc) return rc;
  const uint32_t* in = (const uint32_t*)d_entries;
  HIP_TRY(rt_cand_unpack(in, (uint32_t)n, (uint32_t)nt, tpr, c->d_cand_keys, c->d_cand_vals, s));
  // keys are tiles < nt, or nt for the globals: nt + 1 keys
  rc = cand_sort(c, c->d_cand_keys, c->d_cand_keys2, c->d_cand_vals, c->d_cand, (uint32_t)n, nt + 1, s);
  if (rc) return rc;
  const uint32_t total = (uint32_t)(n - nglobal);
  HIP_TRY(rt_cand_bounds(c->d_cand_keys2, total, c->d_cand_start, (uint32_t)nt, nullptr, s));
  // the spent unsorted keys take the skip bounds, the spent indices the prims
  HIP_TRY(rt_cand_gather(in, c->d_cand, (uint32_t)n, c->d_cand_vals, (float*)c->d_cand_keys.get(), s));
  KParams kp;
  std::memset(&kp, 0, sizeof kp);
  rc = cand_order(c, &kp, nt, s, f, rank, nranks);
  if (rc) return rc;
  c->ext = kp;
  c->ext.cand = c->d_cand_vals;
  c->ext.cand_skip = (const float*)c->d_cand_keys.get();
  c->ext.cand_global = c->d_cand_vals + total;
  c->ext.n_cand_global = nglobal;
  c->ext_ready = 1;
  c->ext_rank = rank;
  c->ext_nranks = nranks;
  std::memcpy(&c->ext_frame, f, sizeof *f);
  c->ext_total = total;
  return RT_OK;
}
