// rt_hip.cpp -- host side of the C ABI (include/rt_hip.h): the context's
// lifetime and settings, light buffers, the render and its stats, assemble,
// the gpu/rt compatibility mode and rt_raytrace.  Owns device memory,
// streams and launches; the scene preparation (flatten, octree) is host C
// (host/accel.c).  No CPU fallback: every entry point fails with RT_ENODEV /
// RT_EHIP when the gfx950 device or the kernels are missing.  Shared state:
// rt_ctx.h.
#include "rt_ctx.h"

extern "C" int rt_hip_tiles_per_rank(int width, int height, int nranks) {
  if (width <= 0 || height <= 0 || nranks <= 0) return 0;
  const int tb = rt_block_side(nranks);
  return (int)(rt_max_rank_blocks((uint32_t)rt_blocks_x(tiles_x_of(width), tb),
                                  (uint32_t)rt_blocks_y(tiles_y_of(height), tb), (uint32_t)nranks) * tb * tb);
}

extern "C" size_t rt_hip_tile_buffer_floats(int width, int height, int nranks) {
  return (size_t)rt_hip_tiles_per_rank(width, height, nranks) * 64 * 3;
}

extern "C" int rt_hip_device_count(int* n) {
  if (!n) return rt_set_error(RT_EINVAL, "null argument");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess || c <= 0) {
    *n = 0;
    return rt_set_error(RT_ENODEV, "no HIP device (%s)", hipGetErrorString(e));
  }
  *n = c;
  return RT_OK;
}

template <class T>
static int upload(DevBuf<T>& dst, const void* src, size_t bytes) {
  HIP_TRY(dst.alloc(bytes / sizeof(T)));
  if (src && bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return RT_OK;
}

// The shading tables (csrc/rt_shade_rows.h) of the light rows in d_light
// (lights) and / or the material rows in d_mat (materials), after an upload of
// either: allocated to the rows' count and derived on the device, finished
// when this returns (setup; a render may run on any stream).
static int shade_tables(rt_hip_ctx* c, bool lights, bool materials) {
  const uint32_t nl = lights ? c->nlight : 0u;
  const uint32_t no = materials ? (uint32_t)(c->mat_host.size() / RT_MAT_FLOATS) : 0u;
  if (lights) HIP_TRY(c->d_lshade.alloc((size_t)nl * RT_LSHADE_FLOATS_D));
  if (materials) HIP_TRY(c->d_mshade.alloc((size_t)no * RT_MAT_FLOATS));
  HIP_TRY(rt_launch_shade_tables(c->d_light, nl, c->d_lshade, c->d_mat, no, c->d_mshade, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RT_OK;
}

extern "C" void rt_hip_destroy(rt_hip_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;  // (waits for the side stream's build first: ~rt_hip_ctx)
}

extern "C" int rt_hip_set_overlap_lists(rt_hip_ctx* c, int enable) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->overlap.set_enabled(enable != 0);
  return RT_OK;
}

extern "C" int rt_hip_overlap_builds(const rt_hip_ctx* c, unsigned long long* n) {
  if (!c || !n) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  *n = c->overlap.side_builds;
  return RT_OK;
}

// Per-node slack multipliers of the shadow walk for the context's culling
// slack (csrc/rt_shadow.hip): once per scene and slack, on the context's
// stream, synchronous (setup; it reads back the global list's length).
int shadow_prepare(rt_hip_ctx* c, hipStream_t s) {
  if (!c->exact_shadows || c->accel != RT_ACCEL_OCTREE || !c->d_node) return RT_OK;
  if (c->d_node_mu && c->sh_ulps == c->eps_ulps) return RT_OK;
  const size_t np = c->nprim, nn = c->info.nodes;
  if (!c->d_node_mu) {
    HIP_TRY(c->d_prim_mu.alloc(np + 1));
    HIP_TRY(c->d_sh_global.alloc(np + 1));
    HIP_TRY(c->d_node_mu.alloc(nn + 1));
  }
  DevBuf<uint32_t> d_n;
  HIP_TRY(d_n.alloc(1));
  ShadowParams sp;
  std::memset(&sp, 0, sizeof sp);
  sp.tri = c->d_tri_prim;
  sp.nprim = c->nprim;
  sp.light = c->d_light;
  sp.nlight = c->nlight;
  sp.node = c->d_node;
  sp.nnode = (uint32_t)nn;
  sp.rec = c->d_tri;
  for (int a = 0; a < 3; a++) sp.c[a] = c->scene_c[a];
  sp.R = c->scene_r;
  // the walk computes eps(o) in float (host/rt_cull.h); the multipliers keep
  // a relative margin of 1e-6 and the +1 of the original slack on top
  sp.eps_rel = (double)(c->eps_ulps * kSlackUnit);
  const double cmag = std::fmax(std::fabs(c->scene_c[0]), std::fmax(std::fabs(c->scene_c[1]),
                                                                  std::fabs(c->scene_c[2])));
  sp.plane_eps = (double)RT_CULL_PLANE * (cmag + c->scene_r) + 1e-6;
  // point lights: shadow rays leave hit points, which lie on the scene's
  // triangles up to the float error of their hit; origins beyond twice the
  // scene's extent are counted (rt_stats.shadow_unproven), never assumed
  sp.omax_assumed = 2.0 * c->scene_r + 1.0;
  sp.reach_cap = c->scene_r + 1.0;
  sp.prim_mu = c->d_prim_mu;
  sp.node_mu = c->d_node_mu;
  sp.global = c->d_sh_global;
  sp.nglobal = d_n;
  uint32_t n = 0;
  std::vector<float2> nm(1);
  HIP_TRY(hipMemsetAsync(d_n, 0, sizeof(uint32_t), s));
  HIP_TRY(rt_shadow_build(&sp, (int)c->info.max_depth + 2, s));
  HIP_TRY(hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(nm.data(), c->d_node_mu, sizeof(float2), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  c->n_sh_global = n;
  c->sh_omax = (float)(sp.omax_assumed * (1.0 - 1e-6));
  c->sh_mu_max = nm[0].x;  // the root's: the max over the scene
  c->sh_ulps = c->eps_ulps;
  c->info.shadow_global = n;
  c->info.shadow_mu_max = nm[0].x;
  return RT_OK;
}

// Light buffers of the scene's directional and point lights for the
// context's culling slack (csrc/rt_lightbuf.hip): once per scene and slack,
// synchronous (setup).  The shadow queries of the default walk then look up
// the cells their origins project to instead of walking the octree.
static void lbuf_release(rt_hip_ctx* c) {
  for (LBDevice*& d : c->lb_dev) {
    rt_lightbuf_free(d);
    d = nullptr;
  }
  c->d_lbuf.reset();
  c->lb_ulps = -1.0f;
}

// The buffer of light li (lb_dev[li] is null, lb_host / lb_failed hold nlight
// entries) for the context's slack and mode; a light that casts no shadow has
// none.  RT_OK also when the build fell back to the walk (lb_failed[li]); an
// error is a failed launch or an inconsistent build, and the caller gives
// every buffer up.
static int lbuf_build_one(rt_hip_ctx* c, uint32_t li, hipStream_t s) {
  std::memset(&c->lb_host[li], 0, sizeof(RtLightBuf));
  c->lb_failed[li] = 0;
  const uint32_t t = c->light_type[li];
  if (t != 1 && t != 2) return RT_OK;
  char err[256] = {0};
  LBParams lp;
  lb_fill(lp, c->scene_c, c->scene_r, c->scene_lo, c->scene_hi, c->eps_ulps, t, &c->light_v[3 * li], c->nprim,
          c->exact_shadows);
  lp.tri = c->d_tri_prim;
  lp.max_entries = c->lb_entry_cap;
  if (const char* e = std::getenv("RT_LB_CELLS")) {  // build tuning: cells per triangle
    const double k = std::atof(e);
    if (k > 0.0) lp.target_cells = (uint32_t)std::fmin((double)(1u << 26), std::fmax(4096.0, lp.target_cells * k));
  }
  const int br = rt_lightbuf_build(&lp, &c->lb_host[li], &c->lb_dev[li], s, err, sizeof err);
  if (br < 0) {  // not a capacity question: a failed launch or an inconsistent build
    (void)hipGetLastError();
    return rt_set_error(RT_EHIP, "light buffer of light %u: %s", li, err);
  }
  if (br > 0) {
    // entry or cell cap, device memory, or a zero directional vector (no
    // grid): the light's queries walk the octree instead (lb_host[li] is
    // zeroed: RT_LB_NONE), as they did before light buffers -- a scene that
    // fits the walk still loads; in the exact-shadow mode that walk is the
    // proven per-node multiplier walk (shadow_prepare, built by the render)
    std::memset(&c->lb_host[li], 0, sizeof(RtLightBuf));
    c->lb_dev[li] = nullptr;
    (void)hipGetLastError();  // an out-of-memory hipMalloc is not sticky; clear it anyway
    std::snprintf(c->info.lightbuf_fail_reason, sizeof c->info.lightbuf_fail_reason, "light %u: %s", li, err);
    c->lb_failed[li] = 1;
  }
  return RT_OK;
}

// The per-light table on the device and rt_accel_info's totals, from lb_host /
// lb_dev / lb_failed as they stand.
static int lbuf_publish(rt_hip_ctx* c) {
  uint32_t failed = 0;
  for (uint8_t f : c->lb_failed) failed += f;
  c->info.lightbuf_failed = failed;
  if (!failed) c->info.lightbuf_fail_reason[0] = 0;
  if (c->d_lbuf.cap() != c->lb_host.size() || !c->d_lbuf) HIP_TRY(c->d_lbuf.alloc(c->lb_host.size()));
  HIP_TRY(hipMemcpy(c->d_lbuf, c->lb_host.data(), c->lb_host.size() * sizeof(RtLightBuf), hipMemcpyHostToDevice));
  c->lb_ulps = c->eps_ulps;
  c->lb_proven = c->exact_shadows;
  unsigned long long e = 0, n = 0, g = 0, te = 0, tg = 0, nv = 0, bd = 0, tnv = 0, tbd = 0;
  for (LBDevice* d : c->lb_dev) {
    rt_lightbuf_sizes(d, &e, &n, &g);
    rt_lightbuf_proof_counts(d, &nv, &bd);
    te += e;
    tg += g;
    tnv += nv;
    tbd += bd;
  }
  c->info.lightbuf_entries = te;
  c->info.lightbuf_global = tg;
  c->info.lightbuf_never = tnv;
  c->info.lightbuf_band = tbd;
  return RT_OK;
}

int lbuf_prepare(rt_hip_ctx* c, hipStream_t s) {
  if (!c->light_buffers || c->accel != RT_ACCEL_OCTREE || !c->d_node || !c->nlight) return RT_OK;
  if (c->d_lbuf && c->lb_ulps == c->eps_ulps && c->lb_proven == c->exact_shadows) return RT_OK;
  lbuf_release(c);
  c->lb_dev.assign(c->nlight, nullptr);
  c->lb_host.assign(c->nlight, RtLightBuf{});
  c->lb_failed.assign(c->nlight, 0);
  c->info.lightbuf_fail_reason[0] = 0;
  for (uint32_t li = 0; li < c->nlight; li++) {
    const int rc = lbuf_build_one(c, li, s);
    if (rc) {
      for (LBDevice*& d : c->lb_dev) {
        rt_lightbuf_free(d);
        d = nullptr;
      }
      return rc;
    }
  }
  return lbuf_publish(c);
}

extern "C" int rt_hip_set_light_buffers(rt_hip_ctx* c, int enable) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->light_buffers = enable ? 1 : 0;
  c->relight.invalidate();  // the kept masks were decided the other way
  if (!c->light_buffers) lbuf_release(c);
  return RT_OK;
}

extern "C" int rt_hip_set_lightbuf_entry_cap(rt_hip_ctx* c, unsigned long long cap) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->lb_entry_cap = cap;
  c->relight.invalidate();
  lbuf_release(c);  // rebuilt (and the cap applied) by the next render
  HIP_TRY(hipSetDevice(c->device));
  return lbuf_prepare(c, c->stream);
}

// ---- what rt_hip_create and rt_hip_set_triangles share: everything that
// follows from the prim-order records and the scene box ----

// The device-built octree of the prim-order records and the box in
// scene_lo / scene_hi (contexts with dev_tree): the old tree and leaf-order
// records go, the new ones are adopted with their counts.  Synchronises the
// context's stream.
static int tree_rebuild(rt_hip_ctx* c) {
  c->d_tri.reset();
  c->d_node.reset();
  c->nrec = 0;
  // leaf cap 24 measured best on C5 with the trace / shade / fold split and
  // the candidate lists (12: 10.01-10.06 ms, 20 / 24: 9.89, 28: 9.99, 32: 10.01;
  // profiles/r05u_leaf_sweep/); clip level 7 (6 / 8 no better)
  rt_device_build_opts o{24, 7};
  if (const char* e = std::getenv("RT_DEV_LEAF")) o.leaf_cap = std::atoi(e);  // tuning knobs
  if (const char* e = std::getenv("RT_DEV_CLIP")) o.clip_level = std::atoi(e);
  rt_device_tree tree{};
  hipError_t he = rt_device_build_octree(c->d_tri_prim, c->nprim, c->scene_lo, c->scene_hi, &o, c->stream, &tree);
  if (he != hipSuccess) return rt_set_error(RT_EHIP, "device octree build: %s", hipGetErrorString(he));
  // leaf-order records for the walk; the prim-order ones stay for the
  // camera candidate lists
  c->d_tri.adopt(tree.tri, (size_t)tree.nref * RT_TRI_FLOATS / 4);
  c->d_node.adopt(tree.node, (size_t)tree.nnode * RT_NODE_FLOATS / 4);
  c->nrec = tree.nref;
  c->info.nodes = tree.nnode;
  c->info.leaves = tree.leaves;
  c->info.max_depth = tree.depth;
  c->info.max_leaf = tree.max_leaf;
  return RT_OK;
}

// The scene's extent and rt_accel_info's sizes, from scene_lo / scene_hi,
// nprim, nrec, the tree's counts and the tables as they stand.
static void scene_publish(rt_hip_ctx* c) {
  scene_extent(c->nprim, c->scene_lo, c->scene_hi, c->scene_c, &c->scene_r);
  c->info.triangles = c->nprim;
  c->info.tri_refs = c->nrec;
  c->info.tri_record_bytes = RT_TRI_FLOATS * sizeof(float);
  c->info.node_record_bytes = RT_NODE_FLOATS * sizeof(float);
  c->info.device_bytes = ((size_t)c->nrec * RT_TRI_FLOATS + (size_t)c->nprim * 9 + c->mat_host.size() +
                          (size_t)c->nlight * RT_LIGHT_FLOATS + (size_t)c->info.nodes * RT_NODE_FLOATS) *
                         sizeof(float);
  for (int a = 0; a < 3; a++) c->info.scene_center[a] = c->scene_c[a];
  c->info.scene_radius = c->scene_r;
}

// Light buffers: part of the scene's setup, like the octree.  Built with the
// buffers on, whatever the setting, so that rt_accel_info's totals describe
// this geometry (rt_hip_set_light_buffers(0) releases buffers, never totals).
static int scene_light_buffers(rt_hip_ctx* c) {
  const auto l0 = std::chrono::steady_clock::now();
  const int want = c->light_buffers;
  c->light_buffers = 1;
  const int rc = lbuf_prepare(c, c->stream);
  c->light_buffers = want;
  if (!rc && !want) lbuf_release(c);
  c->info.lightbuf_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - l0).count();
  return rc;
}

extern "C" int rt_hip_create(int device, const rt_scene* scene, int accel, rt_hip_ctx** out) {
  if (!scene || !out) return rt_set_error(RT_EINVAL, "null argument");
  if (accel != RT_ACCEL_FLAT && accel != RT_ACCEL_OCTREE && accel != RT_ACCEL_OCTREE_GPU)
    return rt_set_error(RT_EINVAL, "unknown accel %d", accel);
  const bool dev_build = accel == RT_ACCEL_OCTREE_GPU;
  int ndev = 0;
  int rc = rt_hip_device_count(&ndev);
  if (rc) return rc;
  if (device < 0 || device >= ndev) return rt_set_error(RT_ENODEV, "device %d of %d", device, ndev);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return rt_set_error(RT_ENODEV, "device %d is %s, kernels are built for gfx950", device,
                        prop.gcnArchName);
  HIP_TRY(hipSetDevice(device));

  auto t0 = std::chrono::steady_clock::now();
  rt_flat_scene fs;
  // device build: the host only flattens (prim-order records, normals,
  // materials, lights); the octree is built from the uploaded records
  rc = rt_flatten(scene, dev_build ? RT_ACCEL_FLAT : accel, &fs);
  if (rc) return rc;
  auto t1 = std::chrono::steady_clock::now();

  rt_hip_ctx* c = new rt_hip_ctx();
  if (const char* e = std::getenv("RT_CAND_REFINE")) c->cand_refine = std::atoi(e) != 0;  // A/B knob
  if (const char* e = std::getenv("RT_ASYNC_LISTS")) c->async_lists = std::atoi(e) != 0;  // A/B knob
  c->device = device;
  c->accel = dev_build ? (fs.ntri ? RT_ACCEL_OCTREE : RT_ACCEL_FLAT) : accel;
  c->nrec = (uint32_t)fs.nrec;
  c->nlight = (uint32_t)fs.nlight;
  size_t bytes_tri = fs.nrec * RT_TRI_FLOATS * sizeof(float);
  size_t bytes_nrm = fs.ntri * 9 * sizeof(float);
  size_t bytes_mat = fs.nobj * RT_MAT_FLOATS * sizeof(float);
  size_t bytes_light = fs.nlight * RT_LIGHT_FLOATS * sizeof(float);
  size_t bytes_node = fs.nnode * RT_NODE_FLOATS * sizeof(float);
  rc = upload(c->d_tri, fs.tri, bytes_tri);
  if (!rc) rc = upload(c->d_nrm, fs.nrm, bytes_nrm);
  if (!rc) rc = upload(c->d_mat, fs.mat, bytes_mat);
  if (!rc) rc = upload(c->d_light, fs.light, bytes_light);
  if (!rc && fs.nnode) rc = upload(c->d_node, fs.node, bytes_node);
  // the per-frame counters in one allocation, zeroed by one memset per frame:
  // 8 item-stream counters (rt_render.hip), the stats, the hit-record and
  // shade-chunk counters
  if (!rc) rc = upload(c->d_counter, nullptr, kFrameCounterBytes);
  if (!rc) {
    c->d_stats = (unsigned long long*)((char*)c->d_counter.get() + kItemCounterBytes);
    c->d_hit_count = (uint32_t*)((char*)c->d_counter.get() + kItemCounterBytes + kStatBytes);
  }
  if (!rc && hipStreamCreateWithFlags(&c->stream.s, hipStreamNonBlocking) != hipSuccess)
    rc = rt_set_error(RT_EHIP, "hipStreamCreate");
  c->nprim = (uint32_t)fs.ntri;
  for (int a = 0; a < 3; a++) {
    c->scene_lo[a] = fs.ntri ? fs.scene_lo[a] : 0.0f;
    c->scene_hi[a] = fs.ntri ? fs.scene_hi[a] : 0.0f;
  }
  c->info.nodes = fs.nnode;  // (the host's tree, or none; a device tree brings its own)
  c->info.leaves = fs.leaves;
  c->info.max_depth = fs.max_depth;
  c->info.max_leaf = fs.max_leaf;
  c->dev_tree = dev_build && fs.ntri;
  if (!rc && c->dev_tree) {
    c->d_tri_prim_own = std::move(c->d_tri);
    c->d_tri_prim = c->d_tri_prim_own;
    rc = tree_rebuild(c);
  }
  auto t2 = std::chrono::steady_clock::now();
  // what a geometry update needs beside the records (rt_hip_set_triangles;
  // a host tree is never updated): every prim's vertex box, each object's
  // first prim
  if (!rc && accel != RT_ACCEL_OCTREE) rc = upload(c->d_pbox, fs.pbox, fs.ntri * 6 * sizeof(float));
  c->obj_start.assign(1, 0u);
  for (size_t o = 0; o < scene->object_count; o++)
    c->obj_start.push_back(c->obj_start.back() + scene->objects[o].triangle_count);
  if (!rc && !c->d_tri_prim) {
    if (c->accel == RT_ACCEL_FLAT) {
      c->d_tri_prim = c->d_tri;  // already prim order (no candidates needed)
    } else {
      rt_flat_scene fp;  // host octree: records are leaf order, with duplicates
      rc = rt_flatten(scene, RT_ACCEL_FLAT, &fp);
      if (!rc) {
        rc = upload(c->d_tri_prim_own, fp.tri, fp.nrec * RT_TRI_FLOATS * sizeof(float));
        c->d_tri_prim = c->d_tri_prim_own;
        rt_flat_free(&fp);
      }
    }
  }
  if (fs.mat) c->mat_host.assign(fs.mat, fs.mat + fs.nobj * RT_MAT_FLOATS);
  scene_publish(c);
  c->info.build_seconds = std::chrono::duration<double>(dev_build ? t2 - t0 : t1 - t0).count();
  rt_flat_free(&fs);
  if (!rc) rc = shade_tables(c, true, true);
  if (rc) {
    rt_hip_destroy(c);
    return rc;
  }
  // persistent grids: as many one-wave workgroups as each kernel's
  // registers and LDS let a CU hold (rt_render_grid); the compat kernel
  // keeps 16 per CU
  c->grid = prop.multiProcessorCount * 16;
  c->cus = prop.multiProcessorCount;
  for (size_t li = 0; li < scene->light_count; li++) {
    c->light_type.push_back((uint32_t)scene->lights[li].type);
    c->light_v.push_back(scene->lights[li].v.x);
    c->light_v.push_back(scene->lights[li].v.y);
    c->light_v.push_back(scene->lights[li].v.z);
  }
  int gmax = c->grid;
  const int dacc = c->accel == RT_ACCEL_FLAT ? RT_ACCEL_FLAT_D : RT_ACCEL_OCTREE_D;
  for (int tr = 0; tr < 2; tr++)
    for (int pol = 0; pol < RT_NPOLICIES; pol++)
      for (int cw = 0; cw < 2; cw++) {
        int g = 0;
        hipError_t he = rt_render_grid(tr, dacc, cw, pol, prop.multiProcessorCount, &g);
        if (he != hipSuccess) {
          rt_hip_destroy(c);
          return rt_set_error(RT_EHIP, "occupancy query: %s", hipGetErrorString(he));
        }
        c->grid_of[tr][pol][cw] = g;
        gmax = g > gmax ? g : gmax;
      }
  c->info.trace_grid = c->grid_of[1][RT_POLICY_DEFAULT][0];
  c->info.shade_grid = c->grid_of[0][RT_POLICY_LBUF][0];
  // per-lane traversal stack spill area, [entry][lane] for the largest grid
  if (c->accel == RT_ACCEL_OCTREE &&
      c->d_spill.alloc((size_t)gmax * 64 * RT_SPILL_STACK) != hipSuccess) {
    rt_hip_destroy(c);
    return rt_set_error(RT_EHIP, "hipMalloc traversal spill stack");
  }
  rc = scene_light_buffers(c);
  if (rc) {
    rt_hip_destroy(c);
    return rc;
  }
  *out = c;
  return RT_OK;
}

extern "C" int rt_hip_accel_info(const rt_hip_ctx* c, rt_accel_info* out) {
  if (!c || !out) return rt_set_error(RT_EINVAL, "null argument");
  *out = c->info;
  return RT_OK;
}

extern "C" int rt_hip_set_cull_slack(rt_hip_ctx* c, float ulps) {
  if (!c || !(ulps >= 0.0f)) return rt_set_error(RT_EINVAL, "bad slack");
  RT_CTX_LIVE(c);
  c->eps_ulps = ulps;
  c->cam_eps_ulps = ulps;
  c->relight.invalidate();
  lists_changed(c);  // the lists change
  return RT_OK;
}

extern "C" int rt_hip_set_camera_slack(rt_hip_ctx* c, float ulps) {
  if (!c || !(ulps >= 0.0f)) return rt_set_error(RT_EINVAL, "bad slack");
  RT_CTX_LIVE(c);
  c->cam_eps_ulps = ulps;
  lists_changed(c);  // the lists change
  return RT_OK;
}

extern "C" int rt_hip_set_exact_camera(rt_hip_ctx* c, int enable) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->exact_camera = enable ? 1 : 0;
  return RT_OK;
}

extern "C" int rt_hip_set_exact_shadows(rt_hip_ctx* c, int enable) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->exact_shadows = enable ? 1 : 0;
  c->relight.invalidate();
  // built now (setup), reported by rt_hip_accel_info: the light buffers in
  // the matching mode, and the walk's multipliers (policies that walk)
  HIP_TRY(hipSetDevice(c->device));
  int rc = lbuf_prepare(c, c->stream);
  if (rc) return rc;
  if (c->exact_shadows) return shadow_prepare(c, c->stream);
  return RT_OK;
}

// The exact reflection walk's per-node bounds (csrc/rt_reflect.hip): once
// per tree, synchronous (setup).
static int reflect_build(rt_hip_ctx* c, hipStream_t s) {
  const size_t nn = c->info.nodes;
  DevBuf<float> phi;
  DevBuf<uint32_t> d_u;
  HIP_TRY(c->d_node_rf.alloc(3 * nn + 3));
  HIP_TRY(phi.alloc(nn + 1));
  HIP_TRY(d_u.alloc(1));
  ReflParams rp;
  std::memset(&rp, 0, sizeof rp);
  rp.node = c->d_node;
  rp.nnode = (uint32_t)nn;
  rp.rec = c->d_tri;
  rp.node_rf = c->d_node_rf;
  rp.node_phi = phi;
  rp.unbounded = d_u;
  uint32_t u = 0;
  HIP_TRY(hipMemsetAsync(c->d_node_rf, 0, (3 * nn + 3) * sizeof(float4), s));
  HIP_TRY(hipMemsetAsync(d_u, 0, sizeof(uint32_t), s));
  HIP_TRY(rt_reflect_build(&rp, (int)c->info.max_depth + 2, s));
  HIP_TRY(hipMemcpyAsync(&u, d_u, sizeof u, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  c->rf_unbounded = u;
  return RT_OK;
}

int reflect_prepare(rt_hip_ctx* c, hipStream_t s) {
  if (c->d_node_rf || c->accel != RT_ACCEL_OCTREE || !c->d_node) return RT_OK;
  const int rc = reflect_build(c, s);
  if (rc) c->d_node_rf.reset();  // (its presence says "built")
  return rc;
}

extern "C" int rt_hip_set_exact_reflections(rt_hip_ctx* c, int enable) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->exact_refl = enable ? 1 : 0;
  if (!c->exact_refl) return RT_OK;
  HIP_TRY(hipSetDevice(c->device));
  return reflect_prepare(c, c->stream);
}

extern "C" int rt_hip_set_policy(rt_hip_ctx* c, int policy) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  if (policy < RT_POLICY_DEFAULT || policy > RT_POLICY_DIR_STAGED)
    return rt_set_error(RT_EINVAL, "unknown traversal policy %d", policy);
  c->policy = policy;
  c->relight.invalidate();  // (the kept masks are another policy's queries')
  return RT_OK;
}

extern "C" int rt_hip_set_camera_refine(rt_hip_ctx* c, int enable) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->cand_refine = enable ? 1 : 0;
  lists_changed(c);  // the lists change
  return RT_OK;
}

extern "C" int rt_hip_set_camera_bound_scale(rt_hip_ctx* c, double scale) {
  if (!c || !(scale > 0.0)) return rt_set_error(RT_EINVAL, "bad bound scale");
  RT_CTX_LIVE(c);
  c->bound_scale = scale;
  lists_changed(c);  // the lists change
  return RT_OK;
}

// Hit-record buffers for a rank of ntiles tiles: first sized for 2 hits per
// camera ray (the reference scenes make 0.5-1.3; C5 0.48), then for what an
// overflowing frame needed (rt_hip_stats -> RT_EHITBUF); `last` for every
// (item, lane).
// The kept records' mask buffer (KParams::hit_lit): 4 B for every record the
// hit buffers hold; a new one holds no current bit.
static int mask_buffer(rt_hip_ctx* c) {
  const size_t n = c->hit_cap() * RT_HIT_REGIONS;
  if (c->d_hit_lit.holds(n)) return RT_OK;
  c->relight.invalidate();
  HIP_TRY(c->d_hit_lit.alloc(n));
  return RT_OK;
}

// (items: the trace's work items of 64 paths each -- 4 per tile of a frame,
// rt_ray_item_count() of a ray batch; capture: the capturing trace's record
// per (item, lane) too)
int hit_buffers(rt_hip_ctx* c, size_t items, bool capture) {
  HIP_TRY(c->d_last.grow(items * 64, items * 64));
  if (capture) HIP_TRY(c->d_capture.grow(items * 64, items * 64));
  const size_t want = rt_hit_region_records(items, c->hit_need);  // within the slot field of a record index
  if (want <= c->hit_cap()) return c->keep_visibility ? mask_buffer(c) : RT_OK;
  // all three or none: hit_cap() is what every one of them holds; the masks
  // of the records that go (rt_hip_set_keep_visibility, rt_hip_relight) with them
  c->d_hit.reset();
  c->d_hit_prev.reset();
  c->d_hit_term.reset();
  c->d_hit_lit.reset();
  c->relight.invalidate();
  c->paths.drop("a reallocation of the hit buffers");
  const size_t n = want * RT_HIT_REGIONS;
  HIP_TRY(c->d_hit.alloc(2 * n));
  HIP_TRY(c->d_hit_prev.alloc(n));
  HIP_TRY(c->d_hit_term.alloc(n));
  return c->keep_visibility ? mask_buffer(c) : RT_OK;
}

// ---- rt_hip_render, step by step (in the order it runs them) ----

// The refusals: nothing of the context has changed when one of them returns.
static int render_refuse(const rt_hip_ctx* c, const rt_frame* f, int rank, int nranks, const float* d_tiles) {
  if (!c || !f || !d_tiles) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (nranks <= 0 || rank < 0 || rank >= nranks)
    return rt_set_error(RT_EINVAL, "rank %d of %d", rank, nranks);
  if (f->width <= 0 || f->height <= 0) return rt_set_error(RT_EINVAL, "empty frame");
  // cpu/rt's frame is even-sized (rt_frame_from_camera; its output for odd
  // sizes is undefined, cpu/raytracer.c:89-91,128-134); the camera sample
  // model of the candidate lists assumes it (rt_cand_geom.h pixel_range)
  if ((f->width | f->height) & 1)
    return rt_set_error(RT_EINVAL, "frame %dx%d: cpu/rt renders even sizes only", f->width, f->height);
  // the G-buffer's capture exists for the default kernels only (its own
  // trace instantiation, RT_POLICY_GBUFFER): refused before anything changes
  if (c->gbuffer) {
    if (c->policy != RT_POLICY_DEFAULT)
      return rt_set_error(RT_EINVAL, "the G-buffer needs the default traversal policy (have %d)", c->policy);
    if (c->count_work) return rt_set_error(RT_EINVAL, "the G-buffer cannot be captured by the work-counting pass");
    if (c->exact_refl) return rt_set_error(RT_EINVAL, "the G-buffer cannot be captured with exact reflections on");
  }
  return RT_OK;
}

// The frame's camera and this rank's share of its tiles.
static void render_frame_params(KParams& p, const rt_hip_ctx* c, const rt_frame* f, int rank, int nranks,
                                float* d_tiles) {
  p.u = rt::f3{f->u.x, f->u.y, f->u.z};
  p.v = rt::f3{f->v.x, f->v.y, f->v.z};
  p.C = rt::f3{f->C.x, f->C.y, f->C.z};
  p.pos = rt::f3{f->position.x, f->position.y, f->position.z};
  p.W = f->width;
  p.H = f->height;
  p.tiles_x = tiles_x_of(f->width);
  p.ntiles_total = tiles_x_of(f->width) * tiles_y_of(f->height);
  p.rank = rank;
  p.nranks = nranks;
  p.ntiles_local = rank_tile_count(f->width, f->height, rank, nranks);
  p.out = d_tiles;
  p.tile_counter = c->d_counter;
  p.stats = c->d_stats;
}

// The frame's bookkeeping, shared by the empty rank and the full render: the
// remaining timing events ev[first_ev .. 4], and what rt_hip_stats,
// rt_hip_verify_shadows and rt_hip_gbuffer read afterwards.
static int render_done(rt_hip_ctx* c, const KParams& p, const rt_frame* f, hipStream_t s, int first_ev) {
  c->last_p = p;
  c->last_batch = 0;
  c->last_occl = 0;
  if (c->gbuffer) {  // (an empty rank's rt_hip_gbuffer writes nothing either)
    c->gb_frame = *f;
    c->gb_valid = 1;
  }
  // rt_hip_relight may shade this frame's records again; their masks are
  // current only if this render's shade pass wrote them
  c->rl_frame = *f;
  c->rl_valid = 1;
  if (p.hit_lit)
    c->relight.masks_written();
  else
    c->relight.invalidate();
  if (c->timing) {
    hipEvent_t* ev = c->ev[c->frames % RT_TIMED_FRAMES];
    for (int k = first_ev; k < 5; k++) HIP_TRY(hipEventRecord(ev[k], s));
    c->frames++;
  }
  c->last_stream = s;
  return RT_OK;
}

// A rank past the frame's last block (e.g. 96x54 over 8 ranks: 6 blocks)
// renders nothing; its tile buffer (sized by rank 0) stays as it is and
// gathers as padding.  Its stats read 0.
static int render_nothing(rt_hip_ctx* c, const KParams& p, const rt_frame* f, hipStream_t s) {
  c->cand_prims = c->cand_entries = c->cand_global = 0;
  c->d_cand_valid = nullptr;
  c->last_async = 0;
  if (c->timing) {
    HIP_TRY(hipEventRecord(c->ev[c->frames % RT_TIMED_FRAMES][0], s));
    c->ev_side[c->frames % RT_TIMED_FRAMES] = 0;
  }
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, kFrameCounterBytes, s));
  c->cost_hist.valid = 0;  // (the counters hold no trace's clocks now)
  return render_done(c, p, f, s, 1);
}

// The kernels' views of the hit-record buffers and their counters.
void hit_views(const rt_hip_ctx* c, KParams& p) {
  p.hit = c->d_hit;
  p.hit_prev = c->d_hit_prev;
  p.hit_term = c->d_hit_term;
  p.hit_count = c->d_hit_count;
  p.shade_counter = c->d_hit_count + RT_HIT_REGIONS * RT_HIT_STRIDE;
  p.hit_cap = (uint32_t)c->hit_cap();
  p.last = c->d_last;
}

// The hit-record, capture and (work-counting pass) item-clock buffers.
static int render_buffers(rt_hip_ctx* c, KParams& p) {
  {
    int rc = hit_buffers(c, RT_TILE_ITEMS * (size_t)p.ntiles_local, c->gbuffer != 0);
    if (rc) return rc;
  }
  if (c->gbuffer) p.capture = c->d_capture;
  if (c->keep_visibility) p.hit_lit = c->d_hit_lit;  // the shade pass keeps each record's mask (rt_hip_relight)
  hit_views(c, p);
  if (c->count_work) {  // per-item clocks of the instrumented pass (rt_hip_tile_cycles)
    const size_t items = 4 * (size_t)p.ntiles_local;
    HIP_TRY(c->d_tile_cycles.grow(6 * items, 6 * items));
    c->tile_cycles_n = items;
    p.tile_cycles = c->d_tile_cycles;
  }
  return RT_OK;
}

// What the shadow queries need: light buffers, the proven walk's multipliers,
// the off-box queries' queue.
int render_shadows(rt_hip_ctx* c, KParams& p, hipStream_t s) {
  {
    // light buffers, proven in exact-shadow mode (no-op unless the slack or
    // the mode changed); the staged policies walk
    int rc = lbuf_prepare(c, s);
    if (rc) return rc;
    if (c->policy == RT_POLICY_DEFAULT || c->policy == RT_POLICY_LANE) p.lbuf = c->d_lbuf;
  }
  // the proven walk's multipliers: only where some light's queries walk
  const bool walks = !p.lbuf || c->info.lightbuf_failed;
  if (walks) {
    int rc = shadow_prepare(c, s);  // no-op unless the culling slack changed
    if (rc) return rc;
  }
  // proven buffers: the off-box queries' queue.  An entry carries the
  // decided bits of lights 0..31 only, so with more lights the off-box
  // queries are counted instead (shadow_unproven -> RT_EINEXACT), never
  // re-shaded without the lights past the 32nd
  if (p.lbuf && c->exact_shadows && c->nlight <= 32) {
    if (!c->d_oob) {
      HIP_TRY(c->d_oob_count.alloc(1));
      HIP_TRY(c->d_oob.alloc(RT_OOB_CAP));
    }
    p.oob = c->d_oob;
    p.oob_count = c->d_oob_count;
    p.oob_cap = RT_OOB_CAP;
    HIP_TRY(hipMemsetAsync(c->d_oob_count, 0, sizeof(uint32_t), s));
  }
  if (c->exact_shadows && walks) {  // the proven walk
    p.node_mu = c->d_node_mu;
    p.sh_global = c->d_sh_global;
    p.n_sh_global = c->n_sh_global;
    p.sh_omax = c->sh_omax;
  }
  return RT_OK;
}

// The camera rays' candidate lists: the ones rt_hip_cand_consume built for
// this frame (use_ext), or this rank's own build.
static int render_lists(rt_hip_ctx* c, const rt_frame* f, KParams& p, bool use_ext, hipStream_t s) {
  c->cand_prims = c->cand_entries = c->cand_global = 0;
  c->d_cand_valid = nullptr;
  c->list_flag = nullptr;
  if (c->timing) {  // (a build on the side stream records its own start and end there)
    HIP_TRY(hipEventRecord(c->ev[c->frames % RT_TIMED_FRAMES][0], s));
    c->ev_side[c->frames % RT_TIMED_FRAMES] = 0;
  }
  if (c->accel == RT_ACCEL_OCTREE && c->d_node && c->exact_camera) {
    if (use_ext) {  // the lists rt_hip_cand_consume built from the producers' entries
      p.cand_start = c->ext.cand_start;
      p.cand = c->ext.cand;
      p.cand_global = c->ext.cand_global;
      p.n_cand_global = c->ext.n_cand_global;
      p.cand_skip = c->ext.cand_skip;
      p.tile_order = c->ext.tile_order;
      p.n_heavy = c->ext.n_heavy;
      p.tri_prim = c->ext.tri_prim;
      c->cand_entries = c->ext_total;
      c->d_cand_valid = nullptr;
      c->cand_global = c->ext.n_cand_global;
      c->cand_prims = 0;
    } else {
      int rc = cand_prepare(c, f, &p, s, 0, true);
      if (rc) return rc;
    }
  }
  if (!(c->accel == RT_ACCEL_OCTREE && c->d_node && c->exact_camera && !use_ext)) c->last_async = 0;
  return RT_OK;
}

// The kernels a render launches (RenderKernels, rt_ctx.h): the device
// acceleration structure, the trace and shade kernels' policies (their
// instantiations) and grids, for `items` work items of the trace.
int render_kernels(rt_hip_ctx* c, KParams& p, long long items, hipStream_t s, RenderKernels* out) {
  // an empty octree scene has nothing to traverse: the FLAT kernels with 0
  // records are exact (their grids are the FLAT instantiation's own)
  const bool empty = c->accel == RT_ACCEL_OCTREE && !c->d_node;
  const int dacc = (c->accel == RT_ACCEL_FLAT || empty) ? RT_ACCEL_FLAT_D : RT_ACCEL_OCTREE_D;
  const int pol = dacc == RT_ACCEL_FLAT_D ? 0 : c->policy, cw = c->count_work ? 1 : 0;
  // the shade kernel without the walk when every directional / point light
  // queries its buffer (the default and per-lane policies use buffers)
  int spol = pol;
  if (dacc == RT_ACCEL_OCTREE_D && p.lbuf && !p.node_mu && !p.n_sh_global &&
      (pol == RT_POLICY_DEFAULT || pol == RT_POLICY_LANE)) {
    bool all = true;
    for (uint32_t li = 0; li < c->nlight && all; li++)
      if (c->light_type[li] == 1 || c->light_type[li] == 2) all = c->lb_dev[li] != nullptr;
    if (all) spol = RT_POLICY_LBUF;
  }
  // exact reflection rays: the default policy's trace kernel with the proven
  // reflection walk (its own instantiation: the default has no switch)
  int tpol = pol;
  if (dacc == RT_ACCEL_OCTREE_D && c->exact_refl) {
    if (pol != RT_POLICY_DEFAULT)
      return rt_set_error(RT_EINVAL, "exact reflections need the default traversal policy (have %d)", pol);
    int rc = reflect_prepare(c, s);
    if (rc) return rc;
    p.node_rf = c->d_node_rf;
    tpol = RT_POLICY_EXACT_REFL;
  }
  // G-buffer: the default trace kernel (octree or FLAT) plus the capture --
  // its own instantiation; lists, shade, fixup and fold are the default's
  if (c->gbuffer) tpol = RT_POLICY_GBUFFER;
  int gt = empty ? c->grid : c->grid_of[1][tpol][cw], gs = empty ? c->grid : c->grid_of[0][spol][cw];
  // small frames: no more persistent waves than work items (every wave pulls
  // items until all 8 streams drain, so any grid covers the frame; the
  // surplus waves of a full grid only cost dispatch on a frame of a few
  // thousand items -- C1 has 4,096).  The shade kernel's records are not
  // known before the trace, at least one 64-record chunk per item is assumed
  {
    if (items < gt) gt = (int)items;
    if (items < gs) gs = (int)items;
  }
  *out = RenderKernels{dacc, tpol, spol, gt, gs};
  return RT_OK;
}

// The frame's launches: counters zeroed, trace, shade, the deferred shadow
// queries' fixup, fold.
static int render_launch(rt_hip_ctx* c, const rt_frame* f, int rank, int nranks, KParams& p,
                         const RenderKernels& k, hipStream_t s) {
  hipEvent_t* ev = c->ev[c->frames % RT_TIMED_FRAMES];
  // every device pointer the kernels will follow must exist (a null one
  // would fault the card, not fail the call)
  if (!p.tri_prim && (p.lbuf || p.n_sh_global || p.cand_start))
    return rt_set_error(RT_EHIP, "render: prim-order records missing");
  if (!p.hit || !p.last || !p.out || (p.nrec && (!p.tri || !p.nrm)))
    return rt_set_error(RT_EHIP, "render: device buffers missing");
  if (c->gbuffer && !p.capture) return rt_set_error(RT_EHIP, "render: G-buffer capture buffer missing");
  // item clocks for the same frame's next work order (only the candidate
  // lists' order uses them)
  if (p.tile_order) {
    const size_t items = 4 * (size_t)p.ntiles_local;
    if (!c->d_item_cost.holds(items)) {
      c->cost_hist.valid = 0;
      HIP_TRY(c->d_item_cost.grow(items, items));
    }
    p.item_cost = c->d_item_cost;
    p.cost_sum = cost_sum_of(c);
  }
  if (!c->d_frame_check) {
    HIP_TRY(c->d_frame_check.alloc(4));
    HIP_TRY(hipMemsetAsync(c->d_frame_check, 0, 4 * sizeof(unsigned long long), s));
  }
  p.frame_check = c->d_frame_check;
  // (bounds_kernel's copy of the build's counters)
  p.list_flag = c->last_async ? c->list_flag : nullptr;
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, kFrameCounterBytes, s));  // item streams, stats, record counters
  if (c->timing) HIP_TRY(hipEventRecord(ev[1], s));
  HIP_TRY(rt_launch_trace(&p, k.dacc, c->count_work, k.tpol, k.gt, s));
  // the trace is the frame's last reader of the list buffers: the next
  // frame's build may start behind it, beside the shade pass (csrc/rt_overlap.h)
  if (p.cand_start && c->overlap.enabled) {
    if (!c->side_stream.s) HIP_TRY(hipStreamCreateWithFlags(&c->side_stream.s, hipStreamNonBlocking));
    if (!c->ev_lists_free) HIP_TRY(hipEventCreateWithFlags(&c->ev_lists_free, hipEventDisableTiming));
    if (!c->ev_lists_done) HIP_TRY(hipEventCreateWithFlags(&c->ev_lists_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->ev_lists_free, s));
    c->overlap.trace_launched();
  } else {
    c->overlap.lists_touched();
  }
  if (p.item_cost) {
    c->cost_hist.set(f, rank, nranks);
    c->cost_waves = (uint32_t)k.gt;
  } else {
    c->cost_hist.valid = 0;
  }
  if (c->timing) HIP_TRY(hipEventRecord(ev[2], s));
  HIP_TRY(rt_launch_shade(&p, k.dacc, c->count_work, k.spol, k.gs, s));
  HIP_TRY(rt_launch_shade_fixup(&p, c->nprim, s));
  if (c->timing) HIP_TRY(hipEventRecord(ev[3], s));
  HIP_TRY(rt_launch_fold(&p, s));
  return RT_OK;
}

extern "C" int rt_hip_render(rt_hip_ctx* c, const rt_frame* f, int rank, int nranks,
                             float* d_tiles, void* stream) {
  int rc = render_refuse(c, f, rank, nranks, d_tiles);
  if (rc) return rc;
  c->gb_valid = 0;
  c->rl_valid = 0;
  c->paths.drop("rt_hip_render");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // lists rt_hip_cand_consume built for exactly this frame and rank: used once
  const bool use_ext = c->ext_ready && c->ext_rank == rank && c->ext_nranks == nranks &&
                       std::memcmp(&c->ext_frame, f, sizeof *f) == 0;
  c->ext_ready = 0;
  KParams p = scene_params(c);
  render_frame_params(p, c, f, rank, nranks, d_tiles);
  if (p.ntiles_local == 0) return render_nothing(c, p, f, s);
  RenderKernels k;
  if ((rc = render_buffers(c, p)) || (rc = render_shadows(c, p, s)) || (rc = render_lists(c, f, p, use_ext, s)) ||
      (rc = render_kernels(c, p, RT_TILE_ITEMS * (long long)p.ntiles_local, s, &k)) ||
      (rc = render_launch(c, f, rank, nranks, p, k, s)))
    return rc;
  return render_done(c, p, f, s, 4);
}

extern "C" int rt_hip_stats(rt_hip_ctx* c, rt_stats* out) {
  if (!c || !out) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  HIP_TRY(hipSetDevice(c->device));
  // an occlusion batch counted into its own block and touched nothing a
  // frame's readers use (csrc/rt_batch.cpp)
  if (c->last_occl) return occl_stats(c, out);
  unsigned long long hs[RT_STAT_SETS * RT_STAT_STRIDE], h[RT_NSTATS];
  uint32_t hc[RT_HIT_REGIONS * RT_HIT_STRIDE];
  hipStream_t s = c->last_stream ? c->last_stream : c->stream;
  HIP_TRY(hipMemcpyAsync(hs, c->d_stats, sizeof hs, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hc, c->d_hit_count, sizeof hc, hipMemcpyDeviceToHost, s));
  uint32_t valid = 0, actr[RT_CC_BUILD_WORDS] = {};
  // a ray batch (rt_hip_trace_rays) used no list: a frame's list counts stay
  // where they are for that frame's own readers, and the batch reports none
  const bool batch = c->last_batch != 0;
  if (c->d_cand_valid && !batch)
    HIP_TRY(hipMemcpyAsync(&valid, c->d_cand_valid, sizeof valid, hipMemcpyDeviceToHost, s));
  const int was_async = batch ? 0 : c->last_async;
  if (was_async)
    HIP_TRY(hipMemcpyAsync(actr, c->d_cand_ctr + RT_CAND_CTR_SNAPSHOT, sizeof actr, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (c->d_cand_valid && !batch) {
    c->cand_entries = valid;
    c->d_cand_valid = nullptr;
  }
  if (was_async) {
    c->last_async = 0;
    c->cand_global = actr[RT_CC_GLOBAL];
    if (actr[RT_CC_OVERFLOW]) {  // never expected (the same frame's lists): reported, and the next build reads back
      lists_changed(c);
      return rt_set_error(RT_EHITBUF, "%u candidate-list entries, %u expected: render again", actr[RT_CC_TOTAL],
                          c->forecast.known.total);
    }
  }
  for (int k = 0; k < RT_NSTATS; k++) {  // the copies of each counter (RT_STAT_SETS)
    h[k] = 0;
    for (int set = 0; set < RT_STAT_SETS; set++) h[k] += hs[set * RT_STAT_STRIDE + k];
  }
  size_t need = 0;
  unsigned long long records = 0;
  for (int x = 0; x < RT_HIT_REGIONS; x++) {
    need = hc[RT_HIT_STRIDE * x] > need ? hc[RT_HIT_STRIDE * x] : need;
    records += hc[RT_HIT_STRIDE * x];
  }
  std::memset(out, 0, sizeof *out);
  for (int k = 0; k < RT_NSTATS; k++) out->*rt_stat_member[k] = h[k];
  out->camera = 4 * h[RT_ST_PIXELS];
  out->hit_records = records;
  if (batch) {  // the rays traced, counted in the pixels' slot; no pixel, no list
    out->camera = h[RT_ST_PIXELS];
    out->pixels = 0;
  } else {
    out->cand_prims = c->cand_prims;
    out->cand_entries = c->cand_entries;
    out->cand_global = c->cand_global;
  }
  if (need > c->hit_cap()) {  // the frame is incomplete: grow for the next render
    c->hit_need = need + need / 4 + 1024;
    return rt_set_error(RT_EHITBUF, "%llu hit records, %zu per region held (grown to %zu: render again)",
                        records, c->hit_cap(), c->hit_need);
  }
  if (out->depth_overflow)
    return rt_set_error(RT_EDEPTH, "%llu paths overflowed the bounce limit or a traversal stack",
                        out->depth_overflow);
  // never silent: the image may differ from cpu/rt's there
  if (out->zero_normal)
    return rt_set_error(RT_EZERONORMAL,
                        "%llu closest hits had an exactly zero interpolated normal (cpu/hit.c:79 "
                        "would skip those objects)",
                        out->zero_normal);
  if (out->shadow_zero_risk)
    return rt_set_error(RT_EZERONORMAL,
                        "%llu shadow rays hit an object whose interpolated normal can vanish "
                        "(cpu/hit.c:99 may skip it; early any-hit exit not proven exact)",
                        out->shadow_zero_risk);
  if (c->last_p.oob) {
    uint32_t q = 0;
    HIP_TRY(hipMemcpy(&q, c->d_oob_count, sizeof q, hipMemcpyDeviceToHost));
    out->shadow_deferred = q;
    if (q > RT_OOB_CAP)
      return rt_set_error(RT_EINEXACT, "%u shadow queries from off the exact mode's proof box, %u decided",
                          q, RT_OOB_CAP);
  }
  if (out->closest_unproven)
    return rt_set_error(RT_EINEXACT,
                        "%llu reflection rays with |d| past the exact reflection walk's bound "
                        "(csrc/rt_reflect.h RT_RF_DLMAX)", out->closest_unproven);
  if (out->shadow_unproven)
    return rt_set_error(RT_EINEXACT,
                        "%llu shadow rays left from beyond the extent the exact shadow mode's "
                        "bound assumes (csrc/rt_shadow.hip, csrc/rt_lightbuf.hip)",
                        out->shadow_unproven);
  // tuning knobs that give up the parity guarantee (A/B measurements only):
  // the image is complete, but not promised to equal cpu/rt's
  if (c->accel == RT_ACCEL_OCTREE && c->d_node &&
      (!c->exact_camera || c->bound_scale < 1.0 || c->eps_ulps < RT_EPS_ULPS_DEFAULT))
    return rt_set_error(RT_EINEXACT,
                        "rendered with exact_camera=%d, camera bound scale %g, culling slack %g ulps "
                        "(defaults 1, 1, %d): cpu/rt parity not guaranteed",
                        c->exact_camera, c->bound_scale, (double)c->eps_ulps, RT_EPS_ULPS_DEFAULT);
  return RT_OK;
}

extern "C" int rt_hip_assemble(rt_hip_ctx* c, const rt_frame* f, const float* d_gathered,
                               int nranks, float* d_rgb, void* stream) {
  if (!c || !f || !d_gathered || !d_rgb || nranks <= 0)
    return rt_set_error(RT_EINVAL, "bad argument");
  RT_CTX_LIVE(c);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  int tx = tiles_x_of(f->width);
  int nt = tx * tiles_y_of(f->height);
  HIP_TRY(rt_launch_assemble(d_gathered, d_rgb, f->width, f->height, tx, nt, nranks,
                             rt_hip_tiles_per_rank(f->width, f->height, nranks), s));
  return RT_OK;
}

extern "C" int rt_hip_render_image(rt_hip_ctx* c, const rt_frame* f, float* h_rgb, rt_stats* st) {
  if (!c || !f || !h_rgb) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  HIP_TRY(hipSetDevice(c->device));
  size_t nt = rt_hip_tile_buffer_floats(f->width, f->height, 1);
  size_t npx = (size_t)f->width * f->height;
  DevBuf<float> d_tiles, d_rgb;
  HIP_TRY(d_tiles.alloc(nt));
  if (d_rgb.alloc(npx * 3) != hipSuccess) return rt_set_error(RT_EHIP, "hipMalloc image");
  rt_stats tmp;
  int rc = RT_OK;
  for (int attempt = 0; attempt < 3; attempt++) {  // again after the hit or list buffers grew
    rc = rt_hip_render(c, f, 0, 1, d_tiles, nullptr);
    if (!rc) rc = rt_hip_assemble(c, f, d_tiles, 1, d_rgb, nullptr);
    if (!rc && hipMemcpyAsync(h_rgb, d_rgb, npx * 3 * sizeof(float), hipMemcpyDeviceToHost,
                              c->stream) != hipSuccess)
      rc = rt_set_error(RT_EHIP, "D2H image");
    if (!rc) rc = rt_hip_stats(c, st ? st : &tmp);
    if (rc != RT_EHITBUF) break;
  }
  return rc;
}

// ------------------------------------------------------------------ relight
// Lights and materials edited in place, and the last render's kept hit
// records shaded again under them (include/rt_hip.h; the bookkeeping is
// csrc/rt_relight.h, the kernels csrc/rt_recolour.h and shade_kernel).

static std::vector<RelightLight> light_table(const rt_hip_ctx* c) {
  std::vector<RelightLight> t(c->nlight);
  for (uint32_t li = 0; li < c->nlight; li++) t[li] = RelightLight(c->light_type[li], &c->light_v[3 * li]);
  return t;
}

// Setup calls that free or overwrite what a kernel in flight may read wait
// for the last render's stream and the context's own first.
static int relight_quiesce(rt_hip_ctx* c) {
  if (c->last_stream && c->last_stream != c->stream.s) HIP_TRY(hipStreamSynchronize(c->last_stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RT_OK;
}

extern "C" int rt_hip_set_lights(rt_hip_ctx* c, const rt_light* lights, size_t n) {
  if (!c || (n && !lights)) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (n > 0x7fffffffu / RT_LIGHT_FLOATS) return rt_set_error(RT_EINVAL, "%zu lights", n);
  HIP_TRY(hipSetDevice(c->device));
  int rc = relight_quiesce(c);
  if (rc) return rc;
  std::vector<float> rows(n * RT_LIGHT_FLOATS, 0.0f), lv(3 * n);
  std::vector<uint32_t> type(n);
  for (size_t li = 0; li < n; li++) {  // the rows rt_flatten writes (host/accel.c)
    const rt_light& l = lights[li];
    float* L = &rows[RT_LIGHT_FLOATS * li];
    type[li] = (uint32_t)l.type;
    std::memcpy(&L[0], &type[li], sizeof(float));
    L[1] = l.r, L[2] = l.g, L[3] = l.b;
    L[4] = lv[3 * li] = l.v.x, L[5] = lv[3 * li + 1] = l.v.y, L[6] = lv[3 * li + 2] = l.v.z;
  }
  const std::vector<RelightLight> was = light_table(c);
  const size_t old_n = c->nlight;
  rc = upload(c->d_light, rows.data(), rows.size() * sizeof(float));
  if (rc) return rc;
  c->nlight = (uint32_t)n;
  c->light_type = type;
  c->light_v = lv;
  const std::vector<RelightLight> now = light_table(c);
  std::vector<uint8_t> rebuild, release;
  c->relight.set_lights(was, now, rebuild, release);
  bool edited = was.size() != now.size();
  for (size_t li = 0; li < now.size() && !edited; li++) edited = !now[li].same(was[li]);
  if (edited) c->sh_ulps = -1.0f;  // the proven walk's multipliers are per light table (shadow_prepare)
  // the last render's parameters are views into the context's buffers
  c->last_p.light = c->d_light;
  c->last_p.nlight = c->nlight;
  rc = shade_tables(c, true, false);
  c->last_p.lshade = c->d_lshade;
  if (rc) return rc;
  if (!(c->light_buffers && c->accel == RT_ACCEL_OCTREE && c->d_node)) return RT_OK;  // no light has a buffer
  const bool current = c->d_lbuf && c->lb_ulps == c->eps_ulps && c->lb_proven == c->exact_shadows &&
                       c->lb_dev.size() == old_n && c->lb_host.size() == old_n && c->lb_failed.size() == old_n;
  if (!current || n == 0) {  // every buffer: none is built for this slack and mode, or none is left
    lbuf_release(c);
    c->lb_dev.clear();
    c->lb_host.clear();
    c->lb_failed.clear();
    c->last_p.lbuf = nullptr;
    c->info.lightbuf_entries = c->info.lightbuf_global = c->info.lightbuf_never = c->info.lightbuf_band = 0;
    c->info.lightbuf_failed = 0;
    c->info.lightbuf_fail_reason[0] = 0;
    rc = lbuf_prepare(c, c->stream);
    if (c->last_p.hit) c->last_p.lbuf = c->d_lbuf;
    return rc;
  }
  for (size_t li = 0; li < old_n; li++)
    if (release[li]) {
      rt_lightbuf_free(c->lb_dev[li]);
      c->lb_dev[li] = nullptr;
    }
  c->lb_dev.resize(n, nullptr);
  c->lb_host.resize(n, RtLightBuf{});
  c->lb_failed.resize(n, 0);
  for (uint32_t li = 0; li < n; li++) {
    if (!now[li].casts()) {  // (its buffer, if it had one, was released)
      c->lb_host[li] = RtLightBuf{};
      c->lb_failed[li] = 0;
    }
    if (!rebuild[li]) continue;
    rc = lbuf_build_one(c, li, c->stream);
    if (rc) {  // a failed launch: no buffer is trusted, the next render builds them all
      lbuf_release(c);
      c->last_p.lbuf = nullptr;
      return rc;
    }
  }
  rc = lbuf_publish(c);
  c->last_p.lbuf = c->last_p.lbuf ? c->d_lbuf.get() : nullptr;
  return rc;
}

extern "C" int rt_hip_set_materials(rt_hip_ctx* c, const rt_object* objects, size_t n) {
  if (!c || (n && !objects)) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (n * RT_MAT_FLOATS != c->mat_host.size())
    return rt_set_error(RT_EINVAL, "%zu objects, the context has %zu", n, c->mat_host.size() / RT_MAT_FLOATS);
  std::vector<float> rows(c->mat_host.size(), 0.0f);
  for (size_t o = 0; o < n; o++) {  // the rows rt_flatten writes (host/accel.c)
    const rt_object& ob = objects[o];
    float* m = &rows[RT_MAT_FLOATS * o];
    m[0] = ob.ka.x, m[1] = ob.ka.y, m[2] = ob.ka.z;
    m[3] = ob.kd.x, m[4] = ob.kd.y, m[5] = ob.kd.z;
    m[6] = ob.ks.x, m[7] = ob.ks.y, m[8] = ob.ks.z;
    m[9] = ob.ns;
    m[10] = ob.nr;
    // what the trace reads of the row (trace_path: obj.nr * coef) decides the
    // paths: it must be what the kept records were traced with
    if (std::memcmp(&m[10], &c->mat_host[RT_MAT_FLOATS * o + 10], 2 * sizeof(float)) != 0)
      return rt_set_error(RT_EINVAL, "object %zu: nr %g differs from the context's %g (reflectivity changes the paths: "
                          "create a new context)", o, (double)ob.nr, (double)c->mat_host[RT_MAT_FLOATS * o + 10]);
  }
  if (!n) return RT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const int rc = relight_quiesce(c);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(c->d_mat, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
  c->mat_host = rows;
  const int tables = shade_tables(c, false, true);
  c->last_p.mshade = c->d_mshade;  // (the last render's parameters are views into the context's buffers)
  return tables;
}

// --------------------------------------------------------- moving geometry
// New triangles in a live context (include/rt_hip.h rt_hip_set_triangles):
// the device derives what rt_flatten derives (csrc/rt_geom.hip), then
// everything keyed on the geometry is rebuilt in rt_hip_create's order and
// everything that described the old geometry is forgotten.

// Nothing of the old geometry's frames, lists or batches is current.
static int geometry_forget(rt_hip_ctx* c) {
  lists_changed(c);  // joins a side-stream build; the forecast and pknown start over
  c->overlap.lists_touched();
  c->ext_ready = 0;
  c->cost_hist.valid = 0;
  c->rl_valid = 0;
  c->gb_valid = 0;
  c->relight.invalidate();
  c->paths.drop("rt_hip_set_triangles");
  c->last_batch = 0;
  c->last_occl = 0;
  c->last_async = 0;
  c->d_cand_valid = nullptr;
  c->list_flag = nullptr;
  c->cand_prims = c->cand_entries = c->cand_global = 0;
  c->send_n = 0;
  std::memset(&c->last_p, 0, sizeof c->last_p);  // its views pointed into the old records and nodes
  std::memset(&c->ext, 0, sizeof c->ext);
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, kFrameCounterBytes, c->stream));  // no frame's counters either
  return RT_OK;
}

// d_src: count (> 0) records in device memory; the range is inside the
// context's prims.  Leaves the context broken on failure.
static int geometry_update(rt_hip_ctx* c, const float* d_src, size_t first, size_t count) {
  using clk = std::chrono::steady_clock;
  const auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  HIP_TRY(hipSetDevice(c->device));
  int rc = relight_quiesce(c);
  if (rc) return rc;
  if (c->occl_stream && c->occl_stream != c->stream.s) HIP_TRY(hipStreamSynchronize(c->occl_stream));
  c->broken = 1;
  if ((rc = geometry_forget(c))) return rc;
  hipStream_t s = c->stream;
  const size_t nobj = c->obj_start.size() - 1;
  if (!c->d_pbox.holds((size_t)c->nprim * 6)) return rt_set_error(RT_EHIP, "geometry update: the prims' boxes are missing");
  if (!c->d_objflag.holds(nobj)) HIP_TRY(c->d_objflag.alloc(nobj));
  if (!c->d_geom_box.holds(RT_GEOM_BOX_FLOATS)) HIP_TRY(c->d_geom_box.alloc(RT_GEOM_BOX_FLOATS));
  const auto t0 = clk::now();
  // 1: the range's records, normal rows and vertex boxes
  HIP_TRY(rt_geom_flatten(d_src, (uint32_t)first, (uint32_t)count, c->d_tri_prim, c->d_nrm, c->d_pbox, s));
  // 2: the scene box, over every prim (a partial update can shrink it)
  HIP_TRY(rt_geom_scene_box(c->d_pbox, c->nprim, c->d_geom_box, s));
  float box[6];
  HIP_TRY(hipMemcpyAsync(box, c->d_geom_box + 6 * RT_GEOM_BOX_BLOCKS, sizeof box, hipMemcpyDeviceToHost, s));
  // 3: the zero-normal risk flags of the objects the range touches, from all
  // their triangles
  {
    const auto ob = [&](size_t p) {  // the object holding prim p (empty objects hold none)
      return (uint32_t)(std::upper_bound(c->obj_start.begin(), c->obj_start.end(), (uint32_t)p) -
                        c->obj_start.begin() - 1);
    };
    const uint32_t o0 = ob(first), o1 = ob(first + count - 1);
    HIP_TRY(rt_geom_zero_risk(c->d_tri_prim, c->d_nrm, c->obj_start[o0], c->obj_start[o1 + 1], c->d_objflag, o0, o1,
                              s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  for (int a = 0; a < 3; a++) c->scene_lo[a] = box[a], c->scene_hi[a] = box[3 + a];
  const auto t1 = clk::now();
  // 4: the tree (FLAT: the prim-order records are the scene image)
  if (c->dev_tree && (rc = tree_rebuild(c))) return rc;
  scene_publish(c);
  const auto t2 = clk::now();
  // everything keyed on the geometry: dropped, and rebuilt where rt_hip_create
  // or the context's settings had built it
  c->d_prim_leaf.reset();
  const bool had_mu = c->d_node_mu;
  c->d_prim_mu.reset();
  c->d_node_mu.reset();
  c->d_sh_global.reset();
  c->sh_ulps = -1.0f;
  c->n_sh_global = 0;
  c->sh_omax = 0.0f;
  c->sh_mu_max = 1.0f;
  c->info.shadow_global = 0;
  c->info.shadow_mu_max = 0.0;
  c->d_node_rf.reset();
  c->rf_unbounded = 0;
  lbuf_release(c);
  if ((rc = scene_light_buffers(c))) return rc;
  const auto t3 = clk::now();
  if (had_mu && (rc = shadow_prepare(c, s))) return rc;
  if (c->exact_refl && (rc = reflect_prepare(c, s))) return rc;
  c->info.build_seconds = secs(t0, t2);
  c->geom_seconds[0] = secs(t0, t1);
  c->geom_seconds[1] = secs(t1, t2);
  c->geom_seconds[2] = secs(t2, t3);
  c->broken = 0;
  c->geom_updates++;
  return RT_OK;
}

// The refusals: nothing of the context has changed when one of them returns.
static int geometry_refuse(const rt_hip_ctx* c, const void* triangles, size_t first, size_t count) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  if (c->accel == RT_ACCEL_OCTREE && !c->dev_tree)
    return rt_set_error(RT_EINVAL, "the context's octree was built on the host from the rt_scene (RT_ACCEL_OCTREE): "
                                   "make a new context, or use RT_ACCEL_OCTREE_GPU");
  if (first > c->nprim || count > c->nprim - first)
    return rt_set_error(RT_EINVAL, "triangles [%zu, %zu + %zu) of %u", first, first, count, c->nprim);
  if (count && !triangles) return rt_set_error(RT_EINVAL, "null triangles");
  return RT_OK;
}

extern "C" int rt_hip_set_triangles(rt_hip_ctx* c, const void* d_triangles, size_t first, size_t count) {
  const int rc = geometry_refuse(c, d_triangles, first, count);
  if (rc || !count) return rc;
  return geometry_update(c, (const float*)d_triangles, first, count);
}

static_assert(sizeof(rt_triangle) == 18 * sizeof(float), "rt_triangle is the 18 floats k_flatten reads");
extern "C" int rt_hip_set_triangles_host(rt_hip_ctx* c, const rt_triangle* h_triangles, size_t first, size_t count) {
  const int rc = geometry_refuse(c, h_triangles, first, count);
  if (rc || !count) return rc;
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<float> d_src;  // (nothing of the context is touched before the upload holds)
  HIP_TRY(d_src.alloc(count * 18));
  HIP_TRY(hipMemcpy(d_src, h_triangles, count * sizeof(rt_triangle), hipMemcpyHostToDevice));
  return geometry_update(c, d_src, first, count);
}

extern "C" int rt_hip_geometry_updates(const rt_hip_ctx* c, unsigned long long* n) {
  if (!c || !n) return rt_set_error(RT_EINVAL, "null argument");
  *n = c->geom_updates;
  return RT_OK;
}

extern "C" int rt_hip_geometry_times(const rt_hip_ctx* c, double seconds[3]) {
  if (!c || !seconds) return rt_set_error(RT_EINVAL, "null argument");
  for (int k = 0; k < 3; k++) seconds[k] = c->geom_seconds[k];
  return RT_OK;
}

extern "C" int rt_hip_set_keep_visibility(rt_hip_ctx* c, int enable) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->keep_visibility = enable ? 1 : 0;  // (the mask buffer comes with the next render's hit buffers)
  return RT_OK;
}

extern "C" int rt_hip_relight(rt_hip_ctx* c, const rt_frame* f, int rank, int nranks, float* d_tiles,
                              void* stream) {
  if (!c || !f || !d_tiles) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  // the refusals: nothing of the context has changed when one of them returns
  if (!c->rl_valid)
    return rt_set_error(RT_EINVAL, "no kept hit records: rt_hip_render first (rt_hip_render_compat keeps none)");
  const KParams& lp = c->last_p;
  if (lp.rank != rank || lp.nranks != nranks || std::memcmp(&c->rl_frame, f, sizeof *f) != 0)
    return rt_set_error(RT_EINVAL, "the kept records are another frame's (last render: %dx%d, rank %d of %d)", lp.W,
                        lp.H, lp.rank, lp.nranks);
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (s != c->last_stream) return rt_set_error(RT_EINVAL, "a relight runs on the stream of its render");
  if (c->policy != RT_POLICY_DEFAULT)
    return rt_set_error(RT_EINVAL, "a relight needs the default traversal policy (have %d)", c->policy);
  if (c->count_work) return rt_set_error(RT_EINVAL, "a relight cannot run as the work-counting pass");
  if (lp.ntiles_local == 0) {  // a rank past the last block: nothing rendered, nothing written
    c->last_occl = 0;
    return RT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  // the render's parameters with the scene as it is now and nothing of the
  // render's shadow set-up (rebuilt below for the current lights and mode)
  KParams p = lp;
  {
    const KParams sp = scene_params(c);
    p.light = sp.light;
    p.nlight = sp.nlight;
    p.mat = sp.mat;
    p.mshade = sp.mshade;
    p.lshade = sp.lshade;
    p.eps_rel = sp.eps_rel;
    p.eps_rel_cam = sp.eps_rel_cam;
  }
  p.out = d_tiles;
  p.lbuf = nullptr;
  p.node_mu = nullptr;
  p.sh_global = nullptr;
  p.n_sh_global = 0;
  p.sh_omax = 0.0f;
  p.oob = nullptr;
  p.oob_count = nullptr;
  p.oob_cap = 0;
  p.shade_stride = p.shade_first = 0;
  p.relight_dirty = 0;
  // the fold's frame check counts renders only (rt_hip_frame_check)
  p.frame_check = nullptr;
  p.list_flag = nullptr;
  int rc = mask_buffer(c);  // (a new one: every bit is stale, the full shade writes them)
  if (rc) return rc;
  p.hit_lit = c->d_hit_lit;
  RenderKernels k;
  if ((rc = render_shadows(c, p, s)) || (rc = render_kernels(c, p, RT_TILE_ITEMS * (long long)p.ntiles_local, s, &k)))
    return rc;
  const RelightWork w = c->relight.work(light_table(c));
  if (w.path == RT_RELIGHT_RECOLOUR) p.oob = nullptr;  // no query, so none deferred: no fixup
  // every device pointer the kernels will follow must exist (a null one
  // would fault the card, not fail the call)
  if (!p.tri_prim && (p.lbuf || p.n_sh_global)) return rt_set_error(RT_EHIP, "relight: prim-order records missing");
  if (!p.hit || !p.hit_prev || !p.hit_term || !p.hit_lit || !p.hit_count || !p.shade_counter || !p.stats ||
      !p.last || !p.out || (p.nlight && (!p.light || !p.lshade)) || (p.nrec && (!p.tri || !p.nrm)) || !p.mat ||
      !p.mshade ||
      p.hit_cap != c->hit_cap() || !c->d_hit_lit.holds((size_t)p.hit_cap * RT_HIT_REGIONS))
    return rt_set_error(RT_EHIP, "relight: device buffers missing");
  HIP_TRY(rt_launch_relight_zero(&p, s));
  if (w.path == RT_RELIGHT_RECOLOUR) {
    HIP_TRY(rt_launch_recolour(&p, c->cus, s));
  } else if (w.path == RT_RELIGHT_PARTIAL) {
    p.relight_dirty = w.dirty;
    HIP_TRY(rt_launch_reshade(&p, k.dacc, k.spol, k.gs, s));
  } else {
    HIP_TRY(rt_launch_shade(&p, k.dacc, 0, k.spol, k.gs, s));
  }
  HIP_TRY(rt_launch_shade_fixup(&p, c->nprim, s));
  HIP_TRY(rt_launch_fold(&p, s));
  c->relight.masks_written();
  c->last_occl = 0;
  c->last_p = p;  // rt_hip_stats (the deferred count), rt_hip_verify_shadows, rt_hip_gbuffer (its fields are the render's)
  return RT_OK;
}

extern "C" int rt_hip_relight_image(rt_hip_ctx* c, const rt_frame* f, float* h_rgb, rt_stats* st) {
  if (!c || !f || !h_rgb) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (f->width <= 0 || f->height <= 0) return rt_set_error(RT_EINVAL, "empty frame");
  HIP_TRY(hipSetDevice(c->device));
  const size_t nt = rt_hip_tile_buffer_floats(f->width, f->height, 1);
  const size_t npx = (size_t)f->width * f->height;
  DevBuf<float> d_tiles, d_rgb;
  HIP_TRY(d_tiles.alloc(nt));
  if (d_rgb.alloc(npx * 3) != hipSuccess) return rt_set_error(RT_EHIP, "hipMalloc image");
  rt_stats tmp;
  int rc = rt_hip_relight(c, f, 0, 1, d_tiles, nullptr);
  if (rc) return rc;
  rc = rt_hip_assemble(c, f, d_tiles, 1, d_rgb, nullptr);
  if (!rc && hipMemcpyAsync(h_rgb, d_rgb, npx * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
    rc = rt_set_error(RT_EHIP, "D2H image");
  const int src = rt_hip_stats(c, st ? st : &tmp);  // (synchronises: the buffers above may go)
  return rc ? rc : src;
}

// ----------------------------------------------------------------- G-buffer
static_assert(RT_GB_WORDS == RT_GB_WORDS_D && sizeof(rt_gsample) == 4 * RT_GB_WORDS,
              "rt_gsample is the record gbuffer_kernel writes");
extern "C" int rt_hip_set_gbuffer(rt_hip_ctx* c, int enable) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  c->gbuffer = enable ? 1 : 0;
  if (!c->gbuffer) c->gb_valid = 0;
  return RT_OK;
}

extern "C" size_t rt_hip_gbuffer_tile_words(int width, int height, int nranks) {
  return (size_t)rt_hip_tiles_per_rank(width, height, nranks) * 64 * 4 * RT_GB_WORDS;
}

extern "C" int rt_hip_gbuffer(rt_hip_ctx* c, const rt_frame* f, int rank, int nranks, void* d_tiles,
                              void* stream) {
  if (!c || !f || !d_tiles) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if ((uintptr_t)d_tiles & 7) return rt_set_error(RT_EINVAL, "G-buffer tiles must be 8-byte aligned");
  if (!c->gbuffer || !c->gb_valid)
    return rt_set_error(RT_EINVAL, "no G-buffer capture: rt_hip_set_gbuffer(1), then rt_hip_render");
  const KParams& lp = c->last_p;
  if (lp.rank != rank || lp.nranks != nranks || std::memcmp(&c->gb_frame, f, sizeof *f) != 0)
    return rt_set_error(RT_EINVAL, "the G-buffer holds another frame (last render: %dx%d, rank %d of %d)",
                        lp.W, lp.H, lp.rank, lp.nranks);
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (s != c->last_stream)
    return rt_set_error(RT_EINVAL, "the G-buffer must be read on the stream of its render");
  if (lp.ntiles_local == 0) return RT_OK;  // a rank past the last block: nothing rendered, nothing written
  HIP_TRY(hipSetDevice(c->device));
  // every pointer gbuffer_kernel follows (a null one would fault the card)
  if (!lp.capture || !lp.hit || (lp.nrec && !lp.tri_prim))
    return rt_set_error(RT_EHIP, "G-buffer: device buffers missing");
  HIP_TRY(rt_launch_gbuffer(&lp, (uint32_t*)d_tiles, s));
  return RT_OK;
}

extern "C" int rt_hip_assemble_gbuffer(rt_hip_ctx* c, const rt_frame* f, const void* d_gathered, int nranks,
                                       void* d_samples, void* stream) {
  if (!c || !f || !d_gathered || !d_samples || nranks <= 0) return rt_set_error(RT_EINVAL, "bad argument");
  RT_CTX_LIVE(c);
  if (f->width <= 0 || f->height <= 0) return rt_set_error(RT_EINVAL, "empty frame");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(rt_launch_assemble_words((const uint32_t*)d_gathered, (uint32_t*)d_samples, f->width, f->height,
                                   tiles_x_of(f->width), nranks,
                                   rt_hip_tiles_per_rank(f->width, f->height, nranks), 4 * RT_GB_WORDS, s));
  return RT_OK;
}

// rt_hip_render_image with the G-buffer on for the call (the context's
// setting is restored): the image, and the samples in PPM pixel order
extern "C" int rt_hip_render_image_gbuffer(rt_hip_ctx* c, const rt_frame* f, float* h_rgb,
                                           rt_gsample* h_samples, rt_stats* st) {
  if (!c || !f || !h_rgb || !h_samples) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (f->width <= 0 || f->height <= 0) return rt_set_error(RT_EINVAL, "empty frame");
  HIP_TRY(hipSetDevice(c->device));
  const size_t nt = rt_hip_tile_buffer_floats(f->width, f->height, 1);
  const size_t ng = rt_hip_gbuffer_tile_words(f->width, f->height, 1);
  const size_t npx = (size_t)f->width * f->height;
  const size_t nsw = npx * 4 * RT_GB_WORDS;
  DevBuf<float> d_tiles, d_rgb;
  DevBuf<uint32_t> d_gt, d_gs;
  if (d_tiles.alloc(nt) != hipSuccess || d_rgb.alloc(npx * 3) != hipSuccess || d_gt.alloc(ng) != hipSuccess ||
      d_gs.alloc(nsw) != hipSuccess)
    return rt_set_error(RT_EHIP, "hipMalloc image and G-buffer");
  int rc = RT_OK;
  const int was = c->gbuffer;
  c->gbuffer = 1;
  rt_stats tmp;
  for (int attempt = 0; attempt < 3; attempt++) {  // again after the hit or list buffers grew
    rc = rt_hip_render(c, f, 0, 1, d_tiles, nullptr);
    if (!rc) rc = rt_hip_assemble(c, f, d_tiles, 1, d_rgb, nullptr);
    if (!rc) rc = rt_hip_gbuffer(c, f, 0, 1, d_gt, nullptr);
    if (!rc) rc = rt_hip_assemble_gbuffer(c, f, d_gt, 1, d_gs, nullptr);
    if (!rc && (hipMemcpyAsync(h_rgb, d_rgb, npx * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream) !=
                    hipSuccess ||
                hipMemcpyAsync(h_samples, d_gs, nsw * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) !=
                    hipSuccess))
      rc = rt_set_error(RT_EHIP, "D2H image and G-buffer");
    if (!rc) rc = rt_hip_stats(c, st ? st : &tmp);
    if (rc != RT_EHITBUF) break;
  }
  c->gbuffer = was;
  if (!was) c->gb_valid = 0;
  return rc;
}

int choose_accel(const rt_scene* s);

// gpu/rt compatibility mode (csrc/rt_compat.h compat_kernel): the frame
// of the camera at 3x its size (gpu/rt.cpp:72-83: width and height scaled,
// so L and C follow), one ray per high-resolution pixel, then the 3x3
// downscale; h_rgba = width x height RGBA8 in gpu/rt's PNG row order.
extern "C" int rt_hip_render_compat(rt_hip_ctx* c, const rt_camera* cam, unsigned char* h_rgba,
                                    rt_stats* st) {
  if (!c || !cam || !h_rgba) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (cam->width <= 0 || cam->height <= 0) return rt_set_error(RT_EINVAL, "empty frame");
  if ((long long)cam->width * cam->height > (1ll << 28) / 9)
    return rt_set_error(RT_EINVAL, "frame too large for the 3x render");
  HIP_TRY(hipSetDevice(c->device));
  rt_camera big = *cam;
  big.width = 3 * cam->width;
  big.height = 3 * cam->height;
  rt_frame f;
  int rc = rt_frame_from_camera_any(&big, &f);
  if (rc) return rc;
  const size_t nhi = (size_t)big.width * big.height, nlo = (size_t)cam->width * cam->height;
  DevBuf<uint32_t> d_hi, d_lo;
  HIP_TRY(d_hi.alloc(nhi));
  if (d_lo.alloc(nlo) != hipSuccess) return rt_set_error(RT_EHIP, "hipMalloc image");
  hipStream_t s = c->stream;
  KParams p = scene_params(c);
  p.u = rt::f3{f.u.x, f.u.y, f.u.z};
  p.v = rt::f3{f.v.x, f.v.y, f.v.z};
  p.C = rt::f3{f.C.x, f.C.y, f.C.z};
  p.pos = rt::f3{f.position.x, f.position.y, f.position.z};
  p.W = big.width;
  p.H = big.height;
  p.tiles_x = tiles_x_of(big.width);
  p.ntiles_total = tiles_x_of(big.width) * tiles_y_of(big.height);
  p.nranks = 1;
  p.ntiles_local = p.ntiles_total;
  p.out = (float*)d_hi.get();
  p.tile_counter = c->d_counter;
  p.stats = c->d_stats;
  const int accel = (c->accel == RT_ACCEL_FLAT || !c->d_node) ? RT_ACCEL_FLAT_D : RT_ACCEL_OCTREE_D;
  rc = shadow_prepare(c, s);
  if (rc) return rc;
  if (c->exact_shadows) {
    p.node_mu = c->d_node_mu;
    p.sh_global = c->d_sh_global;
    p.n_sh_global = c->n_sh_global;
    p.sh_omax = c->sh_omax;
  }
  // exact camera rays in this mode too: the candidate lists of the 3x frame's
  // one-sample-per-pixel camera (csrc/rt_cand.h CandParams::compat)
  c->cand_prims = c->cand_entries = c->cand_global = 0;
  c->d_cand_valid = nullptr;
  if (c->accel == RT_ACCEL_OCTREE && c->d_node && c->exact_camera) {
    rc = cand_prepare(c, &f, &p, s, 1);
    if (rc) return rc;
  }
  c->cost_hist.valid = 0;  // the counters are the compat render's
  c->last_batch = 0;
  c->last_occl = 0;
  c->rl_valid = 0;         // (and no hit records are kept: nothing to relight)
  c->paths.drop("rt_hip_render_compat");
  c->relight.invalidate();
  if (hipMemsetAsync(c->d_counter, 0, kFrameCounterBytes, s) != hipSuccess ||
      rt_launch_compat(&p, accel, c->grid, s) != hipSuccess ||
      rt_launch_downscale(d_hi, d_lo, cam->width, cam->height, s) != hipSuccess ||
      hipMemcpyAsync(h_rgba, d_lo, nlo * sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = rt_set_error(RT_EHIP, "compat render: %s", hipGetErrorString(hipGetLastError()));
  c->last_stream = s;
  rt_stats tmp;
  if (!rc) rc = rt_hip_stats(c, st ? st : &tmp);
  if (st) st->camera = st->pixels;  // one camera ray per high-resolution pixel
  return rc;
}

// gpu/rt.cpp:56-97: `rt file.svati output.png` with gpu/rt's semantics
extern "C" int rt_raytrace_gpu(const char* input, const char* output, int accel) {
  rt_scene* scene = nullptr;
  int rc = rt_scene_load_svati(input, &scene);
  if (rc) return rc;
  if (accel < 0) accel = choose_accel(scene);
  rt_hip_ctx* ctx = nullptr;
  std::vector<unsigned char> img((size_t)4 * (scene->camera.width > 0 ? scene->camera.width : 0) *
                                 (scene->camera.height > 0 ? scene->camera.height : 0) + 4);
  rc = rt_hip_create(0, scene, accel, &ctx);
  if (!rc) rc = rt_hip_render_compat(ctx, &scene->camera, img.data(), nullptr);
  if (!rc) rc = rt_png_write_rgba(output, scene->camera.width, scene->camera.height, img.data());
  if (ctx) rt_hip_destroy(ctx);
  rt_scene_free(scene);
  return rc;
}

extern "C" int rt_hip_malloc(int device, size_t bytes, void** d_ptr) {
  if (!d_ptr) return rt_set_error(RT_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMalloc(d_ptr, bytes ? bytes : 16));
  return RT_OK;
}
extern "C" int rt_hip_free(void* d_ptr) {
  HIP_TRY(hipFree(d_ptr));
  return RT_OK;
}
extern "C" int rt_hip_memcpy_d2h(void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}
extern "C" int rt_hip_memcpy_h2d(void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return RT_OK;
}

extern "C" int rt_hip_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  if (!bytes) return RT_OK;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RT_OK;
}

// ------------------------------------------------------------ drop-in entry

int choose_accel(const rt_scene* s) {
  // brute force is exact and cheapest for tiny scenes; the host SAH octree
  // renders the reference's small scenes fastest (C3/C4); from ~10^5
  // triangles the device-built octree both builds (0.7 s vs 6 s) and renders
  // (C5: 19.0 vs 29.0 ms) faster
  size_t n = rt_scene_triangle_count(s);
  return n <= 64 ? RT_ACCEL_FLAT : (n < 100000 ? RT_ACCEL_OCTREE : RT_ACCEL_OCTREE_GPU);
}

extern "C" int rt_raytrace(const char* input, const char* output) {
  return rt_raytrace_multi(input, output, 1, -1, nullptr, nullptr);
}
