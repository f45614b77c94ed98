// rt_occl.cpp -- host side of the occlusion batches (include/rt_hip.h
// rt_hip_occluded, rt_hip_occluded_host): a batch's refusals, its kernel
// (csrc/rt_occl.h) and launch, its own stats block and what rt_hip_stats reads
// from it.  A batch writes no hit record and no capture: the kept frame's
// records, its relight plan and G-buffer validity, the list buffers, the
// overlap state, the frame check and the render's counters stay as they are.
// It uses the context's stack spill area and item counters, in stream order.
// Which rays are traced and the tmax -> t_cut bound: csrc/rt_occl_items.h.
#include "rt_ctx.h"
#include "rt_occl_items.h"

// The refusals: nothing of the context has changed when one of them returns.
static int occl_refuse(const rt_hip_ctx* c, const float* origins, const float* dirs, size_t n, unsigned flags,
                       const unsigned char* out) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  if (n > RT_RAYS_MAX)
    return rt_set_error(RT_EINVAL, "%zu rays: a batch holds at most %llu", n, (unsigned long long)RT_RAYS_MAX);
  if (n && (!origins || !dirs)) return rt_set_error(RT_EINVAL, "null rays");
  if (n && !out) return rt_set_error(RT_EINVAL, "null occlusion output");
  if (flags & ~RT_RAYS_PACKET) return rt_set_error(RT_EINVAL, "unknown occlusion batch flags %#x", flags);
  if (c->policy != RT_POLICY_DEFAULT)
    return rt_set_error(RT_EINVAL, "an occlusion batch needs the default traversal policy (have %d)", c->policy);
  if (c->count_work) return rt_set_error(RT_EINVAL, "an occlusion batch cannot run as the work-counting pass");
  return RT_OK;
}

extern "C" int rt_hip_occluded(rt_hip_ctx* c, const float* d_origins, const float* d_dirs, const float* d_tmax,
                               size_t n, unsigned flags, unsigned char* d_occluded, void* stream) {
  int rc = occl_refuse(c, d_origins, d_dirs, n, flags, d_occluded);
  if (rc || n == 0) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // an empty octree scene has nothing to traverse: the FLAT kernel with 0 records
  const bool empty = c->accel == RT_ACCEL_OCTREE && !c->d_node;
  const int dacc = (c->accel == RT_ACCEL_FLAT || empty) ? RT_ACCEL_FLAT_D : RT_ACCEL_OCTREE_D;
  const bool octree = dacc == RT_ACCEL_OCTREE_D;
  KParams p = scene_params(c);
  OcclArgs a;
  std::memset(&a, 0, sizeof a);
  a.org = d_origins;
  a.dir = d_dirs;
  a.tmax = d_tmax;
  a.n = n;
  a.nitems = rt_ray_item_count(n);
  a.out = d_occluded;
  if (octree && c->exact_refl) {  // the proven closest walk and its bounds
    if ((rc = reflect_prepare(c, s))) return rc;
    p.node_rf = c->d_node_rf;
    a.walk = RT_RAYS_WALK_EXACT;
  } else if (octree && (flags & RT_RAYS_PACKET)) {
    a.walk = RT_RAYS_WALK_PACKET;
  }
  // the batch's own stats block and the kernel's grid
  if (!c->d_occl_stats) HIP_TRY(c->d_occl_stats.alloc(RT_STAT_SETS * RT_STAT_STRIDE));
  if (!c->occl_grid) {
    int g = 0;
    HIP_TRY(rt_occl_grid(dacc, c->cus, &g));
    c->occl_grid = g;
  }
  int grid = c->occl_grid;
  // the spill area holds [entry][lane] for so many one-wave workgroups
  if (octree) grid = (int)std::min<size_t>((size_t)grid, c->d_spill.cap() / ((size_t)64 * RT_SPILL_STACK));
  if ((long long)a.nitems < grid) grid = (int)a.nitems;
  p.tile_counter = c->d_counter;
  p.stats = c->d_occl_stats;
  // every device pointer the kernel follows must exist (a null one would
  // fault the card, not fail the call)
  if (!p.tile_counter || !p.stats || grid <= 0 || (p.nrec && !p.tri))
    return rt_set_error(RT_EHIP, "occlusion batch: device buffers missing");
  if (octree && (!p.node || !p.spill || !p.tri || ((a.walk & RT_RAYS_WALK_EXACT) && (!p.node_rf || !p.tri_prim))))
    return rt_set_error(RT_EHIP, "occlusion batch: octree buffers missing");
  // the item streams' counters and the batch's stats: not the render's stats,
  // record counters or item-clock sum behind the item counters
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, kItemCounterBytes, s));
  HIP_TRY(hipMemsetAsync(c->d_occl_stats, 0, kStatBytes, s));
  HIP_TRY(rt_launch_occl(&p, &a, dacc, grid, s));
  c->last_occl = 1;  // what rt_hip_stats reads next
  c->occl_stream = s;
  return RT_OK;
}

// rt_hip_stats directly after an occlusion batch: the batch's own counters.
int occl_stats(rt_hip_ctx* c, rt_stats* out) {
  unsigned long long hs[RT_STAT_SETS * RT_STAT_STRIDE], h[RT_NSTATS];
  hipStream_t s = c->occl_stream ? c->occl_stream : c->stream;
  HIP_TRY(hipMemcpyAsync(hs, c->d_occl_stats, sizeof hs, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < RT_NSTATS; k++) {
    h[k] = 0;
    for (int set = 0; set < RT_STAT_SETS; set++) h[k] += hs[set * RT_STAT_STRIDE + k];
  }
  std::memset(out, 0, sizeof *out);
  out->camera = h[RT_ST_PIXELS];  // the rays traced, counted in the pixels' slot
  out->shadow = h[RT_ST_SHADOW];  // the queries
  out->depth_overflow = h[RT_ST_DEPTH_OVERFLOW];
  out->shadow_zero_risk = h[RT_ST_SHADOW_ZERO_RISK];
  out->closest_unproven = h[RT_ST_CLOSEST_UNPROVEN];
  // direct light for records (csrc/rt_dlight.h) counts its queries off a light buffer's proof box in the
  // hits' slot, which no walk of a batch adds to: 0 after every other batch
  out->shadow_deferred = h[RT_ST_HITS];
  if (out->depth_overflow)
    return rt_set_error(RT_EDEPTH, "%llu occlusion queries overflowed a traversal stack", out->depth_overflow);
  if (out->shadow_zero_risk)
    return rt_set_error(RT_EZERONORMAL,
                        "%llu occlusion rays hit an object whose interpolated normal can vanish "
                        "(cpu/hit.c:99 may skip it; early any-hit exit not proven exact)",
                        out->shadow_zero_risk);
  if (out->closest_unproven)
    return rt_set_error(RT_EINEXACT,
                        "%llu occlusion rays with |d| past the exact reflection walk's bound "
                        "(csrc/rt_reflect.h RT_RF_DLMAX)", out->closest_unproven);
  return RT_OK;
}

extern "C" int rt_hip_occluded_host(rt_hip_ctx* c, const float* h_origins, const float* h_dirs, const float* h_tmax,
                                    size_t n, unsigned flags, unsigned char* h_occluded, rt_stats* st) {
  int rc = occl_refuse(c, h_origins, h_dirs, n, flags, h_occluded);
  if (rc) return rc;
  if (n == 0) {  // nothing launched, nothing written
    if (st) std::memset(st, 0, sizeof *st);
    return RT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<float> d_o, d_d, d_t;
  DevBuf<unsigned char> d_out;
  if (d_o.alloc(3 * n) != hipSuccess || d_d.alloc(3 * n) != hipSuccess || (h_tmax && d_t.alloc(n) != hipSuccess) ||
      d_out.alloc(n) != hipSuccess)
    return rt_set_error(RT_EHIP, "hipMalloc occlusion batch");
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_o, h_origins, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_d, h_dirs, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  if (h_tmax) HIP_TRY(hipMemcpyAsync(d_t, h_tmax, n * sizeof(float), hipMemcpyHostToDevice, s));
  rt_stats tmp;
  rc = rt_hip_occluded(c, d_o, d_d, h_tmax ? d_t.get() : nullptr, n, flags, d_out, nullptr);
  if (!rc && hipMemcpyAsync(h_occluded, d_out, n, hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = rt_set_error(RT_EHIP, "D2H occlusion bytes");
  if (!rc) rc = rt_hip_stats(c, st ? st : &tmp);  // (synchronises)
  (void)hipStreamSynchronize(s);  // the buffers above go
  return rc;
}
