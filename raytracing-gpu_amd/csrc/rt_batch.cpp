// rt_batch.cpp -- the one host path of the batches that count into the batch
// stats block (csrc/rt_batch.h): their common refusals, their launch sequence
// and the stats rt_hip_stats reads after one of them.
#include "rt_batch.h"

int batch_refuse_ctx(const rt_hip_ctx* c) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  return ctx_live(c);
}

int batch_refuse_size(size_t n, const char* things) {
  if (n > RT_RAYS_MAX)
    return rt_set_error(RT_EINVAL, "%zu %s: a batch holds at most %llu", n, things, (unsigned long long)RT_RAYS_MAX);
  return RT_OK;
}

int batch_refuse_mode(const rt_hip_ctx* c, unsigned flags, const char* a, const char* noun) {
  if (flags & ~RT_RAYS_PACKET) return rt_set_error(RT_EINVAL, "unknown %s flags %#x", noun, flags);
  // a batch's walks exist for the default kernels only, like the G-buffer's
  if (c->policy != RT_POLICY_DEFAULT)
    return rt_set_error(RT_EINVAL, "%s%s needs the default traversal policy (have %d)", a, noun, c->policy);
  if (c->count_work) return rt_set_error(RT_EINVAL, "%s%s cannot run as the work-counting pass", a, noun);
  return RT_OK;
}

int batch_begin(rt_hip_ctx* c, void* stream, unsigned flags, int kind, uint32_t nitems, bool lbuf, const char* noun,
                BatchLaunch* b) {
  HIP_TRY(hipSetDevice(c->device));
  b->s = stream ? (hipStream_t)stream : c->stream;
  b->kind = kind;
  // an empty octree scene has nothing to traverse: the FLAT kernel with 0 records
  const bool empty = c->accel == RT_ACCEL_OCTREE && !c->d_node;
  b->dacc = (c->accel == RT_ACCEL_FLAT || empty) ? RT_ACCEL_FLAT_D : RT_ACCEL_OCTREE_D;
  b->octree = b->dacc == RT_ACCEL_OCTREE_D;
  b->walk = 0;
  KParams& p = b->p;
  p = scene_params(c);
  int rc;
  if (b->octree && lbuf) {
    // the light buffers, as a render has them (a no-op unless the slack or the
    // exact-shadow mode changed; none with rt_hip_set_light_buffers off).  It
    // changes nothing scene_params reads
    if ((rc = lbuf_prepare(c, b->s))) return rc;
    // (one descriptor per light, or none: the kernel indexes them by light)
    p.lbuf = c->lb_host.size() == c->nlight ? c->d_lbuf.get() : nullptr;
  }
  if (b->octree && c->exact_refl) {  // the proven closest walk and its bounds
    if ((rc = reflect_prepare(c, b->s))) return rc;
    p.node_rf = c->d_node_rf;
    b->walk = RT_RAYS_WALK_EXACT;
  } else if (b->octree && (flags & RT_RAYS_PACKET)) {
    b->walk = RT_RAYS_WALK_PACKET;
  }
  // the batches' stats block and the kernel's own grid.  The occupancy answer
  // is kept per (kind, FLAT or octree): a context whose octree scene is empty
  // now and gains geometry later (rt_hip_set_triangles) changes kernels
  if (!c->d_occl_stats) HIP_TRY(c->d_occl_stats.alloc(RT_STAT_SETS * RT_STAT_STRIDE));
  int& cached = c->batch_grid[kind][b->dacc];
  if (!cached) HIP_TRY(rt_batch_grid(kind, b->dacc, c->cus, &cached));
  b->grid = cached;
  // the spill area holds [entry][lane] for so many one-wave workgroups
  if (b->octree) b->grid = (int)std::min<size_t>((size_t)b->grid, c->d_spill.cap() / ((size_t)64 * RT_SPILL_STACK));
  if ((long long)nitems < b->grid) b->grid = (int)nitems;
  p.tile_counter = c->d_counter;
  p.stats = c->d_occl_stats;
  // every device pointer the kernel follows must exist (a null one would
  // fault the card, not fail the call)
  if (!p.tile_counter || !p.stats || b->grid <= 0 || (p.nrec && !p.tri))
    return rt_set_error(RT_EHIP, "%s: device buffers missing", noun);
  if (b->octree && (!p.node || !p.spill || !p.tri || ((b->walk & RT_RAYS_WALK_EXACT) && !p.node_rf)))
    return rt_set_error(RT_EHIP, "%s: octree buffers missing", noun);
  return RT_OK;
}

int batch_run(rt_hip_ctx* c, const BatchLaunch& b, const void* args) {
  // the item streams' counters and the batches' stats: not the render's stats,
  // record counters or item-clock sum behind the item counters
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, kItemCounterBytes, b.s));
  HIP_TRY(hipMemsetAsync(c->d_occl_stats, 0, kStatBytes, b.s));
  HIP_TRY(rt_launch_batch(&b.p, args, b.kind, b.dacc, b.grid, b.s));
  c->last_occl = 1;  // what rt_hip_stats reads next
  c->occl_stream = b.s;
  return RT_OK;
}

// rt_hip_stats directly after such a batch: the batch's own counters.
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
