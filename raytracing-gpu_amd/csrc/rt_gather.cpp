// rt_gather.cpp -- host side of the gather (include/rt_hip.h rt_hip_gather,
// rt_hip_gather_host): the refusals, the gather's share of the context's
// hit-record buffers, its kernels (csrc/rt_gather.h) and launches.  To the
// context a gather is a ray batch (csrc/rt_rays.cpp): the same steps in the
// same order, with the rays made in the trace from records by ambient
// occlusion's rule (csrc/rt_ao_items.h) and k paths folded per record.  The
// slots and the buffers' sizing are csrc/rt_gather_items.h.
#include "rt_batch.h"  // the refusals every batch words alike
#include "rt_gather_items.h"

// The refusals: nothing of the context has changed when one of them returns.
// (samples, table, rgb: device pointers, or the host wrapper's)
static int gather_refuse(const rt_hip_ctx* c, const void* samples, size_t n, unsigned k, const float* table,
                         unsigned m, unsigned flags, const float* rgb) {
  int rc = ao_refuse(c, n, k, m);
  if (!rc && n && (!samples || !table)) rc = rt_set_error(RT_EINVAL, "null samples or table");
  if (!rc && n && !rgb) rc = rt_set_error(RT_EINVAL, "null gather output");
  if (!rc) rc = batch_refuse_mode(c, flags, "a ", "gather");
  return rc;
}

extern "C" int rt_hip_gather(rt_hip_ctx* c, const void* d_samples, size_t n, unsigned long long base, unsigned k,
                             const float* d_table, unsigned m, unsigned seed, unsigned flags, float* d_rgb,
                             void* stream) {
  int rc = gather_refuse(c, d_samples, n, k, d_table, m, flags, d_rgb);
  if (!rc) rc = ao_refuse_ptrs(d_samples, n, d_table);
  if (rc || n == 0) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // the gather overwrites the kept frame's hit records and capture
  c->gb_valid = 0;
  c->rl_valid = 0;
  c->relight.invalidate();
  c->paths.drop("rt_hip_gather");
  KParams p = scene_params(c);
  p.tile_counter = c->d_counter;
  p.stats = c->d_stats;
  GatherArgs a;
  std::memset(&a, 0, sizeof a);
  a.ao.samples = (const uint2*)d_samples;
  a.ao.n = n;
  a.ao.base = base;
  a.ao.table = d_table;
  a.ao.k = k;
  a.ao.m = m;
  a.ao.seed = seed;
  a.ao.spi = rt_ao_spi(k);
  a.ao.kinv = rt_ao_kinv(k);
  a.ao.nitems = (uint32_t)rt_gather_item_count(n, k);
  a.rgb = d_rgb;
  // buffers, sized by the groups of 64 paths: two records per path at first,
  // as frames get; a `last` slot for every lane of every (item, round)
  if ((rc = hit_buffers(c, (size_t)rt_gather_path_groups(n, k), false))) return rc;
  hit_views(c, p);
  RenderKernels rk;
  if ((rc = render_shadows(c, p, s)) || (rc = render_kernels(c, p, a.ao.nitems, s, &rk))) return rc;
  // the gather's trace: its own instantiation's grid, held by the spill area
  // and clamped to the items
  const bool octree = rk.dacc == RT_ACCEL_OCTREE_D;
  const int wide = k > 64 ? 1 : 0;  // k > 64: its own kernel (csrc/rt_gather.h)
  int& cached = c->gather_grid[rk.dacc][wide];
  if (!cached) HIP_TRY(rt_gather_grid(rk.dacc, wide, c->cus, &cached));
  int gt = cached;
  if (octree) gt = (int)std::min<size_t>((size_t)gt, c->d_spill.cap() / ((size_t)64 * RT_SPILL_STACK));
  if ((long long)a.ao.nitems < gt) gt = (int)a.ao.nitems;
  if (octree && c->exact_refl)
    a.ao.walk |= RT_RAYS_WALK_EXACT;  // (render_kernels built the bounds: p.node_rf)
  else if (octree && (flags & RT_RAYS_PACKET))
    a.ao.walk |= RT_RAYS_WALK_PACKET;
  // every device pointer the kernels will follow must exist (a null one
  // would fault the card, not fail the call)
  if (!p.tri_prim && (p.lbuf || p.n_sh_global))
    return rt_set_error(RT_EHIP, "gather: prim-order records missing");
  if (!p.hit || !p.hit_prev || !p.hit_term || !p.hit_count || !p.shade_counter || !p.last || !p.stats ||
      !p.tile_counter || (p.nlight && (!p.light || !p.lshade)) ||
      (p.nrec && (!p.tri || !p.nrm || !p.mat || !p.mshade)) || gt <= 0 || rk.gs <= 0 ||
      !c->d_last.holds((size_t)rt_gather_slot_count(n, k)))
    return rt_set_error(RT_EHIP, "gather: device buffers missing");
  if (octree && (!p.node || !p.spill || ((a.ao.walk & RT_RAYS_WALK_EXACT) && !p.node_rf)))
    return rt_set_error(RT_EHIP, "gather: octree buffers missing");
  if (!c->d_frame_check) {
    HIP_TRY(c->d_frame_check.alloc(4));
    HIP_TRY(hipMemsetAsync(c->d_frame_check, 0, 4 * sizeof(unsigned long long), s));
  }
  p.frame_check = c->d_frame_check;
  // item streams, stats, record counters -- not the last frame's item-clock
  // sum behind them, which the next frame's work order may still read
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, kFrameCounterBytes - kCostBytes, s));
  HIP_TRY(rt_launch_gather_trace(&p, &a, rk.dacc, gt, s));
  HIP_TRY(rt_launch_shade(&p, rk.dacc, 0, rk.spol, rk.gs, s));
  HIP_TRY(rt_launch_shade_fixup(&p, c->nprim, s));
  HIP_TRY(rt_launch_gather_fold(&p, &a, s));
  // what rt_hip_stats reads afterwards: a ray batch's; no list, timing event
  // or work-order history of the frames around the gather is touched
  c->last_p = p;
  c->last_batch = 1;
  c->last_occl = 0;
  c->last_stream = s;
  return RT_OK;
}

extern "C" int rt_hip_gather_host(rt_hip_ctx* c, const rt_gsample* h_samples, size_t n, unsigned long long base,
                                  unsigned k, const float* h_table, unsigned m, unsigned seed, unsigned flags,
                                  float* h_rgb, rt_stats* st) {
  int rc = gather_refuse(c, h_samples, n, k, h_table, m, flags, h_rgb);
  if (rc) return rc;
  if (n == 0) return batch_host_none(st);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<rt_gsample> d_s;
  DevBuf<float> d_t, d_rgb;
  if (d_s.alloc(n) != hipSuccess || d_t.alloc(3 * (size_t)m) != hipSuccess || d_rgb.alloc(3 * n) != hipSuccess)
    return rt_set_error(RT_EHIP, "hipMalloc gather");
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_s, h_samples, n * sizeof(rt_gsample), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_t, h_table, 3 * (size_t)m * sizeof(float), hipMemcpyHostToDevice, s));
  rt_stats tmp;
  for (int attempt = 0; attempt < 2; attempt++) {  // again after the hit buffers grew
    rc = rt_hip_gather(c, d_s.get(), n, base, k, d_t.get(), m, seed, flags, d_rgb.get(), nullptr);
    if (!rc && hipMemcpyAsync(h_rgb, d_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess)
      rc = rt_set_error(RT_EHIP, "D2H gather sums");
    if (!rc) rc = rt_hip_stats(c, st ? st : &tmp);  // (synchronises)
    if (rc != RT_EHITBUF) break;
  }
  (void)hipStreamSynchronize(s);  // the buffers above go
  return rc;
}
