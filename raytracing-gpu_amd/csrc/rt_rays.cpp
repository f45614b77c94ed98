// rt_rays.cpp -- host side of the ray batches (include/rt_hip.h
// rt_hip_trace_rays, rt_hip_trace_rays_host, rt_hip_frame_rays): a batch's
// refusals, its share of the context's hit-record buffers, its kernels
// (csrc/rt_rays.h) and launches, in the steps of rt_hip_render (rt_hip.cpp).
// The item count, the buffers' sizing and the ray orders are csrc/rt_ray_items.h.
#include "rt_batch.h"  // the refusals every batch words alike

static_assert(RT_RAYS_MAX == RT_RAY_BATCH_MAX, "rt_hip.h states what a record index addresses");

// The refusals: nothing of the context has changed when one of them returns.
// (origins, dirs, rgb, samples: device pointers, or the host wrapper's)
static int rays_refuse(const rt_hip_ctx* c, const float* origins, const float* dirs, size_t n, unsigned flags,
                       const float* rgb, const void* samples) {
  if (int rc = batch_refuse_ctx(c)) return rc;
  if (!rgb && !samples) return rt_set_error(RT_EINVAL, "a ray batch needs a colour or a sample output");
  if (n && (!origins || !dirs)) return rt_set_error(RT_EINVAL, "null rays");
  if (n > RT_RAYS_MAX)
    return rt_set_error(RT_EINVAL, "%zu rays: a hit record's index addresses %llu", n, (unsigned long long)RT_RAYS_MAX);
  return batch_refuse_mode(c, flags, "a ", "ray batch");
}

extern "C" int rt_hip_trace_rays(rt_hip_ctx* c, const float* d_origins, const float* d_dirs, size_t n,
                                 unsigned flags, float* d_rgb, void* d_samples, void* stream) {
  int rc = rays_refuse(c, d_origins, d_dirs, n, flags, d_rgb, d_samples);
  if (!rc && ((uintptr_t)d_samples & 7)) rc = rt_set_error(RT_EINVAL, "ray samples must be 8-byte aligned");
  if (rc || n == 0) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // the batch overwrites the kept frame's hit records and capture
  c->gb_valid = 0;
  c->rl_valid = 0;
  c->relight.invalidate();
  c->paths.drop(d_rgb ? "a newer rt_hip_trace_rays" : "a ray cast (rt_hip_trace_rays without d_rgb)");
  KParams p = scene_params(c);
  p.tile_counter = c->d_counter;
  p.stats = c->d_stats;
  RayArgs a;
  std::memset(&a, 0, sizeof a);
  a.org = d_origins;
  a.dir = d_dirs;
  a.n = n;
  a.nitems = rt_ray_item_count(n);
  a.rgb = d_rgb;
  a.samples = (uint32_t*)d_samples;
  const bool cast = !d_rgb;
  // buffers, sized by items: two records per ray at first, as frames get
  if ((rc = hit_buffers(c, a.nitems, d_samples != nullptr))) return rc;
  hit_views(c, p);
  if (d_samples) p.capture = c->d_capture;
  RenderKernels k;
  if ((rc = render_shadows(c, p, s)) || (rc = render_kernels(c, p, a.nitems, s, &k))) return rc;
  // the batch's trace: the ray policies' instantiation, its grid clamped to the items
  const int tpol = d_samples ? RT_POLICY_RAYS_GB : RT_POLICY_RAYS;
  const bool octree = k.dacc == RT_ACCEL_OCTREE_D;
  int gt = (c->accel == RT_ACCEL_OCTREE && !c->d_node) ? c->grid : c->grid_of[1][tpol][0];
  if ((long long)a.nitems < gt) gt = (int)a.nitems;
  if (octree && c->exact_refl)
    a.walk |= RT_RAYS_WALK_EXACT;  // (render_kernels built the bounds: p.node_rf)
  else if (octree && (flags & RT_RAYS_PACKET))
    a.walk |= RT_RAYS_WALK_PACKET;
  if (cast) a.walk |= RT_RAYS_WALK_CAST;
  // every device pointer the kernels will follow must exist (a null one
  // would fault the card, not fail the call)
  if (!p.tri_prim && (p.lbuf || p.n_sh_global || (d_samples && p.nrec)))
    return rt_set_error(RT_EHIP, "ray batch: prim-order records missing");
  if (!p.hit || !p.hit_prev || !p.hit_term || !p.hit_count || !p.shade_counter || !p.last || !p.stats ||
      !p.tile_counter || (p.nlight && (!p.light || !p.lshade)) ||
      (p.nrec && (!p.tri || !p.nrm || !p.mat || !p.mshade)) || (d_samples && !p.capture) || gt <= 0 || k.gs <= 0)
    return rt_set_error(RT_EHIP, "ray batch: device buffers missing");
  if (octree && (!p.node || !p.spill || ((a.walk & RT_RAYS_WALK_EXACT) && !p.node_rf)))
    return rt_set_error(RT_EHIP, "ray batch: octree buffers missing");
  if (!c->d_frame_check) {
    HIP_TRY(c->d_frame_check.alloc(4));
    HIP_TRY(hipMemsetAsync(c->d_frame_check, 0, 4 * sizeof(unsigned long long), s));
  }
  p.frame_check = c->d_frame_check;
  // item streams, stats, record counters -- not the last frame's item-clock
  // sum behind them, which the next frame's work order may still read
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, kFrameCounterBytes - kCostBytes, s));
  HIP_TRY(rt_launch_rays_trace(&p, &a, k.dacc, tpol, gt, s));
  if (!cast) {
    HIP_TRY(rt_launch_shade(&p, k.dacc, 0, k.spol, k.gs, s));
    HIP_TRY(rt_launch_shade_fixup(&p, c->nprim, s));
  }
  HIP_TRY(rt_launch_rays_fold(&p, &a, s));
  if (d_samples) HIP_TRY(rt_launch_rays_samples(&p, &a, s));
  // what rt_hip_stats reads afterwards; no list, timing event or work-order
  // history of the frames around the batch is touched
  c->last_p = p;
  c->last_batch = 1;
  c->last_occl = 0;
  c->last_stream = s;
  if (!cast) c->paths.keep(n, s);  // rt_hip_path_records exports this batch's paths
  return RT_OK;
}

extern "C" int rt_hip_trace_rays_host(rt_hip_ctx* c, const float* h_origins, const float* h_dirs, size_t n,
                                      unsigned flags, float* h_rgb, rt_gsample* h_samples, rt_stats* st) {
  int rc = rays_refuse(c, h_origins, h_dirs, n, flags, h_rgb, h_samples);
  if (rc) return rc;
  if (n == 0) return batch_host_none(st);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<float> d_o, d_d, d_rgb;
  DevBuf<uint32_t> d_smp;
  if (d_o.alloc(3 * n) != hipSuccess || d_d.alloc(3 * n) != hipSuccess ||
      (h_rgb && d_rgb.alloc(3 * n) != hipSuccess) || (h_samples && d_smp.alloc(RT_GB_WORDS * n) != hipSuccess))
    return rt_set_error(RT_EHIP, "hipMalloc ray batch");
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_o, h_origins, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_d, h_dirs, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  rt_stats tmp;
  for (int attempt = 0; attempt < 2; attempt++) {  // again after the hit buffers grew
    rc = rt_hip_trace_rays(c, d_o, d_d, n, flags, h_rgb ? d_rgb.get() : nullptr,
                           h_samples ? (void*)d_smp.get() : nullptr, nullptr);
    if (!rc && h_rgb && hipMemcpyAsync(h_rgb, d_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess)
      rc = rt_set_error(RT_EHIP, "D2H ray colours");
    if (!rc && h_samples &&
        hipMemcpyAsync(h_samples, d_smp, n * sizeof(rt_gsample), hipMemcpyDeviceToHost, s) != hipSuccess)
      rc = rt_set_error(RT_EHIP, "D2H ray samples");
    if (!rc) rc = rt_hip_stats(c, st ? st : &tmp);  // (synchronises)
    if (rc != RT_EHITBUF) break;
  }
  (void)hipStreamSynchronize(s);  // the buffers above go
  return rc;
}

extern "C" int rt_hip_frame_rays(rt_hip_ctx* c, const rt_frame* f, int order, float* d_origins, float* d_dirs,
                                 void* stream) {
  if (!c || !f || !d_origins || !d_dirs) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (f->width <= 0 || f->height <= 0) return rt_set_error(RT_EINVAL, "empty frame");
  if ((f->width | f->height) & 1)
    return rt_set_error(RT_EINVAL, "frame %dx%d: cpu/rt renders even sizes only", f->width, f->height);
  if (order != 0 && order != 1) return rt_set_error(RT_EINVAL, "unknown ray order %d", order);
  if (order == 1 && ((f->width | f->height) & 3))
    return rt_set_error(RT_EINVAL, "frame %dx%d: quarter order needs multiples of 4", f->width, f->height);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  KParams p;
  std::memset(&p, 0, sizeof p);
  p.u = rt::f3{f->u.x, f->u.y, f->u.z};
  p.v = rt::f3{f->v.x, f->v.y, f->v.z};
  p.C = rt::f3{f->C.x, f->C.y, f->C.z};
  p.pos = rt::f3{f->position.x, f->position.y, f->position.z};
  p.W = f->width;
  p.H = f->height;
  HIP_TRY(rt_launch_frame_rays(&p, order, d_origins, d_dirs, s));
  return RT_OK;
}

extern "C" int rt_hip_frame_rays_host(rt_hip_ctx* c, const rt_frame* f, int order, float* h_origins, float* h_dirs) {
  if (!c || !f || !h_origins || !h_dirs) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (f->width <= 0 || f->height <= 0) return rt_set_error(RT_EINVAL, "empty frame");
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = 12 * (size_t)f->width * (size_t)f->height;  // floats of 4 W H rays
  DevBuf<float> d_o, d_d;
  if (d_o.alloc(n) != hipSuccess || d_d.alloc(n) != hipSuccess) return rt_set_error(RT_EHIP, "hipMalloc camera rays");
  const int rc = rt_hip_frame_rays(c, f, order, d_o, d_d, nullptr);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h_origins, d_o, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(h_dirs, d_d, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RT_OK;
}
