// rt_occl.cpp -- host side of the occlusion batches (include/rt_hip.h
// rt_hip_occluded, rt_hip_occluded_host): a batch's refusals, its argument
// block and the launch of its kernel (csrc/rt_occl.h) through the batches' one
// host path (csrc/rt_batch.h), which also says what a batch leaves as it is.
// Which rays are traced and the tmax -> t_cut bound: csrc/rt_occl_items.h.
#include "rt_batch.h"
#include "rt_occl_items.h"

// The refusals: nothing of the context has changed when one of them returns.
static int occl_refuse(const rt_hip_ctx* c, const float* origins, const float* dirs, size_t n, unsigned flags,
                       const unsigned char* out) {
  int rc = batch_refuse_ctx(c);
  if (!rc) rc = batch_refuse_size(n, "rays");
  if (rc) return rc;
  if (n && (!origins || !dirs)) return rt_set_error(RT_EINVAL, "null rays");
  if (n && !out) return rt_set_error(RT_EINVAL, "null occlusion output");
  return batch_refuse_mode(c, flags, "an ", "occlusion batch");
}

extern "C" int rt_hip_occluded(rt_hip_ctx* c, const float* d_origins, const float* d_dirs, const float* d_tmax,
                               size_t n, unsigned flags, unsigned char* d_occluded, void* stream) {
  int rc = occl_refuse(c, d_origins, d_dirs, n, flags, d_occluded);
  if (rc || n == 0) return rc;
  OcclArgs a;
  std::memset(&a, 0, sizeof a);
  a.org = d_origins;
  a.dir = d_dirs;
  a.tmax = d_tmax;
  a.n = n;
  a.nitems = rt_ray_item_count(n);
  a.out = d_occluded;
  BatchLaunch b;
  if ((rc = batch_begin(c, stream, flags, RT_BATCH_OCCL, a.nitems, false, "occlusion batch", &b))) return rc;
  a.walk = b.walk;
  if ((a.walk & RT_RAYS_WALK_EXACT) && !b.p.tri_prim)  // the winner's flag is read from its prim-order record
    return rt_set_error(RT_EHIP, "occlusion batch: octree buffers missing");
  return batch_run(c, b, &a);
}

extern "C" int rt_hip_occluded_host(rt_hip_ctx* c, const float* h_origins, const float* h_dirs, const float* h_tmax,
                                    size_t n, unsigned flags, unsigned char* h_occluded, rt_stats* st) {
  int rc = occl_refuse(c, h_origins, h_dirs, n, flags, h_occluded);
  if (rc) return rc;
  if (n == 0) return batch_host_none(st);
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
  rc = rt_hip_occluded(c, d_o, d_d, h_tmax ? d_t.get() : nullptr, n, flags, d_out, nullptr);
  if (!rc && hipMemcpyAsync(h_occluded, d_out, n, hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = rt_set_error(RT_EHIP, "D2H occlusion bytes");
  return batch_host_end(c, rc, st);
}
