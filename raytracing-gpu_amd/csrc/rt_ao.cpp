// rt_ao.cpp -- host side of ambient occlusion from G-buffer records
// (include/rt_hip.h rt_hip_ambient_occlusion, rt_hip_ambient_occlusion_host,
// rt_hip_ao_rays, rt_hip_ao_rays_host): the refusals, the fused kernel's launch (csrc/rt_ao.h) and
// the generator's.  To the context a counting call is a batch of the one host
// path (csrc/rt_batch.h), which says what it uses and what it leaves as it is.
// The ray rule and the items: csrc/rt_ao_items.h.
#include "rt_batch.h"
#include "rt_ao_items.h"

static_assert(RT_AO_KMAX == RT_AO_KMAX_D, "include/rt_hip.h and csrc/rt_ao_items.h disagree on k's limit");

// What the entry points (and a gather's, csrc/rt_gather.cpp: declared in
// rt_batch.h) refuse alike, by the sizes alone; nothing of the context has
// changed when a refusal returns.
int ao_refuse(const rt_hip_ctx* c, size_t n, unsigned k, unsigned m) {
  if (int rc = batch_refuse_ctx(c)) return rc;
  if (k == 0 || k > RT_AO_KMAX) return rt_set_error(RT_EINVAL, "%u rays per sample: 1 to %u", k, (unsigned)RT_AO_KMAX);
  if (m == 0) return rt_set_error(RT_EINVAL, "an empty direction table");
  if (n > RT_RAYS_MAX / k)
    return rt_set_error(RT_EINVAL, "%zu samples x %u rays: a batch holds at most %llu rays", n, k,
                        (unsigned long long)RT_RAYS_MAX);
  if (rt_ao_item_count(n, k) > 0xfffffff8ull)
    return rt_set_error(RT_EINVAL, "%zu samples x %u rays: more work items than the streams address", n, k);
  return RT_OK;
}
// ... and the records and table in device memory
int ao_refuse_ptrs(const void* d_samples, size_t n, const float* d_table) {
  if (n && (!d_samples || !d_table)) return rt_set_error(RT_EINVAL, "null samples or table");
  if ((uintptr_t)d_samples & 7u) return rt_set_error(RT_EINVAL, "samples must be 8-byte aligned");
  return RT_OK;
}

static AoArgs ao_args(const void* d_samples, size_t n, unsigned long long base, unsigned k, const float* d_table,
                      unsigned m, unsigned seed) {
  AoArgs a;
  std::memset(&a, 0, sizeof a);
  a.samples = (const uint2*)d_samples;
  a.n = n;
  a.base = base;
  a.table = d_table;
  a.k = k;
  a.m = m;
  a.seed = seed;
  a.spi = rt_ao_spi(k);
  a.kinv = rt_ao_kinv(k);
  a.nitems = (uint32_t)rt_ao_item_count(n, k);
  return a;
}

extern "C" int rt_hip_ambient_occlusion(rt_hip_ctx* c, const void* d_samples, size_t n, unsigned long long base,
                                        unsigned k, const float* d_table, unsigned m, unsigned seed, float tmax,
                                        unsigned flags, unsigned* d_occluded, void* stream) {
  int rc = ao_refuse(c, n, k, m);
  if (!rc) rc = ao_refuse_ptrs(d_samples, n, d_table);
  if (!rc && n && !d_occluded) rc = rt_set_error(RT_EINVAL, "null occlusion output");
  if (!rc) rc = batch_refuse_mode(c, flags, "", "ambient occlusion");
  if (rc || n == 0) return rc;
  AoArgs a = ao_args(d_samples, n, base, k, d_table, m, seed);
  a.tmax = tmax;
  a.out = d_occluded;
  BatchLaunch b;
  const int kind = k > 64 ? RT_BATCH_AO_WIDE : RT_BATCH_AO;  // k > 64: its own kernel (csrc/rt_ao.h)
  if ((rc = batch_begin(c, stream, flags, kind, a.nitems, false, "ambient occlusion", &b))) return rc;
  a.walk = b.walk;
  if ((a.walk & RT_RAYS_WALK_EXACT) && !b.p.tri_prim)  // the winner's flag is read from its prim-order record
    return rt_set_error(RT_EHIP, "ambient occlusion: octree buffers missing");
  return batch_run(c, b, &a);
}

extern "C" int rt_hip_ao_rays(rt_hip_ctx* c, const void* d_samples, size_t n, unsigned long long base, unsigned k,
                              const float* d_table, unsigned m, unsigned seed, float* d_origins, float* d_dirs,
                              unsigned char* d_shot, void* stream) {
  int rc = ao_refuse(c, n, k, m);
  if (!rc) rc = ao_refuse_ptrs(d_samples, n, d_table);
  if (!rc && n && (!d_origins || !d_dirs)) rc = rt_set_error(RT_EINVAL, "null ray output");
  if (rc || n == 0) return rc;
  HIP_TRY(hipSetDevice(c->device));
  AoArgs a = ao_args(d_samples, n, base, k, d_table, m, seed);
  a.org = d_origins;
  a.dir = d_dirs;
  a.shot = d_shot;
  HIP_TRY(rt_launch_ao_rays(&a, stream ? (hipStream_t)stream : c->stream));
  return RT_OK;
}

extern "C" int rt_hip_ao_rays_host(rt_hip_ctx* c, const rt_gsample* h_samples, size_t n, unsigned long long base,
                                   unsigned k, const float* h_table, unsigned m, unsigned seed, float* h_origins,
                                   float* h_dirs, unsigned char* h_shot) {
  int rc = ao_refuse(c, n, k, m);
  if (!rc && n && (!h_samples || !h_table || !h_origins || !h_dirs)) rc = rt_set_error(RT_EINVAL, "null samples, table or ray output");
  if (rc || n == 0) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nr = n * (size_t)k;
  DevBuf<rt_gsample> d_s;
  DevBuf<float> d_t, d_o, d_d;
  DevBuf<unsigned char> d_m;
  if (d_s.alloc(n) != hipSuccess || d_t.alloc(3 * (size_t)m) != hipSuccess || d_o.alloc(3 * nr) != hipSuccess ||
      d_d.alloc(3 * nr) != hipSuccess || d_m.alloc(n) != hipSuccess)
    return rt_set_error(RT_EHIP, "hipMalloc ambient occlusion rays");
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_s, h_samples, n * sizeof(rt_gsample), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_t, h_table, 3 * (size_t)m * sizeof(float), hipMemcpyHostToDevice, s));
  rc = rt_hip_ao_rays(c, d_s.get(), n, base, k, d_t.get(), m, seed, d_o.get(), d_d.get(), d_m.get(), nullptr);
  if (!rc && (hipMemcpyAsync(h_origins, d_o, 3 * nr * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
              hipMemcpyAsync(h_dirs, d_d, 3 * nr * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
              (h_shot && hipMemcpyAsync(h_shot, d_m, n, hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = rt_set_error(RT_EHIP, "D2H ambient occlusion rays");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = rt_set_error(RT_EHIP, "ambient occlusion rays");  // the buffers above go
  return rc;
}

extern "C" int rt_hip_ambient_occlusion_host(rt_hip_ctx* c, const rt_gsample* h_samples, size_t n,
                                             unsigned long long base, unsigned k, const float* h_table, unsigned m,
                                             unsigned seed, float tmax, unsigned flags, unsigned* h_occluded,
                                             rt_stats* st) {
  int rc = ao_refuse(c, n, k, m);
  if (!rc && n && (!h_samples || !h_table || !h_occluded)) rc = rt_set_error(RT_EINVAL, "null samples, table or output");
  if (!rc) rc = batch_refuse_mode(c, flags, "", "ambient occlusion");
  if (rc) return rc;
  if (n == 0) return batch_host_none(st);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<rt_gsample> d_s;
  DevBuf<float> d_t;
  DevBuf<unsigned> d_out;
  if (d_s.alloc(n) != hipSuccess || d_t.alloc(3 * (size_t)m) != hipSuccess || d_out.alloc(n) != hipSuccess)
    return rt_set_error(RT_EHIP, "hipMalloc ambient occlusion");
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_s, h_samples, n * sizeof(rt_gsample), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_t, h_table, 3 * (size_t)m * sizeof(float), hipMemcpyHostToDevice, s));
  rc = rt_hip_ambient_occlusion(c, d_s.get(), n, base, k, d_t.get(), m, seed, tmax, flags, d_out.get(), nullptr);
  if (!rc && hipMemcpyAsync(h_occluded, d_out, n * sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = rt_set_error(RT_EHIP, "D2H occlusion counts");
  return batch_host_end(c, rc, st);
}
