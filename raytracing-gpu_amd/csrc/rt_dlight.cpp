// rt_dlight.cpp -- host side of direct light for caller's surface records
// (include/rt_hip.h rt_hip_direct_light, rt_hip_direct_light_host): the
// refusals, the argument block and the launch of csrc/rt_dlight.h through the
// batches' one host path (csrc/rt_batch.h), which builds the light buffers the
// kernel scans as a render builds them (csrc/rt_hip.cpp lbuf_prepare) and says
// what a call leaves as it is.  Which records shade: csrc/rt_dlight_items.h.
#include "rt_batch.h"
#include "rt_dlight_items.h"

// The refusals: nothing of the context has changed when one of them returns.
static int dlight_refuse(const rt_hip_ctx* c, const void* samples, size_t n, unsigned flags, const float* rgb) {
  int rc = batch_refuse_ctx(c);
  if (!rc) rc = batch_refuse_size(n, "records");
  if (rc) return rc;
  if (n && (!samples || !rgb)) return rt_set_error(RT_EINVAL, "null samples or colour output");
  return batch_refuse_mode(c, flags, "", "direct light");
}

extern "C" int rt_hip_direct_light(rt_hip_ctx* c, const void* d_samples, size_t n, unsigned flags, float* d_rgb,
                                   unsigned* d_lit, void* stream) {
  int rc = dlight_refuse(c, d_samples, n, flags, d_rgb);
  if (!rc && ((uintptr_t)d_samples & 7u)) rc = rt_set_error(RT_EINVAL, "samples must be 8-byte aligned");
  if (rc || n == 0) return rc;
  DlArgs a;
  std::memset(&a, 0, sizeof a);
  a.samples = (const uint2*)d_samples;
  a.n = n;
  a.nitems = rt_ray_item_count(n);
  a.nobj = (uint32_t)(c->mat_host.size() / RT_MAT_FLOATS);
  a.rgb = d_rgb;
  a.lit = d_lit;
  // with the light buffers: a light without one, and a point off a buffer's
  // proof box, walk
  BatchLaunch b;
  if ((rc = batch_begin(c, stream, flags, RT_BATCH_DLIGHT, a.nitems, true, "direct light", &b))) return rc;
  a.walk = b.walk;
  if ((b.p.nlight && !b.p.lshade) || (a.nobj && !b.p.mshade))
    return rt_set_error(RT_EHIP, "direct light: device buffers missing");
  if (b.octree && !b.p.tri_prim) return rt_set_error(RT_EHIP, "direct light: octree buffers missing");
  return batch_run(c, b, &a);
}

extern "C" int rt_hip_direct_light_host(rt_hip_ctx* c, const rt_gsample* h_samples, size_t n, unsigned flags,
                                        float* h_rgb, unsigned* h_lit, rt_stats* st) {
  int rc = dlight_refuse(c, h_samples, n, flags, h_rgb);
  if (rc) return rc;
  if (n == 0) return batch_host_none(st);
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<rt_gsample> d_s;
  DevBuf<float> d_rgb;
  DevBuf<unsigned> d_lit;
  if (d_s.alloc(n) != hipSuccess || d_rgb.alloc(3 * n) != hipSuccess || (h_lit && d_lit.alloc(n) != hipSuccess))
    return rt_set_error(RT_EHIP, "hipMalloc direct light");
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_s, h_samples, n * sizeof(rt_gsample), hipMemcpyHostToDevice, s));
  rc = rt_hip_direct_light(c, d_s.get(), n, flags, d_rgb.get(), h_lit ? d_lit.get() : nullptr, nullptr);
  if (!rc && (hipMemcpyAsync(h_rgb, d_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
              (h_lit && hipMemcpyAsync(h_lit, d_lit, n * sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = rt_set_error(RT_EHIP, "D2H direct light");
  return batch_host_end(c, rc, st);
}

// Test hook (include/rt_hip_test.h): the proof box of a light's buffer, as the
// kernel reads it.
extern "C" int rt_hip_lightbuf_box(rt_hip_ctx* c, unsigned light, int* has, float lo[3], float hi[3]) {
  if (!c || !has || !lo || !hi) return rt_set_error(RT_EINVAL, "null argument");
  RT_CTX_LIVE(c);
  if (light >= c->nlight) return rt_set_error(RT_EINVAL, "light %u of %u", light, c->nlight);
  *has = 0;
  if (!c->d_lbuf || light >= c->lb_host.size() || c->lb_host[light].kind == RT_LB_NONE) return RT_OK;
  *has = 1;
  for (int a = 0; a < 3; a++) lo[a] = c->lb_host[light].olo[a], hi[a] = c->lb_host[light].ohi[a];
  return RT_OK;
}
