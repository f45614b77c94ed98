// rt_dlight.cpp -- host side of direct light for caller's surface records
// (include/rt_hip.h rt_hip_direct_light, rt_hip_direct_light_host): the
// refusals, the light buffers the kernel scans (built as a render builds them,
// csrc/rt_hip.cpp lbuf_prepare) and the launch of csrc/rt_dlight.h.  To the
// context a call is an occlusion batch (csrc/rt_occl.cpp): it counts into the
// batches' stats block, sets last_occl, uses the stack spill area and the item
// counters in stream order, and leaves the kept frame, the lists, the overlap
// state and the render's counters as they are.  Which records shade:
// csrc/rt_dlight_items.h.
#include "rt_ctx.h"
#include "rt_dlight_items.h"

// The refusals: nothing of the context has changed when one of them returns.
static int dlight_refuse(const rt_hip_ctx* c, const void* samples, size_t n, unsigned flags, const float* rgb) {
  if (!c) return rt_set_error(RT_EINVAL, "null context");
  RT_CTX_LIVE(c);
  if (n > RT_RAYS_MAX)
    return rt_set_error(RT_EINVAL, "%zu records: a batch holds at most %llu", n, (unsigned long long)RT_RAYS_MAX);
  if (n && (!samples || !rgb)) return rt_set_error(RT_EINVAL, "null samples or colour output");
  if (flags & ~RT_RAYS_PACKET) return rt_set_error(RT_EINVAL, "unknown direct light flags %#x", flags);
  if (c->policy != RT_POLICY_DEFAULT)
    return rt_set_error(RT_EINVAL, "direct light needs the default traversal policy (have %d)", c->policy);
  if (c->count_work) return rt_set_error(RT_EINVAL, "direct light cannot run as the work-counting pass");
  return RT_OK;
}

extern "C" int rt_hip_direct_light(rt_hip_ctx* c, const void* d_samples, size_t n, unsigned flags, float* d_rgb,
                                   unsigned* d_lit, void* stream) {
  int rc = dlight_refuse(c, d_samples, n, flags, d_rgb);
  if (!rc && ((uintptr_t)d_samples & 7u)) rc = rt_set_error(RT_EINVAL, "samples must be 8-byte aligned");
  if (rc || n == 0) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // an empty octree scene has nothing to traverse: the FLAT kernel with 0 records
  const bool empty = c->accel == RT_ACCEL_OCTREE && !c->d_node;
  const int dacc = (c->accel == RT_ACCEL_FLAT || empty) ? RT_ACCEL_FLAT_D : RT_ACCEL_OCTREE_D;
  const bool octree = dacc == RT_ACCEL_OCTREE_D;
  KParams p = scene_params(c);
  DlArgs a;
  std::memset(&a, 0, sizeof a);
  a.samples = (const uint2*)d_samples;
  a.n = n;
  a.nitems = rt_ray_item_count(n);
  a.nobj = (uint32_t)(c->mat_host.size() / RT_MAT_FLOATS);
  a.rgb = d_rgb;
  a.lit = d_lit;
  if (octree) {
    // the light buffers, as a render has them (a no-op unless the slack or the
    // exact-shadow mode changed; none with rt_hip_set_light_buffers off): a
    // light without one, and a point off a buffer's proof box, walk
    if ((rc = lbuf_prepare(c, s))) return rc;
    // (one descriptor per light, or none: the kernel indexes them by light)
    p.lbuf = c->lb_host.size() == c->nlight ? c->d_lbuf.get() : nullptr;
    if (c->exact_refl) {  // the proven closest walk and its bounds
      if ((rc = reflect_prepare(c, s))) return rc;
      p.node_rf = c->d_node_rf;
      a.walk = RT_RAYS_WALK_EXACT;
    } else if (flags & RT_RAYS_PACKET) {
      a.walk = RT_RAYS_WALK_PACKET;
    }
  }
  // the batches' stats block and this kernel's own grid
  if (!c->d_occl_stats) HIP_TRY(c->d_occl_stats.alloc(RT_STAT_SETS * RT_STAT_STRIDE));
  if (!c->dlight_grid) {
    int g = 0;
    HIP_TRY(rt_dlight_grid(dacc, c->cus, &g));
    c->dlight_grid = g;
  }
  int grid = c->dlight_grid;
  // the spill area holds [entry][lane] for so many one-wave workgroups
  if (octree) grid = (int)std::min<size_t>((size_t)grid, c->d_spill.cap() / ((size_t)64 * RT_SPILL_STACK));
  if ((long long)a.nitems < grid) grid = (int)a.nitems;
  p.tile_counter = c->d_counter;
  p.stats = c->d_occl_stats;
  // every device pointer the kernel follows must exist (a null one would
  // fault the card, not fail the call)
  if (!p.tile_counter || !p.stats || grid <= 0 || (p.nrec && !p.tri) || (p.nlight && !p.lshade) ||
      (a.nobj && !p.mshade))
    return rt_set_error(RT_EHIP, "direct light: device buffers missing");
  if (octree && (!p.node || !p.spill || !p.tri || !p.tri_prim || ((a.walk & RT_RAYS_WALK_EXACT) && !p.node_rf)))
    return rt_set_error(RT_EHIP, "direct light: octree buffers missing");
  HIP_TRY(hipMemsetAsync(c->d_counter, 0, kItemCounterBytes, s));
  HIP_TRY(hipMemsetAsync(c->d_occl_stats, 0, kStatBytes, s));
  HIP_TRY(rt_launch_dlight(&p, &a, dacc, grid, s));
  c->last_occl = 1;  // what rt_hip_stats reads next
  c->occl_stream = s;
  return RT_OK;
}

extern "C" int rt_hip_direct_light_host(rt_hip_ctx* c, const rt_gsample* h_samples, size_t n, unsigned flags,
                                        float* h_rgb, unsigned* h_lit, rt_stats* st) {
  int rc = dlight_refuse(c, h_samples, n, flags, h_rgb);
  if (rc) return rc;
  if (n == 0) {  // nothing launched, nothing written
    if (st) std::memset(st, 0, sizeof *st);
    return RT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  DevBuf<rt_gsample> d_s;
  DevBuf<float> d_rgb;
  DevBuf<unsigned> d_lit;
  if (d_s.alloc(n) != hipSuccess || d_rgb.alloc(3 * n) != hipSuccess || (h_lit && d_lit.alloc(n) != hipSuccess))
    return rt_set_error(RT_EHIP, "hipMalloc direct light");
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_s, h_samples, n * sizeof(rt_gsample), hipMemcpyHostToDevice, s));
  rt_stats tmp;
  rc = rt_hip_direct_light(c, d_s.get(), n, flags, d_rgb.get(), h_lit ? d_lit.get() : nullptr, nullptr);
  if (!rc && (hipMemcpyAsync(h_rgb, d_rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
              (h_lit && hipMemcpyAsync(h_lit, d_lit, n * sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess)))
    rc = rt_set_error(RT_EHIP, "D2H direct light");
  if (!rc) rc = rt_hip_stats(c, st ? st : &tmp);  // (synchronises)
  (void)hipStreamSynchronize(s);                  // the buffers above go
  return rc;
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
