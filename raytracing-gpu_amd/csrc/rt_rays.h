// rt_rays.h -- the kernels of a caller's ray batch (include/rt_hip.h
// rt_hip_trace_rays, rt_hip_frame_rays): the ray-source trace, the per-ray
// fold, the per-ray sample records and the camera-ray generator.  Each ray is
// the reference's trace(ray, 1.0) (cpu/raytracer.c:19-34): trace_path under the
// ray policies appends its hit records, the frames' shade pass and off-box
// fixup shade them, and the fold sums each ray's chain deepest-first.
// Part of rt_render.hip's one translation unit, included after every other
// kernel: needs trace_path, flush_counts, rec_addr, frame_check_account,
// gsample_store and camera_ray.  The batch's host-testable arithmetic (items,
// streams, ray orders) is csrc/rt_ray_items.h; its launches csrc/rt_rays.cpp.
#pragma once

#include "rt_ray_items.h"

namespace rt {

static_assert(RT_REC_REGIONS == RT_HIT_REGIONS, "rt_ray_items.h states the record index's regions");

// Ray-source trace: a work item is 64 consecutive rays, lane = ray.  The same
// persistent one-wave workgroups as trace_kernel: 8 item streams (stream x =
// the items k = x (mod 8), its hits in region x, its counter
// p.tile_counter[32 x]), workgroup b at home in stream b mod 8, each home
// wave's first item without an atomic, a drained stream's waves moving on.
// Every item writes its lanes' deepest records (p.last[64 item + lane]) and,
// under RT_POLICY_RAYS_GB, their capture records.  A ray past the batch's end
// or one that is not traced (rt_ray_traced) makes no query.
// (The item claim stays inline here and in the other kernels that pull items
// this way: through a shared function their scalar register allocation changed.)
template <int ACCEL, int POL>
__global__ __launch_bounds__(64, RT_TRACE_MIN_WAVES) void rays_trace_kernel(KParams p, RayArgs a) {
  const int lane = threadIdx.x & 63;
  WorkCount wc = {};
  __shared__ float4 s_stack[ACCEL == RT_ACCEL_FLAT_D ? 1 : kStackArea];
  __shared__ float4 s_stage[ACCEL == RT_ACCEL_FLAT_D ? kStageFlat : kStageOct];
  Stack stk;
  WaveCtx w;
  wave_state(p, s_stack, s_stage, lane, stk, w);
  const uint32_t home = (uint32_t)blockIdx.x & 7u;
  uint32_t probe = 0;
  bool first = true;
  for (;;) {
    const uint32_t x = (home + probe) & 7u;
    uint32_t q = 0;
    if (first) {
      q = (uint32_t)blockIdx.x >> 3;
      first = false;
    } else {
      if (lane == 0) q = atomicAdd(p.tile_counter + 32u * x, 1u);
      q = uni(q) + (gridDim.x - x + 7u) / 8u;
    }
    if (q >= rt_ray_stream_items(a.nitems, x)) {
      if (++probe == 8u) break;  // every stream drained: the wave exits
      continue;
    }
    const size_t i = (size_t)rt_ray_stream_item(q, x) * RT_RAY_ITEM + (size_t)lane;
    // a lane without a ray walks nothing, but its ray takes part in the
    // packet walk's wave-wide arithmetic: a harmless one
    f3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
    bool valid = false;
    if (i < a.n) {
      const f3 ro = ld3(a.org + 3 * i), rd = ld3(a.dir + 3 * i);
      const uint32_t ob[3] = {__float_as_uint(ro.x), __float_as_uint(ro.y), __float_as_uint(ro.z)};
      const uint32_t db[3] = {__float_as_uint(rd.x), __float_as_uint(rd.y), __float_as_uint(rd.z)};
      valid = rt_ray_traced(ob, db);
      if (valid) o = ro, d = rd;
    }
    wc.pixels += (uint32_t)__popcll(__ballot(valid));  // the rays traced (rt_stats.camera of a batch)
    Capture cap;
    p.last[i] = trace_path<ACCEL, false, POL>(p, valid, o, d, x, stk, w, wc, 0u, cap, 0, 1.0f, RT_NO_REC, a.walk);
    if (POL == RT_POLICY_RAYS_GB) p.capture[i] = make_uint4(cap.prim, cap.dist, cap.first, cap.queries);
  }
  flush_counts(p, wc, lane);
}

// Per-ray fold, the batch's last launch: rgb[ray] = its path's terms summed
// deepest-first, color_add(reflected, term) from the deepest call outwards
// (cpu/raytracer.c:29-30) -- the loop fold_kernel runs per sample, without the
// 0.25 average of a pixel's four (fold_kernel keeps its own copy inline: through
// a shared function its register count changed) -- and the frame check's
// bookkeeping.  One thread per ray; a ray cast (a.rgb NULL) launches one
// workgroup for the bookkeeping alone.
template <int>
__global__ __launch_bounds__(256) void rays_fold_kernel(KParams p, RayArgs a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && p.frame_check) frame_check_account(p);
  if (!a.rgb || i >= a.n) return;
  col sc = init_color(0.0f, 0.0f, 0.0f);
  uint32_t r = p.last[i];
  while (r != RT_NO_REC && (r >> 3) < p.hit_cap) {
    const size_t at = rec_addr(p, r);
    const float4 tm = p.hit_term[at];
    sc = color_add(sc, col{tm.x, tm.y, tm.z});
    r = p.hit_prev[at];
  }
  float* o = a.rgb + 3 * i;
  o[0] = sc.r;
  o[1] = sc.g;
  o[2] = sc.b;
}

// Per-ray sample records: gbuffer_kernel's conversion of a capture record and
// its path's first hit record (gsample_store), indexed by ray.
template <int>
__global__ __launch_bounds__(256) void rays_sample_kernel(KParams p, RayArgs a) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  gsample_store(p, true, i, a.samples + i * RT_GB_WORDS_D);
}

// rt_hip_frame_rays: ray idx of the 4 W H camera rays of p's frame, by
// camera_ray -- the arithmetic trace_kernel's samples use -- in pixel order or
// in quarter order (rt_ray_items.h).  One thread per ray.
template <int>
__global__ __launch_bounds__(256) void frame_rays_kernel(KParams p, int order, float* __restrict__ org,
                                                         float* __restrict__ dir) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * (size_t)p.W * (size_t)p.H) return;
  int row, col_, smp;
  if (order)
    rt_quarter_order_ray(p.W, i, &row, &col_, &smp);
  else
    rt_pixel_order_ray(p.W, i, &row, &col_, &smp);
  f3 point, d;
  camera_ray(p, row, col_, smp, point, d);
  org[3 * i] = point.x, org[3 * i + 1] = point.y, org[3 * i + 2] = point.z;
  dir[3 * i] = d.x, dir[3 * i + 1] = d.y, dir[3 * i + 2] = d.z;
}

}  // namespace rt
