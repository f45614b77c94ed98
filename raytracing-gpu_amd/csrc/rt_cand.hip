// rt_cand.hip -- per-frame camera-ray candidate lists: the part of the
// closest-hit decision of camera rays that the octree's culling slack cannot
// guarantee (DESIGN.md §2 "Exact camera rays").
//
// cpu/rt tests every triangle for every ray in float (cpu/hit.c:15-33,
// 72-91).  For a ray nearly parallel to a triangle's plane that float
// test accepts crossings far outside the triangle, so a walk that culls
// by the exact geometry can lose the reference's winner.  The forward error
// bound of the float test (tools/mt_bound.py, checked there against the float
// test itself) says: a float accept implies the exact line crosses the
// triangle's plane inside the expanded triangle
//     T_D = { v0 + U e1 + V e2 : U >= -du, V >= -dv, U + V <= 1 + dw }
// with du, dv, dw ~ eps |o - v0| |e| / |a|, |a| = |d| |e1 x e2| |cos|.
// Camera rays all pass (within dline) through the eye, so for a triangle the
// grazing cosine of every camera ray near it is bounded below by
// (distance of the eye from the plane) / (distance to the eye); that bound
// gives T_D per triangle.  If T_D lies within the walk's slack of the
// triangle the walk finds it (the triangle is "safe"); otherwise T_D is
// projected through the eye onto the image plane (it is planar, so its
// footprint is the triangle of its projected corners), widened by the float
// deviation of camera lines, and rasterised into the 8x8 tiles of this rank.
// Triangles with an unbounded footprint (T_D reaching the eye plane) go to a
// global list every camera ray tests.  Count pass -> rocPRIM exclusive scan
// -> fill pass; the render kernel tests each tile's list after its walk with
// the reference's exact arithmetic (consider()).
//
// One translation unit, split by role; this file keeps the launchers:
//   rt_cand_geom.h     the proof geometry (classify, quick_class, the raster
//                      family, tile_keep): host and device, no kernel
//   rt_cand_passes.h   the per-prim list passes (quick, count, big_count,
//                      item, emit, big, big_item, refine)
//   rt_cand_entries.h  the emitted entries: tile bounds, entry skip, the
//                      multi-GPU route / partition / unpack / gather, the
//                      compaction, the heavy-first work order
//   rt_scan.h          the exclusive scans between the passes
// The headers come in the order their kernels have in the device code
// (tools/asm_same.py compares that order).  The host mirrors of the geometry
// (survey, refinement sample, verification) and the frame constants
// (cand_params) are plain C++: rt_cand_host.cpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>  // rocPRIM's iterators use memset

#include <rocprim/rocprim.hpp>

#include "rt_cand.h"
#include "rt_tiles.h"

#include "rt_cand_geom.h"
#include "rt_cand_passes.h"
#include "rt_cand_entries.h"
#include "rt_scan.h"

extern "C" hipError_t rt_cand_prim_leaf(const float4* node, uint32_t nnode, const float4* tri,
                                        uint32_t* prim_leaf, hipStream_t s) {
  if (nnode == 0) return hipSuccess;
  hipLaunchKernelGGL(rtc::prim_leaf_kernel, dim3((nnode + 255) / 256), dim3(256), 0, s, node, nnode,
                     tri, prim_leaf);
  return hipGetLastError();
}

extern "C" size_t rt_cand_footprint_bytes(void) { return sizeof(rtc::Footprint); }

extern "C" hipError_t rt_cand_quick(const CandParams* p, hipStream_t s) {
  const uint32_t len = p->prim1 - p->prim0;
  if (len == 0) {  // no quick_kernel to zero the counters and the scan's last input
    hipError_t e = hipMemsetAsync(p->ctr, 0, RT_CC_BUILD_WORDS * sizeof(uint32_t), s);
    return e != hipSuccess ? e : hipMemsetAsync(p->visits, 0, sizeof(uint32_t), s);
  }
  hipLaunchKernelGGL(rtc::quick_kernel, dim3((len + RT_LIST_BLOCK - 1) / RT_LIST_BLOCK), dim3(RT_LIST_BLOCK), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_count(const CandParams* p, hipStream_t s) {
  const uint32_t len = p->prim1 - p->prim0;  // the list holds prims of the slice only
  if (len == 0) return hipSuccess;
  // sized for the worst case; threads beyond the list's length exit at once
  hipLaunchKernelGGL(rtc::count_kernel, dim3((len + RT_LIST_BLOCK - 1) / RT_LIST_BLOCK), dim3(RT_LIST_BLOCK), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_big_count(const CandParams* p, hipStream_t s) {
  if (p->nprim == 0) return hipSuccess;
  hipLaunchKernelGGL(rtc::big_count_kernel, dim3(rtc::kBigWaves), dim3(64), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_emit(const CandParams* p, hipStream_t s) {
  const uint32_t len = p->prim1 - p->prim0;
  if (len == 0) return hipSuccess;
  hipLaunchKernelGGL(rtc::emit_kernel, dim3((len + RT_LIST_BLOCK - 1) / RT_LIST_BLOCK), dim3(RT_LIST_BLOCK), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_big(const CandParams* p, uint32_t nbig, hipStream_t s) {
  if (nbig == 0) return hipSuccess;
  const uint32_t g = nbig < (uint32_t)rtc::kBigWaves ? nbig : (uint32_t)rtc::kBigWaves;
  hipLaunchKernelGGL(rtc::big_kernel, dim3(g), dim3(64), 0, s, *p);
  return hipGetLastError();
}

extern "C" uint32_t rt_cand_big_waves(void) { return (uint32_t)rtc::kBigWaves; }

extern "C" hipError_t rt_cand_items(const CandParams* p, hipStream_t s) {
  hipLaunchKernelGGL(rtc::item_kernel, dim3(rtc::kBigWaves), dim3(64), 0, s, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_big_items(const CandParams* p, uint32_t nitems, int check, hipStream_t s) {
  // nitems: the items read back (check = 0), or the same frame's read-back
  // build's (check = 1: an asynchronous build; the kernels compare on the device)
  if (nitems == 0) return hipSuccess;
  if (check) {
    hipLaunchKernelGGL(rtc::big_item_kernel<true>, dim3(nitems), dim3(64), 0, s, *p);
    if (p->refine) hipLaunchKernelGGL(rtc::refine_kernel<true>, dim3(nitems), dim3(64), 0, s, *p);
  } else {
    hipLaunchKernelGGL(rtc::big_item_kernel<false>, dim3(nitems), dim3(64), 0, s, *p);
    if (p->refine) hipLaunchKernelGGL(rtc::refine_kernel<false>, dim3(nitems), dim3(64), 0, s, *p);
  }
  return hipGetLastError();
}

// entries [ctr[RT_CC_TOTAL], n) of keys (the buffers' unused tail in an asynchronous
// build, sized from the previous frame) get `key`: they sort after every tile
__global__ __launch_bounds__(256) void fill_tail_kernel(uint32_t* keys, const uint32_t* total, uint32_t n,
                                                        uint32_t key) {
  for (uint32_t i = *total + blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) keys[i] = key;
}

extern "C" hipError_t rt_cand_fill_tail(uint32_t* keys, const uint32_t* total_dev, uint32_t n, uint32_t key,
                                        hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(fill_tail_kernel, dim3(1024), dim3(256), 0, s, keys, total_dev, n, key);
  return hipGetLastError();
}

extern "C" uint32_t rt_cand_scan_dev_tiles(uint32_t nmax) {
  return (nmax + 1u + (uint32_t)rtc::kScanTile - 1u) / (uint32_t)rtc::kScanTile;
}

extern "C" hipError_t rt_cand_scan_dev(const uint32_t* in, uint32_t* out, uint32_t nmax, const uint32_t* n_dev,
                                       uint32_t* total, uint32_t* bsum, hipStream_t s) {
  const uint32_t nb = rt_cand_scan_dev_tiles(nmax);
  hipLaunchKernelGGL(rtc::scan_sums_kernel, dim3(nb), dim3(rtc::kScanThreads), 0, s, in, nmax, n_dev, bsum);
  CandParams none;
  memset(&none, 0, sizeof none);
  hipLaunchKernelGGL(rtc::scan_apply_kernel<false>, dim3(nb), dim3(rtc::kScanThreads), 0, s, in, out, nmax, n_dev,
                     (const uint32_t*)bsum, total, none);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_scan_scatter(const CandParams* p, uint32_t* bsum, hipStream_t s) {
  const uint32_t len = p->prim1 - p->prim0;
  const uint32_t nb = rt_cand_scan_dev_tiles(len);
  hipLaunchKernelGGL(rtc::scan_sums_kernel, dim3(nb), dim3(rtc::kScanThreads), 0, s, p->visits, len,
                     (const uint32_t*)nullptr, bsum);
  hipLaunchKernelGGL(rtc::scan_apply_kernel<true>, dim3(nb), dim3(rtc::kScanThreads), 0, s,
                     (const uint32_t*)p->visits, (uint32_t*)nullptr, len, (const uint32_t*)nullptr,
                     (const uint32_t*)bsum, (uint32_t*)nullptr, *p);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_scan(const uint32_t* in, uint32_t* out, uint32_t n, void* temp,
                                   size_t* temp_bytes, hipStream_t s) {
  if ((size_t)n + 1 <= rtc::kSmallScanMax) {  // one workgroup, no temporary storage
    if (!temp) {
      *temp_bytes = 0;
      return hipSuccess;
    }
    hipLaunchKernelGGL(rtc::scan_small_kernel, dim3(1), dim3(rtc::kSmallScanThreads), 0, s, in, out, n);
    return hipGetLastError();
  }
  return rocprim::exclusive_scan(temp, *temp_bytes, in, out, 0u, (size_t)n + 1,
                                 rocprim::plus<uint32_t>(), s);
}

extern "C" hipError_t rt_cand_sort(uint32_t* keys_in, uint32_t* keys_out, uint32_t* vals_in,
                                   uint32_t* vals_out, uint32_t n, int begin_bit, int end_bit, void* temp,
                                   size_t* temp_bytes, hipStream_t s) {
  // digits of kSortBits bits per onesweep place (rocPRIM's gfx950 u32/u32
  // tuning otherwise: 8 bits, so C5's 17-bit tile keys take three places)
  // onesweep from RT_SORT_MERGE_LIMIT items up (rocPRIM's default switches
  // at 2^20: a consume of ~1 M entries at N = 8 went through 9 merge passes,
  // 0.14 ms)
  using cfg = rocprim::radix_sort_config<
      rocprim::default_config, rocprim::default_config,
      rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, 16>, rocprim::kernel_config<1024, 16>,
                                          rtc::kSortBits, rocprim::block_radix_rank_algorithm::match>,
      RT_SORT_MERGE_LIMIT>;
  return rocprim::radix_sort_pairs<cfg>(temp, *temp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n,
                                        begin_bit, end_bit, s);
}

extern "C" hipError_t rt_cand_entry_skip(const uint32_t* cand, const float* skip, float* out,
                                         uint32_t n, const uint32_t* n_dev, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(rtc::entry_skip_kernel, dim3((n + 255) / 256), dim3(256), 0, s, cand, skip,
                     out, n, n_dev);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_bounds(const uint32_t* keys, uint32_t n, uint32_t* start,
                                     uint32_t ntiles, uint32_t* snap, hipStream_t s) {
  hipLaunchKernelGGL(rtc::bounds_kernel, dim3((ntiles + 1 + 255) / 256), dim3(256), 0, s, keys, n,
                     start, ntiles, snap);
  return hipGetLastError();
}


extern "C" hipError_t rt_cand_route_globals(const uint32_t* global, uint32_t nglobal, int nranks, uint32_t tpr,
                                            uint32_t tbits, uint32_t* keys, uint32_t* vals, hipStream_t s) {
  const uint32_t n = nglobal * (uint32_t)nranks;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(rtc::route_globals_kernel, dim3((n + 255) / 256), dim3(256), 0, s, global, nglobal, nranks,
                     tpr, tbits, keys, vals);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_compact(const uint32_t* keys, const uint32_t* vals, uint32_t n, const uint32_t* n_dev,
                                      uint32_t drop_key, uint32_t cap, uint32_t* cnt, uint32_t* off, void* tmp,
                                      size_t* tmp_bytes, uint32_t* keys_out, uint32_t* vals_out, uint32_t* over_flag,
                                      hipStream_t s) {
  const uint32_t nw = rt_cand_part_waves(n);
  if (!tmp) return rt_cand_scan(cnt, off, nw, nullptr, tmp_bytes, s);
  if (nw == 0) return hipErrorInvalidValue;  // (the host compacts only a build with entries)
  hipLaunchKernelGGL(rtc::compact_count_kernel, dim3(nw), dim3(64), 0, s, keys, n, drop_key, cnt, n_dev);
  hipError_t e = rt_cand_scan(cnt, off, nw, tmp, tmp_bytes, s);  // off[nw] = the kept entries
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rtc::compact_scatter_kernel, dim3(nw), dim3(64), 0, s, keys, vals, n, drop_key, off, cap,
                     keys_out, vals_out, over_flag, n_dev);
  return hipGetLastError();
}

extern "C" uint32_t rt_cand_part_waves(uint32_t n) {
  return (n + rtc::kPartChunk - 1) / rtc::kPartChunk;
}

extern "C" hipError_t rt_cand_part_count(uint32_t* keys, uint32_t n, uint32_t tbits, int nranks, uint32_t* hist,
                                         uint32_t nroute, int tiles_x, int blocks_x, int tb, uint32_t drop_key,
                                         const uint32_t* total_dev, hipStream_t s) {
  const uint32_t nw = rt_cand_part_waves(n);
  if (nw == 0) return hipSuccess;
  hipLaunchKernelGGL(rtc::part_count_kernel, dim3(nw), dim3(64), 0, s, keys, n, tbits, nranks, hist, nroute,
                     tiles_x, blocks_x, tb, drop_key, total_dev);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_part_scatter(const uint32_t* keys, const uint32_t* prims, const float* skip,
                                           uint32_t n, uint32_t tbits, int nranks, const uint32_t* off,
                                           uint32_t* start, uint32_t* out, const uint32_t* ctr, hipStream_t s) {
  const uint32_t nw = rt_cand_part_waves(n);
  hipLaunchKernelGGL(rtc::part_scatter_kernel, dim3(nw ? nw : 1u), dim3(64), 0, s, keys, prims, skip, n, tbits,
                     nranks, off, start, out, ctr);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_unpack(const uint32_t* in, uint32_t n, uint32_t ntiles, uint32_t tpr, uint32_t* keys,
                                     uint32_t* idx, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(rtc::unpack_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, n, ntiles, tpr, keys, idx);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_gather(const uint32_t* in, const uint32_t* idx, uint32_t n, uint32_t* cand,
                                     float* skip, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(rtc::gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, idx, n, cand, skip);
  return hipGetLastError();
}

extern "C" hipError_t rt_cand_order(const uint32_t* start, uint32_t ntiles, uint32_t* flags, uint32_t* pos,
                                    uint32_t* perm, const uint32_t* item_cost,
                                    const unsigned long long* cost_sum, uint32_t waves, void* tmp,
                                    size_t* tmp_bytes, hipStream_t s) {
  if (!tmp) return rt_cand_scan(flags, pos, ntiles, nullptr, tmp_bytes, s);
  const dim3 b(256), g((ntiles + 1 + 255) / 256);
  hipLaunchKernelGGL(rtc::heavy_flag_kernel, g, b, 0, s, start, ntiles, flags, item_cost, cost_sum, waves);
  hipError_t e = rt_cand_scan(flags, pos, ntiles, tmp, tmp_bytes, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rtc::heavy_perm_kernel, g, b, 0, s, flags, pos, ntiles, perm);
  return hipGetLastError();
}
