// rt_scan.h -- the lists' exclusive scans of uint32 counts: the two-launch
// scan whose length is read on the device (scan_sums_kernel +
// scan_apply_kernel; its SCATTER instantiation writes the fast path's compact
// list instead of offsets) and the one-workgroup scan of the short arrays
// between passes (scan_small_kernel).  Longer host-length scans go to rocPRIM
// (rt_cand.hip rt_cand_scan).
// Part of rt_cand.hip's one translation unit.  Needs CandParams (rt_cand.h)
// and, for SCATTER only, slice_prim (rt_cand_passes.h), both included here.
// Known wart: scan_apply_kernel<false> takes a CandParams by value (the
// launcher passes a zeroed one) only because the SCATTER instantiation needs
// it.  Splitting the two would change a kernel's argument layout, hence its
// device code; the split of rt_cand.hip into headers left it alone so that the
// device code stayed comparable.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cand_passes.h"

namespace rtc {

// Exclusive scan of in[0 .. n] (n + 1 values: out[n] = the sum of in[0 ..
// n - 1], also written to *total) with n read on the device (min(*n_dev,
// nmax); n_dev NULL: nmax) -- the classification's scan runs over the listed
// prims only, whose count the host does not know before its one
// synchronisation.  Three passes over tiles of kScanTile values: tile sums,
// one workgroup scanning them, tile-local scans through LDS (coalesced loads
// and stores).  Deterministic (integer adds).
constexpr int kScanThreads = 256, kScanPer = 16, kScanTile = kScanThreads * kScanPer;

__device__ __forceinline__ uint32_t scan_len(uint32_t nmax, const uint32_t* n_dev) {
  const uint32_t n = n_dev ? *n_dev : nmax;
  return (n < nmax ? n : nmax) + 1u;
}

// exclusive scan of one value per thread over a 256-thread block; *sum = total
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* sh, uint32_t* sum) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t inc = x;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  uint32_t before = 0, tot = 0;
  for (int k = 0; k < kScanThreads / 64; k++) {
    if (k < wv) before += sh[k];
    tot += sh[k];
  }
  __syncthreads();
  *sum = tot;
  return before + inc - x;
}

__global__ __launch_bounds__(kScanThreads) void scan_sums_kernel(const uint32_t* __restrict__ in, uint32_t nmax,
                                                                 const uint32_t* n_dev, uint32_t* bsum) {
  __shared__ uint32_t sh[kScanThreads / 64];
  const uint32_t n1 = scan_len(nmax, n_dev), base = blockIdx.x * (uint32_t)kScanTile;
  uint32_t x = 0;
  if (base < n1)
    for (int k = 0; k < kScanPer; k++) {
      const uint32_t i = base + (uint32_t)(k * kScanThreads) + threadIdx.x;
      if (i < n1) x += in[i];
    }
  uint32_t tot;
  block_excl_scan(x, sh, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// The tiles' prefix: each apply workgroup sums the tile sums before its own
// (a few thousand tiles at most: ~10 loads per thread from L2) instead of a
// one-workgroup pass over them between the two launches.
// SCATTER (the fast path's flags over the build's slice, CandParams p): the
// exclusive prefix of a flagged prim is its place in the compact list, which
// this pass writes directly (list[o] = prim), and the scan's last value is
// the list length (ctr[RT_CC_LIST]) -- no offsets array, no scatter launch.
template <bool SCATTER>
__global__ __launch_bounds__(kScanThreads) void scan_apply_kernel(const uint32_t* __restrict__ in, uint32_t* out,
                                                                  uint32_t nmax, const uint32_t* n_dev,
                                                                  const uint32_t* bsum, uint32_t* total,
                                                                  CandParams p) {
  __shared__ uint32_t v[kScanTile + kScanThreads];  // thread t's 16 values at t * 17 (no bank conflicts)
  __shared__ uint32_t sh[kScanThreads / 64];
  const uint32_t n1 = scan_len(nmax, n_dev), base = blockIdx.x * (uint32_t)kScanTile;
  if (base >= n1) return;  // uniform per block
  const int t = threadIdx.x;
  uint32_t before = 0;
  for (uint32_t b = (uint32_t)t; b < blockIdx.x; b += kScanThreads) before += bsum[b];
  uint32_t tot0;
  block_excl_scan(before, sh, &tot0);  // tot0 = the tiles before this one
  for (int k = 0; k < kScanPer; k++) {
    const uint32_t e = (uint32_t)(k * kScanThreads + t), i = base + e;
    v[e + e / kScanPer] = i < n1 ? in[i] : 0u;
  }
  __syncthreads();
  uint32_t run = 0;
  for (int k = 0; k < kScanPer; k++) run += v[t * (kScanPer + 1) + k];
  uint32_t tot;
  uint32_t pre = tot0 + block_excl_scan(run, sh, &tot);
  uint32_t flags = 0;  // SCATTER: which of this thread's values were set
  for (int k = 0; k < kScanPer; k++) {
    const uint32_t x = v[t * (kScanPer + 1) + k];
    if (SCATTER && x) flags |= 1u << k;
    v[t * (kScanPer + 1) + k] = pre;
    pre += x;
  }
  if (SCATTER) {
    // thread t's values are elements t * 16 + k of the tile: write the list
    // entries of its flagged ones (in[] holds 0 / 1)
    for (int k = 0; k < kScanPer; k++) {
      const uint32_t e = (uint32_t)(t * kScanPer + k), i = base + e;
      if (i >= n1) break;
      const uint32_t o = v[t * (kScanPer + 1) + k];
      if (i == n1 - 1u) {
        p.ctr[RT_CC_LIST] = o;  // list length (the scan's last input is 0)
      } else if ((flags >> k) & 1u) {
        p.list[o] = slice_prim(p, i);
      }
    }
    return;
  }
  __syncthreads();
  for (int k = 0; k < kScanPer; k++) {
    const uint32_t e = (uint32_t)(k * kScanThreads + t), i = base + e;
    if (i < n1) {
      const uint32_t o = v[e + e / kScanPer];
      out[i] = o;
      if (i == n1 - 1u && total) *total = o;
    }
  }
}

// Exclusive scan of in[0 .. n] (n + 1 values, out[n] = their sum) in one
// workgroup, for the short scans between list passes (the big footprints'
// items, a partition's per-wave counts, a rank's work order): one launch
// instead of rocPRIM's two.  Wave w owns a contiguous segment of the values,
// loaded and stored lane-consecutive (coalesced) in steps of 64, its lanes'
// values held in registers; a wave scan per step with a running carry, the
// 16 waves' totals combined through LDS.
constexpr uint32_t kSmallScanThreads = 1024, kSmallScanPer = 32;
constexpr uint32_t kSmallScanWaves = kSmallScanThreads / 64;
constexpr uint32_t kSmallScanMax = kSmallScanThreads * kSmallScanPer;

__global__ __launch_bounds__(kSmallScanThreads) void scan_small_kernel(const uint32_t* __restrict__ in,
                                                                       uint32_t* __restrict__ out, uint32_t n) {
  __shared__ uint32_t wsum[kSmallScanWaves];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t m = n + 1u;
  const uint32_t seg = ((m + kSmallScanWaves - 1u) / kSmallScanWaves + 63u) & ~63u;  // per wave, whole steps
  const uint32_t base = wv * seg, steps = seg / 64u;
  uint32_t v[kSmallScanPer], tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < kSmallScanPer; k++) {
    const uint32_t i = base + k * 64u + lane;
    v[k] = (k < steps && i < m) ? in[i] : 0u;
    tot += v[k];
  }
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
  if (lane == 0) wsum[wv] = tot;
  __syncthreads();
  uint32_t carry = 0;
  for (uint32_t k = 0; k < wv; k++) carry += wsum[k];
#pragma unroll
  for (uint32_t k = 0; k < kSmallScanPer; k++) {
    if (k < steps) {  // (uniform)
      uint32_t inc = v[k];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(inc, o, 64);
        if ((int)lane >= o) inc += y;
      }
      const uint32_t i = base + k * 64u + lane;
      if (i < m) out[i] = carry + inc - v[k];
      carry += __shfl(inc, 63, 64);
    }
  }
}

}  // namespace rtc
