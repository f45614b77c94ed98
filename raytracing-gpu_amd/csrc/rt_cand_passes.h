// rt_cand_passes.h -- the per-frame list passes over the prims: their sizing
// constants, the fast path (quick_kernel), the classification and count of
// the small footprints (count_kernel), the big footprints' counts and work
// items (big_count_kernel, item_kernel), the emission (emit_kernel,
// big_kernel, big_item_kernel) and the per-tile refinement pass
// (refine_kernel).  What happens to the emitted (tile, prim) entries is
// rt_cand_entries.h; the scans between the passes are rt_scan.h.
// Part of rt_cand.hip's one translation unit.  Needs the geometry
// (rt_cand_geom.h, included here) and the counter words (rt_counters.h,
// through rt_cand.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cand_geom.h"

namespace rtc {

// persistent waves of the big-footprint passes (they loop over the big list,
// whose length only the device knows before the scan)
constexpr int kBigWaves = 4096;
// Entries per big_item_kernel / refine_kernel wave: 1 << CandParams::
// chunk_shift.  One wave per footprint (big_kernel) left the chip idle behind
// a few long ones: C5's largest footprint has 53,789 entries in rows of ~200
// tiles, each lane writing its row alone, and the kernel ran at 0.42 resident
// waves per SIMD (profiles/r03w_c5/pmc_sq.json).  1024 for a whole frame; a
// build of 1/N of the work (a rank's share, a producer's slice) has 1/N of
// the items, too few to cover the latency of one, and takes smaller chunks
// (rt_hip.cpp cand_chunk_shift).
// threads per workgroup of the per-prim list passes (fast path,
// classification, small emission)
#ifndef RT_LIST_BLOCK
#define RT_LIST_BLOCK 256
#endif
// bits per radix place of the lists' sort (rocPRIM's tuned default is 8):
// 9 sorts C5's 17-bit tile keys in two places instead of three (lists 2.13
// -> 1.98 ms; 6 bits: 2.20; profiles/r04o_sort_bits/)
static constexpr unsigned kSortBits = 9;
#ifndef RT_SORT_MERGE_LIMIT
#define RT_SORT_MERGE_LIMIT (1u << 16)
#endif

// Pass 0: the float fast path over every prim; flags the prims it cannot
// prove safe (visits[prim] = 1), which the fused scan and scatter of
// rt_cand_scan_scatter turn into a compact list, so the f64 classification
// of pass 1 runs on full waves instead of on the scattered third of the lanes
// of every wave.
// the i-th prim of the build's slice (CandParams::prim0, sl_stride)
__device__ __forceinline__ uint32_t slice_prim(const CandParams& p, uint32_t i) {
  if (p.sl_stride <= 1u) return p.prim0 + i;
  const uint32_t b = i / RT_SLICE_BLOCK;
  return (b * p.sl_stride + p.sl_rank) * RT_SLICE_BLOCK + i % RT_SLICE_BLOCK;
}

// waves per SIMD the fast path is compiled for (VGPR budget; A/B knob)
#ifndef RT_QUICK_WAVES
#define RT_QUICK_WAVES 1
#endif
__global__ __launch_bounds__(RT_LIST_BLOCK, RT_QUICK_WAVES) void quick_kernel(CandParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;  // index in the slice
  const uint32_t len = p.prim1 - p.prim0;
  if (i < RT_CC_BUILD_WORDS) p.ctr[i] = 0u;          // the frame's counters (count / big passes, later launches)
  if (i == 0u) p.visits[len] = 0u;    // the scan's last input
  if (i >= len) return;
  p.visits[i] = quick_class(p, (const float*)(p.tri + 3 * (size_t)slice_prim(p, i))) == Q_LIST ? 1u : 0u;
}

// small footprint: few tile rows, counted here row by row; false: big
__host__ __device__ inline bool small_count(const CandParams& p, const Footprint& fp, uint32_t& n) {
  int r0, r1;
  n = 0;
  if (!raster_rows(p, fp, r0, r1)) return true;
  if ((r1 >> 3) - (r0 >> 3) + 1 > kSmallRows) return false;
  for (int ty = r0 >> 3; ty <= (r1 >> 3); ty++) n += count_row(p, fp, ty, r0, r1);
  return n <= kSmallEntries;
}

// A small footprint as emit_kernel needs it: its first tile row and row
// count, and per row (at most kSmallRows) row_ivs's three column intervals as
// 16-bit values -- 32 B instead of the 120 B footprint, and no f64 row
// geometry in the emission.  small_count and this form in one pass (row_ivs's
// counts add up to count_row's).  (cand_prepare keeps the footprint path for
// frames of 32,767 tile columns or more.)
__device__ __forceinline__ bool small_pack(const CandParams& p, const Footprint& fp, uint32_t& n, uint32_t* w) {
  int r0, r1;
  n = 0;
  if (!raster_rows(p, fp, r0, r1)) return true;
  const int ty0 = r0 >> 3, nr = (r1 >> 3) - ty0 + 1;
  if (nr > kSmallRows) return false;
  w[0] = (uint32_t)ty0 | ((uint32_t)nr << 16);
  for (int h = 1; h < 8; h++) w[h] = 0u;
  for (int r = 0; r < nr; r++) {
    int x[6], f[3];
    uint32_t c[3];
    row_ivs(p, fp, ty0 + r, r0, r1, x, f, c);
    n += c[0] + c[1] + c[2];
    for (int i = 0; i < 6; i++) {
      const int h = 1 + r * 3 + i / 2;  // words 1..3 row 0, 4..6 row 1
      w[h] |= ((uint32_t)x[i] & 0xffffu) << (16 * (i & 1));
    }
  }
  return n <= kSmallEntries;
}

// (The classification's leaf box loaded at its start instead of at its use
// measured lists 1.803 -> 1.816 ms at 128 VGPRs, profiles/r08_list_occupancy/,
// removed.)
// Pass 1: classify the listed prims, keep each one's footprint and count the
// tiles of the small ones (visits[j] for list entry j; visits is zero beyond
// the list); big ones are queued for big_count_kernel.
__device__ __forceinline__ void count_one(const CandParams& p, uint32_t j) {
  const uint32_t prim = p.list[j];
  const float* rec = (const float*)(p.tri + 3 * (size_t)prim);
  uint32_t visits = 0;
  Footprint fp;
  const float* lb = p.prim_leaf ? (const float*)(p.node + 2 * (size_t)p.prim_leaf[prim]) : nullptr;
  const int c = classify(p, rec, lb, fp);
  if (c == GLOBAL) {
    p.global[atomicAdd(p.ctr + RT_CC_GLOBAL, 1u)] = prim;
    p.skip[prim] = -1e30f;
  } else if (c == FOOTPRINT) {
    p.skip[prim] = fp.skip;
    uint32_t w[8];
    if (p.sfp ? small_pack(p, fp, visits, w) : small_count(p, fp, visits)) {
      if (visits) {
        if (p.store_fp) p.fp[j] = fp;
        if (p.sfp) {
          p.sfp[2 * (size_t)j] = make_uint4(w[0], w[1], w[2], w[3]);
          p.sfp[2 * (size_t)j + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        }
      }
    } else {
      p.fp[j] = fp;
      if (p.sfp) p.sfp[2 * (size_t)j] = make_uint4(0xffffffffu, 0u, 0u, 0u);  // big: not emit_kernel's
      p.big[atomicAdd(p.ctr + RT_CC_BIG, 1u)] = j;
      visits = 0;  // big_count_kernel
    }
  }
  p.visits[j] = visits;
}

#ifndef RT_COUNT_WAVES
#define RT_COUNT_WAVES 1
#endif
__global__ __launch_bounds__(RT_LIST_BLOCK, RT_COUNT_WAVES) void count_kernel(CandParams p) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < p.ctr[RT_CC_LIST]) count_one(p, j);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// exclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t x, int lane) {
  uint32_t inc = x;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  return inc - x;
}

// Pass 1b: one wave per big footprint, its tile rows over the lanes.
__global__ __launch_bounds__(64) void big_count_kernel(CandParams p) {
  const int lane = threadIdx.x;
  const uint32_t nbig = p.ctr[RT_CC_BIG];
  uint32_t witems = 0;
  for (uint32_t b = blockIdx.x; b < nbig; b += gridDim.x) {
    const uint32_t j = p.big[b];
    const Footprint fp = p.fp[j];
    int r0, r1;
    uint32_t cnt = 0;
    if (raster_rows(p, fp, r0, r1))
      for (int ty = (r0 >> 3) + lane; ty <= (r1 >> 3); ty += 64) cnt += count_row(p, fp, ty, r0, r1);
    if (b < p.big_cap) p.big_lane[(size_t)b * 64 + lane] = cnt;  // big_kernel's offsets
    cnt = wave_sum(cnt);
    if (lane == 0) p.visits[j] = cnt;
    witems += (cnt + (1u << p.chunk_shift) - 1) >> p.chunk_shift;
  }
  // this wave's big_item_kernel items (one per chunk of entries of each of its
  // footprints), placed by a scan over the waves: one atomic per footprint
  // on a shared counter serialised at L2 (big_count 0.16 -> 1.5 ms on C5)
  if (lane == 0) p.wave_items[blockIdx.x] = witems;
}

// After the scan of wave_items: each big_count wave's footprints, in the same
// order, write their items from the wave's offset; past item_cap, ctr[RT_CC_ITEMS_OVER] = 1
// and the host emits with big_kernel instead.
__global__ __launch_bounds__(64) void item_kernel(CandParams p) {
  const int lane = threadIdx.x;
  const uint32_t nbig = p.ctr[RT_CC_BIG];
  uint32_t at = p.wave_base[blockIdx.x];
  if (blockIdx.x == 0 && lane == 0) p.ctr[RT_CC_ITEMS] = p.wave_base[kBigWaves];  // all items (read back with ctr[])
  for (uint32_t b = blockIdx.x; b < nbig; b += gridDim.x) {
    const uint32_t ni = (p.visits[p.big[b]] + (1u << p.chunk_shift) - 1) >> p.chunk_shift;
    if (at + ni <= p.item_cap) {
      for (uint32_t c = (uint32_t)lane; c < ni; c += 64) p.items[at + c] = make_uint2(b, c);
    } else if (lane == 0) {
      p.ctr[RT_CC_ITEMS_OVER] = 1u;
    }
    at += ni;
  }
}

// The rank's tiles of one tile-row column interval [x0, x1] of tile row ty:
// the rank's blocks bx = f, f + n, ... of the row (csrc/rt_tiles.h), each
// contributing its columns inside the interval at consecutive local indices
// (the rank's blocks of a row are consecutive in its buffer) -- one prefix
// count per interval, no division per tile.  Returns the count written at
// keys/vals[o ..].
__device__ __forceinline__ uint32_t emit_interval(const CandParams& p, int ty, int x0, int x1,
                                                  uint32_t o, uint32_t prim, bool refine = false) {
  if (x0 > x1) return 0;
  const uint32_t n = (uint32_t)p.nranks, r = (uint32_t)p.rank;
  int f;
  const int tb = p.tb;
  const uint32_t cnt = rt_rank_row_tiles(ty, x0, x1, n, r, (uint32_t)p.blocks_x, (uint32_t)tb, &f);
  if (cnt == 0) return 0;
  const uint32_t row = (uint32_t)(ty % tb) * (uint32_t)tb;
  uint32_t blk = rt_block_local((uint32_t)f, (uint32_t)(ty / tb), n, (uint32_t)p.blocks_x, r);
  uint32_t k = 0;
  for (int bx = f; k < cnt; bx += (int)n, blk++) {
    const int a = x0 > bx * tb ? x0 : bx * tb, b = x1 < bx * tb + tb - 1 ? x1 : bx * tb + tb - 1;
    const uint32_t base = blk * (uint32_t)(tb * tb) + row;
    for (int tx = a; tx <= b; tx++, k++) {
      if (p.key_cap && o + k >= p.key_cap) {  // the buffers hold the previous frame's total
        p.ctr[RT_CC_OVERFLOW] = 1u;
        continue;
      }
      const bool keep = !refine || tile_keep(p, (const float*)(p.tri + 3 * (size_t)prim), tx, ty);
      p.keys[o + k] = keep ? base + (uint32_t)(tx - bx * tb) : p.drop_key;
      p.vals[o + k] = prim;
    }
  }
  return cnt;
}

// One tile row of a footprint (raster_row's tiles: [a0, a1] and the parts
// of [b0, b1] outside it); returns the entries written.
__device__ __forceinline__ uint32_t emit_row(const CandParams& p, const Footprint& fp, int ty, int r0,
                                             int r1, uint32_t o, uint32_t prim, bool refine = false) {
  int a0, a1, b0, b1;
  row_tiles(p, fp, ty, r0, r1, a0, a1, b0, b1);
  uint32_t k = emit_interval(p, ty, a0, a1, o, prim, refine);
  if (a0 > a1) {
    k += emit_interval(p, ty, b0, b1, o + k, prim, refine);
  } else {
    k += emit_interval(p, ty, b0, b1 < a0 - 1 ? b1 : a0 - 1, o + k, prim, refine);
    k += emit_interval(p, ty, b0 > a1 + 1 ? b0 : a1 + 1, b1, o + k, prim, refine);
  }
  return k;
}

// Pass 2 (after the scan of visits): the small footprints write their
// (tile, prim) pairs at their offsets.
__global__ __launch_bounds__(RT_LIST_BLOCK) void emit_kernel(CandParams p) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.ctr[RT_CC_LIST]) return;
  uint32_t o = p.off[j];
  const uint32_t n = p.off[j + 1] - o;
  if (n == 0 || n > kSmallEntries) return;  // big footprints: big_kernel
  const uint32_t prim = p.list[j];
  if (p.sfp) {
    const uint4 a = p.sfp[2 * (size_t)j];
    if (a.x == 0xffffffffu) return;  // a big footprint of few entries
    const uint4 b = p.sfp[2 * (size_t)j + 1];
    const uint32_t w[7] = {a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int ty0 = (int)(a.x & 0xffffu), nr = (int)(a.x >> 16);
    for (int r = 0; r < nr; r++)
      for (int i = 0; i < 3; i++) {
        const uint32_t v = w[r * 3 + i];
        const int x0 = (int)(int16_t)(v & 0xffffu), x1 = (int)(int16_t)(v >> 16);
        o += emit_interval(p, ty0 + r, x0, x1, o, prim);
      }
    return;
  }
  const Footprint fp = p.fp[j];
  int r0, r1;
  if (!raster_rows(p, fp, r0, r1) || (r1 >> 3) - (r0 >> 3) + 1 > kSmallRows) return;
  for (int ty = r0 >> 3; ty <= (r1 >> 3); ty++) o += emit_row(p, fp, ty, r0, r1, o, prim);
}

// Pass 2b: one wave per big footprint, its tile rows over the lanes; a wave
// prefix sum of the lanes' row counts places each lane's entries.
__global__ __launch_bounds__(64) void big_kernel(CandParams p) {
  // launched only when the build expects more than item_cap items (ctr[RT_CC_ITEMS_OVER]):
  // read back, or -- an asynchronous build -- the same frame's earlier
  // read-back build's shape.  A shape that differs on the device (never
  // expected) means big_item_kernel was not launched: the frame is reported
  // (ctr[RT_CC_OVERFLOW] -> RT_EHITBUF, built again with a read-back), never incomplete.
  if (!p.ctr[RT_CC_ITEMS_OVER]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) p.ctr[RT_CC_OVERFLOW] = 1u;
    return;
  }
  const int lane = threadIdx.x;
  const uint32_t nbig = p.ctr[RT_CC_BIG];
  for (uint32_t b = blockIdx.x; b < nbig; b += gridDim.x) {
    const uint32_t j = p.big[b], prim = p.list[j];
    const Footprint fp = p.fp[j];
    int r0 = 0, r1 = -1;
    const bool rows = raster_rows(p, fp, r0, r1);
    const int ty0 = r0 >> 3, ty1 = r1 >> 3;
    uint32_t cnt = 0;
    if (b < p.big_cap)
      cnt = p.big_lane[(size_t)b * 64 + lane];  // big_count_kernel's row subtotals
    else if (rows)
      for (int ty = ty0 + lane; ty <= ty1; ty += 64) cnt += count_row(p, fp, ty, r0, r1);
    uint32_t o = p.off[j] + wave_excl_scan(cnt, lane);
    const bool refine = p.refine != 0u && rows && refined_rows(r0, r1);
    if (rows)
      for (int ty = ty0 + lane; ty <= ty1; ty += 64) o += emit_row(p, fp, ty, r0, r1, o, prim, refine);
  }
}

// Column of the k-th of this rank's tiles in [x0, x1] of tile row ty (f =
// the first of the rank's block columns there, rt_rank_row_tiles): the first
// block may be cut on the left, the ones after it hold tb tiles each, n
// blocks apart.  tb is 1 or RT_TB (a power of two).
__device__ __forceinline__ int kth_rank_col(const CandParams& p, int x0, int x1, int f, uint32_t k) {
  const int tb = p.tb;
  const int s0 = x0 > f * tb ? x0 : f * tb;
  const int e0 = x1 < f * tb + tb - 1 ? x1 : f * tb + tb - 1;
  const uint32_t c0 = (uint32_t)(e0 - s0 + 1);
  if (k < c0) return s0 + (int)k;
  const uint32_t kk = k - c0, sh = (uint32_t)(__ffs(tb) - 1);
  const int m = 1 + (int)(kk >> sh);
  return (f + m * p.nranks) * tb + (int)(kk & (uint32_t)(tb - 1));
}

// Pass 2b, entry-parallel (big_count_kernel's items): the wave writes entries
// [c chunk, (c + 1) chunk) of big footprint b, lane-consecutive (coalesced
// stores).  Row by row in row-major order, each row's intervals in
// raster_row's order; the rows are taken 64 at a time -- the lanes compute
// their intervals and counts (row_ivs), a wave scan places them, and each
// entry of the chunk finds its row by binary search over the 64 prefixes in
// LDS.  Same (tile, prim) set as big_kernel; the sort orders it.
// One workgroup per item.  CHECK (an asynchronous build: its grid is the
// same frame's read-back build's) reads the item count and the over-cap flag
// on the device: an over-cap flag (ctr[RT_CC_ITEMS_OVER]) the launch did not expect, or a
// count the grid does not cover -- never expected -- sets ctr[RT_CC_OVERFLOW], so the
// frame is reported rather than incomplete.  (The checks cost 16-18 VGPRs -- 4 waves
// per SIMD instead of 5 -- so the read-back build's launch, whose grid is
// the exact count, goes without them; a grid-stride loop over the items held
// 118 VGPRs.)
template <bool CHECK>
__global__ __launch_bounds__(64) void big_item_kernel(CandParams p) {
  __shared__ uint32_t pre[65];
  __shared__ int rx[64][6], rf[64][3];
  __shared__ uint32_t rc[64][2];
  __shared__ int rty[64];
  const int lane = threadIdx.x;
  if (CHECK) {
    if (p.ctr[RT_CC_ITEMS_OVER]) {  // more items than item_cap after all: big_kernel was not launched (as big_kernel)
      if (blockIdx.x == 0 && lane == 0) p.ctr[RT_CC_OVERFLOW] = 1u;
      return;
    }
    const uint32_t n_items = p.wave_base[kBigWaves];
    if (blockIdx.x == 0 && lane == 0 && n_items > gridDim.x) p.ctr[RT_CC_OVERFLOW] = 1u;
    if (blockIdx.x >= n_items) return;
  }
  const uint2 it = p.items[blockIdx.x];
  const uint32_t j = p.big[it.x], prim = p.list[j];
  const uint32_t base = p.off[j], total = p.off[j + 1] - base;
  const uint32_t c0 = it.y << p.chunk_shift;
  uint32_t c1 = c0 + (1u << p.chunk_shift) < total ? c0 + (1u << p.chunk_shift) : total;
  if (CHECK && base + c1 > p.key_cap) {  // entries past the buffers: not written, the frame reported
    if (lane == 0) p.ctr[RT_CC_OVERFLOW] = 1u;
    c1 = p.key_cap > base ? p.key_cap - base : 0u;
  }
  const Footprint fp = p.fp[j];
  int r0, r1;
  if (!raster_rows(p, fp, r0, r1)) return;  // no entries, no items
  uint32_t g0 = 0;  // entries of the footprint before this group of rows
  for (int gy = r0 >> 3; gy <= (r1 >> 3) && g0 < c1; gy += 64) {
    const int ty = gy + lane;
    int x[6] = {1, 0, 1, 0, 1, 0}, f[3] = {0, 0, 0};
    uint32_t c[3] = {0u, 0u, 0u};
    if (ty <= (r1 >> 3)) row_ivs(p, fp, ty, r0, r1, x, f, c);
    const uint32_t n = c[0] + c[1] + c[2];
    const uint32_t ex = wave_excl_scan(n, lane);
    const uint32_t gt = __shfl(ex + n, 63, 64);
    if (g0 + gt > c0) {
      __syncthreads();  // after the previous group's readers
      pre[lane] = g0 + ex;
      if (lane == 63) pre[64] = g0 + gt;
#pragma unroll
      for (int i = 0; i < 6; i++) rx[lane][i] = x[i];
#pragma unroll
      for (int i = 0; i < 3; i++) rf[lane][i] = f[i];
      rc[lane][0] = c[0];
      rc[lane][1] = c[1];
      rty[lane] = ty;
      __syncthreads();
      const uint32_t e0 = c0 > g0 ? c0 : g0, e1 = c1 < g0 + gt ? c1 : g0 + gt;
      for (uint32_t e = e0 + (uint32_t)lane; e < e1; e += 64) {
        // the last row whose prefix is <= e (it holds e: e < pre[64], and a
        // row without entries shares its prefix with the next one)
        int r = 0;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1)
          if (pre[r + s] <= e) r += s;
        uint32_t k = e - pre[r];
        int iv = 0;
        if (k >= rc[r][0]) {
          k -= rc[r][0];
          iv = 1;
          if (k >= rc[r][1]) {
            k -= rc[r][1];
            iv = 2;
          }
        }
        const int tx = kth_rank_col(p, rx[r][2 * iv], rx[r][2 * iv + 1], rf[r][iv], k);
        uint32_t rk;
        p.keys[base + e] = rt_tile_local(tx, rty[r], (uint32_t)p.nranks, (uint32_t)p.blocks_x,
                                         (uint32_t)p.tb, &rk);
        p.vals[base + e] = prim;
      }
    }
    g0 += gt;
  }
}

// The per-tile refinement (CandParams::refine) as its own pass over
// big_item_kernel's items: each wave re-reads its chunk's keys and rewrites
// the dropped ones with drop_key.  A pass of its own, with the triangle's and
// the frame's parts in LDS and re-read per entry, runs at 80 VGPRs and 6
// waves per SIMD; inside big_item_kernel the same test held 137-175 VGPRs (2-3
// waves) and the frame took 0.1 ms longer on C5 (profiles/r06e/ab.log).
__device__ __forceinline__ void refine_item(const CandParams& p, uint32_t item);

#ifndef RT_REFINE_WAVES
#define RT_REFINE_WAVES 1
#endif
template <bool CHECK>
__global__ __launch_bounds__(64, RT_REFINE_WAVES) void refine_kernel(CandParams p) {
  if (CHECK && (p.ctr[RT_CC_ITEMS_OVER] || blockIdx.x >= p.wave_base[kBigWaves])) return;
  refine_item(p, blockIdx.x);
}

__device__ __forceinline__ void refine_item(const CandParams& p, uint32_t item) {
  const int lane = threadIdx.x;
  const uint2 it = p.items[item];
  const uint32_t j = p.big[it.x], prim = p.list[j];
  const Footprint fp = p.fp[j];
  int r0, r1;
  if (!raster_rows(p, fp, r0, r1) || !refined_rows(r0, r1)) return;
  const uint32_t base = p.off[j], total = p.off[j + 1] - base;
  const uint32_t c0 = it.y << p.chunk_shift;
  const uint32_t c1 = c0 + (1u << p.chunk_shift) < total ? c0 + (1u << p.chunk_shift) : total;
  __shared__ TileTri tt;
  __shared__ TileFrame tf;
  __shared__ int tt_ok;
  if (lane == 0) {
    tt_ok = tile_tri(p, (const float*)(p.tri + 3 * (size_t)prim), tt) ? 1 : 0;
    tile_frame(p, tf);
  }
  __syncthreads();
  if (!tt_ok) return;
  for (uint32_t e = c0 + (uint32_t)lane; e < c1; e += 64) {
    // re-read the LDS inputs per entry instead of holding them live across
    // the loop (a compiler memory barrier; 161 -> 80 VGPRs)
    __asm__ volatile("" ::: "memory");
    if (p.key_cap && base + e >= p.key_cap) break;  // not written (ctr[RT_CC_OVERFLOW] is set)
    int tx, ty;
    rt_tile_xy(p.keys[base + e], (uint32_t)p.rank, (uint32_t)p.nranks, (uint32_t)p.blocks_x, (uint32_t)p.tb, &tx, &ty);
    if (!tile_keep(tf, tt, tx, ty)) p.keys[base + e] = p.drop_key;
  }
}

}  // namespace rtc
