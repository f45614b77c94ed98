// rt_cand_entries.h -- what happens to the entries the list passes emitted,
// and the scene-time leaf of each prim: prim_leaf_kernel; the sorted lists'
// per-tile bounds and per-entry depth-skip bounds (bounds_kernel,
// entry_skip_kernel); the triangle-parallel multi-GPU exchange (route_key,
// route_globals_kernel, part_count_kernel / part_scatter_kernel,
// unpack_kernel, gather_kernel; rt_cand.h "route"); the compaction of the
// entries the refinement dropped (compact_count_kernel /
// compact_scatter_kernel); and the heavy-first work order of the tiles
// (heavy_flag_kernel, heavy_perm_kernel).  Integer work on keys and indices:
// nothing here reads a Footprint or calls the geometry.
// Part of rt_cand.hip's one translation unit.  Needs the tile map
// (rt_tiles.h) and the counter words (rt_counters.h, through rt_cand.h),
// included here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cand.h"
#include "rt_tiles.h"

namespace rtc {

__global__ __launch_bounds__(256) void prim_leaf_kernel(const float4* node, uint32_t nnode,
                                                        const float4* tri, uint32_t* prim_leaf) {
  const uint32_t ni = blockIdx.x * blockDim.x + threadIdx.x;
  if (ni >= nnode) return;
  const uint32_t first = __float_as_uint(node[2 * ni].w), info = __float_as_uint(node[2 * ni + 1].w);
  if (!(info & 0x80000000u)) return;  // RT_NODE_LEAF
  const uint32_t cnt = info & 0x7fffffffu;
  // the smallest leaf index holding the prim (a prim referenced by several
  // leaves -- the host SAH tree duplicates -- gets the same leaf on every
  // build, so the lists do not depend on the order of these writes)
  for (uint32_t k = 0; k < cnt; k++) atomicMin(prim_leaf + __float_as_uint(tri[3 * (size_t)(first + k) + 2].y), ni);
}

// start[t] = first entry of tile t in the tile-sorted keys; start[ntiles] =
// the entries with a tile (the refinement's dropped entries, key ntiles, sort
// after them)
__global__ __launch_bounds__(256) void bounds_kernel(const uint32_t* keys, uint32_t n, uint32_t* start,
                                                     uint32_t ntiles, uint32_t* snap) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  // an asynchronous build's counters -> the block's snapshot region for
  // rt_hip_stats, after every pass that may set its overflow flag
  if (snap && t < RT_CC_BUILD_WORDS) snap[RT_CAND_CTR_SNAPSHOT + t] = snap[t];
  if (t > ntiles) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < t)
      lo = mid + 1;
    else
      hi = mid;
  }
  start[t] = lo;
}

// per list entry: the depth-skip bound of its prim (coalesced for the render
// kernel, which would otherwise gather it right after loading the entry)
// n_dev (optional): the entries with a tile, start[ntiles] -- the ones the
// refinement dropped sort after them and are never read
__global__ __launch_bounds__(256) void entry_skip_kernel(const uint32_t* cand, const float* skip,
                                                         float* out, uint32_t n, const uint32_t* n_dev) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!n_dev || i < *n_dev)) out[i] = skip[cand[i]];
}

// --- triangle-parallel multi-GPU lists (rt_cand.h "route") ---------------
// A whole-frame entry (scanline tile of the one-rank map) -> its rank d and
// rank-local tile l under the N-rank block map: key d << tbits | l (l <= tpr
// < 2^tbits), partitioned by d below.
__device__ __forceinline__ uint32_t route_key(uint32_t t, int tiles_x, int nranks, int blocks_x, int tb,
                                              uint32_t tbits, uint32_t drop_key) {
  if (t == drop_key) return (uint32_t)nranks << tbits;  // dropped by the refinement: after every rank's entries
  uint32_t d;
  const uint32_t l = rt_tile_local((int)(t % (uint32_t)tiles_x), (int)(t / (uint32_t)tiles_x), (uint32_t)nranks,
                                   (uint32_t)blocks_x, (uint32_t)tb, &d);
  return d << tbits | l;
}

// the slice's globals: one entry per rank, local slot tpr
__global__ __launch_bounds__(256) void route_globals_kernel(const uint32_t* global, uint32_t nglobal, int nranks,
                                                            uint32_t tpr, uint32_t tbits, uint32_t* keys,
                                                            uint32_t* vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nglobal * (uint32_t)nranks) return;
  const uint32_t d = i / nglobal, g = i % nglobal;
  keys[i] = d << tbits | tpr;
  vals[i] = global[g];
}

// Stable partition of the routed entries by destination rank, packed for
// the exchange (replaces a radix sort on the rank bits + rank_bounds + pack:
// 3 launches and a scan instead of 9; the produce step is latency-bound at
// 1/N of a frame).  Wave w owns entries [w kPartChunk, (w + 1) kPartChunk);
// part_count_kernel -> hist[d nw + w] = its entries of rank d (d <= nranks,
// nranks = dropped) -> exclusive scan (rank-major: every rank's entries in
// wave order) -> part_scatter_kernel writes each entry at its rank's running
// offset, in entry order (a per-step ballot per distinct rank), 3 words
// (local tile or tpr, prim, skip bits); start[d] = hist offset of (d, 0).
constexpr uint32_t kPartSteps = 16, kPartChunk = 64 * kPartSteps;

// (with the routing of the entries [0, nroute) fused in: route_key's
// key, written back for part_scatter; the globals past them come routed)
__global__ __launch_bounds__(64) void part_count_kernel(uint32_t* keys, uint32_t n, uint32_t tbits, int nranks,
                                                        uint32_t* hist, uint32_t nroute, int tiles_x, int blocks_x,
                                                        int tb, uint32_t drop_key, const uint32_t* total_dev) {
  __shared__ uint32_t cnt[257];
  const int lane = threadIdx.x;
  const uint32_t nw = gridDim.x, w = blockIdx.x;
  for (int d = lane; d <= nranks; d += 64) cnt[d] = 0u;
  __syncthreads();
  const uint32_t e0 = w * kPartChunk, e1 = e0 + kPartChunk < n ? e0 + kPartChunk : n;
  const uint32_t own = total_dev ? *total_dev : nroute;  // entries the build wrote (async: <= nroute)
  uint32_t k[kPartSteps];  // every load in flight at once (the pass is latency-bound)
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++) {
    const uint32_t i = e0 + t * 64u + (uint32_t)lane;
    k[t] = i < e1 ? keys[i] : 0u;
  }
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++) {
    const uint32_t i = e0 + t * 64u + (uint32_t)lane;
    if (i < e1 && i < nroute) {
      const uint32_t key = route_key(i < own ? k[t] : drop_key, tiles_x, nranks, blocks_x, tb, tbits, drop_key);
      keys[i] = key;
      k[t] = key;
    }
    k[t] = i < e1 ? k[t] >> tbits : 0xffffffffu;
  }
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++)
    if (k[t] != 0xffffffffu) atomicAdd(&cnt[k[t]], 1u);
  __syncthreads();
  for (int d = lane; d <= nranks; d += 64) hist[(size_t)d * nw + w] = cnt[d];
}

__global__ __launch_bounds__(64) void part_scatter_kernel(const uint32_t* keys, const uint32_t* prims,
                                                          const float* skip, uint32_t n, uint32_t tbits, int nranks,
                                                          const uint32_t* off, uint32_t* start, uint32_t* out,
                                                          const uint32_t* ctr) {
  __shared__ uint32_t base[257];
  const int lane = threadIdx.x;
  const uint32_t nw = (n + kPartChunk - 1) / kPartChunk, w = blockIdx.x;  // (one workgroup when n = 0)
  for (int d = lane; d <= nranks; d += 64) {
    base[d] = nw ? off[(size_t)d * nw + w] : 0u;
    if (w == 0) start[d] = base[d];
  }
  // the build's counters beside the starts: the host reads both in one copy
  if (w == 0 && lane < (int)RT_CC_BUILD_WORDS) start[rt_rstart_ctr(nranks) + lane] = ctr[lane];
  __syncthreads();
  const uint32_t e0 = w * kPartChunk, e1 = e0 + kPartChunk < n ? e0 + kPartChunk : n;
  const uint64_t lt = (1ull << lane) - 1ull;
  uint32_t kk[kPartSteps], pr[kPartSteps];
  float sk[kPartSteps];
  // the chunk's keys, prims and skip bounds in flight at once (latency-bound)
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++) {
    const uint32_t i = e0 + t * 64u + (uint32_t)lane;
    kk[t] = i < e1 ? keys[i] : 0xffffffffu;
    pr[t] = i < e1 ? prims[i] : 0u;
  }
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++) sk[t] = kk[t] != 0xffffffffu ? skip[pr[t]] : 0.0f;
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++) {
    const uint32_t i = e0 + t * 64u + (uint32_t)lane;
    if (e0 + t * 64u >= e1) break;
    const bool valid = i < e1;
    const uint32_t key = kk[t];
    const uint32_t d = key >> tbits;
    uint64_t left = __ballot(valid);
    uint32_t pos = 0;
    while (left) {  // one round per distinct rank of this step's entries
      const int first = __ffsll((long long)left) - 1;
      const uint32_t dd = (uint32_t)__shfl((int)d, first, 64);
      const uint64_t m = __ballot(valid && d == dd) & left;
      // (one wave: its LDS read of base[dd] completes before its write)
      const uint32_t b = base[dd];
      if (valid && d == dd) pos = b + (uint32_t)__popcll(m & lt);
      if (lane == first) base[dd] = b + (uint32_t)__popcll(m);
      left &= ~m;
    }
    if (valid && d < (uint32_t)nranks) {
      out[3 * (size_t)pos] = key & ((1u << tbits) - 1u);
      out[3 * (size_t)pos + 1] = pr[t];
      out[3 * (size_t)pos + 2] = __float_as_uint(sk[t]);
    }
  }
}

// Stable compaction of the (key, value) entries whose key is not drop_key
// (the per-tile refinement drops ~55 % of C5's entries: the sort then runs
// over the kept ones only).  Wave w owns entries [w kPartChunk, (w + 1)
// kPartChunk): compact_count_kernel -> cnt[w] -> exclusive scan (off, off[nw]
// = the kept total) -> compact_scatter_kernel writes the kept entries in
// order at off[w] + their rank in the wave; past cap they are not written
// and over_flag is set (the host sized cap from the same frame's earlier build).
__global__ __launch_bounds__(64) void compact_count_kernel(const uint32_t* keys, uint32_t n, uint32_t drop_key,
                                                           uint32_t* cnt, const uint32_t* n_dev) {
  const int lane = threadIdx.x;
  const uint32_t e0 = blockIdx.x * kPartChunk;
  const uint32_t m = n_dev && *n_dev < n ? *n_dev : n;  // the build's own entries (the rest: unused)
  uint32_t c = 0;
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++) {
    const uint32_t i = e0 + t * 64u + (uint32_t)lane;
    c += (i < m && keys[i] != drop_key) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) cnt[blockIdx.x] = c;
  if (blockIdx.x == 0 && lane == 0) cnt[gridDim.x] = 0u;  // the scan's last input
}

__global__ __launch_bounds__(64) void compact_scatter_kernel(const uint32_t* keys, const uint32_t* vals, uint32_t n,
                                                             uint32_t drop_key, const uint32_t* off, uint32_t cap,
                                                             uint32_t* keys_out, uint32_t* vals_out, uint32_t* over_flag,
                                                             const uint32_t* n_dev) {
  const int lane = threadIdx.x;
  const uint32_t e0 = blockIdx.x * kPartChunk;
  const uint64_t lt = (1ull << lane) - 1ull;
  const uint32_t m = n_dev && *n_dev < n ? *n_dev : n;
  // fewer kept entries than cap -- never expected for the same frame -- leave
  // a tail: dropped (every workgroup a strided part of it)
  for (uint32_t i = off[gridDim.x] + blockIdx.x * 64u + (uint32_t)lane; i < cap; i += gridDim.x * 64u)
    keys_out[i] = drop_key;
  uint32_t k[kPartSteps], v[kPartSteps];
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++) {
    const uint32_t i = e0 + t * 64u + (uint32_t)lane;
    k[t] = i < m ? keys[i] : drop_key;
    v[t] = i < m ? vals[i] : 0u;
  }
  uint32_t base = off[blockIdx.x];
#pragma unroll
  for (uint32_t t = 0; t < kPartSteps; t++) {
    const bool keep = k[t] != drop_key;
    const uint64_t m = __ballot(keep);
    const uint32_t pos = base + (uint32_t)__popcll(m & lt);
    if (keep) {
      if (pos < cap) {
        keys_out[pos] = k[t];
        vals_out[pos] = v[t];
      } else {
        *over_flag = 1u;
      }
    }
    base += (uint32_t)__popcll(m);
  }
}

__global__ __launch_bounds__(256) void unpack_kernel(const uint32_t* in, uint32_t n, uint32_t ntiles, uint32_t tpr,
                                                     uint32_t* keys, uint32_t* idx) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = in[3 * (size_t)i];
  keys[i] = l >= tpr ? ntiles : l;  // the globals after every tile
  idx[i] = i;
}

__global__ __launch_bounds__(256) void gather_kernel(const uint32_t* in, const uint32_t* idx, uint32_t n,
                                                     uint32_t* cand, float* skip) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const size_t k = 3 * (size_t)idx[j];
  cand[j] = in[k + 1];
  skip[j] = __uint_as_float(in[k + 2]);
}

// Work order of the trace kernel's tiles (longest processing time first): a
// tile's camera-candidate entries predict its cost (r = 0.89 on C5,
// tools/tile_cost.py), so tiles with more than 8x the mean go first and the
// persistent waves' last items are short ones.  flags -> exclusive scan ->
// perm: heavy tiles first, then the rest, each in their own order.
// a tile is heavy when its list is longer than 8x the mean; the mean over
// the entries with a tile (start[ntiles], read here: the host's total also
// counts the entries the refinement dropped).
// Also heavy (item_cost != NULL: the same frame rendered before on this
// context): a tile one of whose items took more than a quarter of a
// balanced wave's share of that trace (cost_sum / waves).  Long reflection
// chains cost little camera-candidate work -- C5's worst items at N = 8 are
// mirror paths through tiles of 30-60 entries -- and one of them started
// late ran past every other wave: rank 0 of 8 traced in 1.23 ms against
// 0.88-0.97 for the others with the same total clocks (tools/tile_cost.py).
__global__ __launch_bounds__(256) void heavy_flag_kernel(const uint32_t* start, uint32_t ntiles,
                                                         uint32_t* flags, const uint32_t* item_cost,
                                                         const unsigned long long* cost_sum, uint32_t waves) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > ntiles) return;
  const uint32_t total = start[ntiles] - start[0];
  bool heavy = t < ntiles && (unsigned long long)(start[t + 1] - start[t]) * ntiles > 8ull * (unsigned long long)total;
  if (item_cost && t < ntiles && !heavy) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) m = item_cost[4 * (size_t)t + k] > m ? item_cost[4 * (size_t)t + k] : m;
    heavy = 4.0 * (double)m * (double)waves > (double)*cost_sum;
  }
  flags[t] = heavy ? 1u : 0u;
}

__global__ __launch_bounds__(256) void heavy_perm_kernel(const uint32_t* flags, const uint32_t* pos,
                                                         uint32_t ntiles, uint32_t* perm) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t nheavy = pos[ntiles];
  perm[flags[t] ? pos[t] : nheavy + t - pos[t]] = t;
}

}  // namespace rtc
