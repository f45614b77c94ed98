// rt_lightbuf.hip -- light buffers for the shadow queries (rt_lightbuf.h,
// DESIGN.md §4 "Light buffers").  Built once per scene and culling slack, on
// the device: count (cells per triangle) -> scan -> emit (cell, key, prim) ->
// radix sort by (cell, key) -> cell starts.
// The footprints and their proof are rt_lightbuf_geom.h; the grid's
// derivation and the host survey are rt_lightbuf_host.cpp.  Here: the kernels
// and the build that launches them.
#include <hip/hip_runtime.h>
#include <cstring>  // before rocPRIM
#include <rocprim/rocprim.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_counters.h"
#include "rt_lightbuf_geom.h"
#include "rt_mem.h"

namespace rtl {

constexpr int kBlock = 256;

// The kernels' parameter: the geometry, then the build's device memory.
struct BP : LbGeom {
  uint32_t* count;
  uint32_t* off;
  unsigned long long* keys;
  uint32_t* vals;
  uint32_t* big;
  uint32_t* ctr;  // RT_LBC_WORDS counters (rt_counters.h RtLbCtr)
  uint32_t* global;
};

__global__ __launch_bounds__(256) void rmin_kernel(BP p, uint32_t* bits) {
  const uint32_t prim = blockIdx.x * blockDim.x + threadIdx.x;
  if (prim >= p.nprim) return;
  const double dist = prim_rmin(p, prim);
  const float fd = dist > 0.0 ? __double2float_rd(dist) : 0.0f;
  atomicMin(bits, __float_as_uint(fd));  // non-negative floats order as their bits
}

__global__ __launch_bounds__(256) void count_kernel(BP p) {
  const uint32_t prim = blockIdx.x * blockDim.x + threadIdx.x;
  if (prim >= p.nprim) return;
  Foot f;
  footprint(p, prim, f);
  uint32_t c = 0;
  if (f.never) {
    atomicAdd(p.ctr + RT_LBC_NEVER, 1u);
  } else if (f.global) {
    p.global[atomicAdd(p.ctr + RT_LBC_GLOBAL, 1u)] = prim;
  } else if (foot_is_big(p, f)) {
    p.big[atomicAdd(p.ctr + RT_LBC_BIG, 1u)] = prim;  // counted and emitted row-wise by a workgroup
    if (f.band) atomicAdd(p.ctr + RT_LBC_BAND, 1u);
  } else {
    const uint32_t rows = foot_rows(p, f);
    for (uint32_t r = 0; r < rows; r++) c += row_entries<false>(p, f, prim, r, 0, 0);
  }
  p.count[prim] = c;  // the host checks the total against 2^31
}

__device__ inline uint32_t block_sum(uint32_t v, uint32_t* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = v;
  __syncthreads();
  uint32_t t = 0;
  for (int w = 0; w < kBlock / 64; w++) t += red[w];
  __syncthreads();
  return t;
}

// one workgroup per big footprint: its rows over the threads
__global__ __launch_bounds__(256) void big_count_kernel(BP p) {
  __shared__ uint32_t red[kBlock / 64];
  for (uint32_t b = blockIdx.x; b < p.ctr[RT_LBC_BIG]; b += gridDim.x) {
    const uint32_t prim = p.big[b];
    Foot f;
    footprint(p, prim, f);
    const uint32_t rows = foot_rows(p, f);
    uint32_t s = 0;
    for (uint32_t r = threadIdx.x; r < rows; r += kBlock) s += row_entries<false>(p, f, prim, r, 0, 0);
    const uint32_t t = block_sum(s, red);
    if (threadIdx.x == 0) p.count[prim] = t;
  }
}

__global__ __launch_bounds__(256) void emit_kernel(BP p) {
  const uint32_t prim = blockIdx.x * blockDim.x + threadIdx.x;
  if (prim >= p.nprim) return;
  if (p.count[prim] == 0) return;
  Foot f;
  footprint(p, prim, f);
  if (f.never || f.global || foot_is_big(p, f)) return;  // big: big_emit_kernel
  uint64_t at = p.off[prim];
  const uint64_t lim = at + p.count[prim];
  const uint32_t rows = foot_rows(p, f);
  for (uint32_t r = 0; r < rows; r++) at += row_entries<true>(p, f, prim, r, at, lim);
}

// one workgroup per big footprint: 256 rows at a time, each row's entries at
// its exclusive prefix within the block
__global__ __launch_bounds__(256) void big_emit_kernel(BP p) {
  __shared__ uint32_t wsum[kBlock / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (uint32_t b = blockIdx.x; b < p.ctr[RT_LBC_BIG]; b += gridDim.x) {
    const uint32_t prim = p.big[b];
    Foot f;
    footprint(p, prim, f);
    const uint32_t rows = foot_rows(p, f);
    uint64_t base = p.off[prim];
    const uint64_t lim = base + p.count[prim];
    for (uint32_t r0 = 0; r0 < rows; r0 += kBlock) {
      const uint32_t r = r0 + threadIdx.x;
      const uint32_t c = r < rows ? row_entries<false>(p, f, prim, r, 0, 0) : 0u;
      uint32_t incl = c;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
      }
      if (lane == 63) wsum[wid] = incl;
      __syncthreads();
      uint32_t woff = 0, tot = 0;
      for (int w = 0; w < kBlock / 64; w++) {
        if (w < wid) woff += wsum[w];
        tot += wsum[w];
      }
      if (c) row_entries<true>(p, f, prim, r, base + woff + incl - c, lim);
      base += tot;
      __syncthreads();
    }
  }
}

// sorted (cell, key) pairs and prims -> per-entry records with the key in
// the prim slot
__global__ __launch_bounds__(256) void rec_kernel(const unsigned long long* keys, const uint32_t* prim,
                                                  const float4* tri, uint32_t n, float4* rec) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4* t = tri + 3 * (size_t)prim[i];
  float4 q2 = t[2];
  q2.y = unorder((uint32_t)keys[i]);
  rec[3 * (size_t)i] = t[0];
  rec[3 * (size_t)i + 1] = t[1];
  rec[3 * (size_t)i + 2] = q2;
}

// start[c] = the first entry of a cell >= c (binary search; empty cells get
// their successor's start), c = 0 .. ncell
__global__ __launch_bounds__(256) void start_kernel(const unsigned long long* keys, uint32_t n,
                                                    uint32_t ncell, uint32_t* start) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ncell) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint32_t)(keys[mid] >> 32) < c)
      lo = mid + 1;
    else
      hi = mid;
  }
  start[c] = lo;
}

}  // namespace rtl

struct LBDevice {
  DevBuf<uint32_t> start, prim, global;
  DevBuf<float4> rec;
  unsigned long long entries = 0, cells = 0, nglobal = 0, never = 0, band = 0;
};

extern "C" void rt_lightbuf_free(LBDevice* d) { delete d; }

extern "C" void rt_lightbuf_sizes(const LBDevice* d, unsigned long long* entries, unsigned long long* cells,
                                  unsigned long long* global) {
  *entries = d ? d->entries : 0;
  *cells = d ? d->cells : 0;
  *global = d ? d->nglobal : 0;
}

extern "C" void rt_lightbuf_proof_counts(const LBDevice* d, unsigned long long* never, unsigned long long* band) {
  *never = d ? d->never : 0;
  *band = d ? d->band : 0;
}

#define LB_TRY(x)                                                 \
  do {                                                            \
    hipError_t e_ = (x);                                          \
    if (e_ != hipSuccess) {                                       \
      snprintf(err, errlen, "%s: %s", #x, hipGetErrorString(e_)); \
      return e_ == hipErrorOutOfMemory ? 1 : -1;                  \
    }                                                             \
  } while (0)

// The build proper, into dev's buffers (freed by the caller on failure; the
// build's own memory is freed on every return).
static int lb_build(const LBParams* in, rtl::BP& p, uint64_t ncell, RtLightBuf* out, LBDevice* dev, hipStream_t s,
                    char* err, size_t errlen) {
  using namespace rtl;
  uint64_t total = 0;
  DevBuf<uint32_t> count, off, ctr, big, rmin, v0;
  DevBuf<unsigned long long> k0, k1;
  DevBuf<void> tmp;
  size_t tb = 0;
  uint32_t hc[RT_LBC_WORDS] = {}, last_off = 0, last_cnt = 0;
  const uint32_t np = in->nprim;
  const dim3 gp((np + 255) / 256), bk(256);
  LB_TRY(count.alloc((size_t)np + 1));
  LB_TRY(off.alloc((size_t)np + 1));
  LB_TRY(ctr.alloc(RT_LBC_WORDS));
  LB_TRY(big.alloc((size_t)np + 1));
  LB_TRY(dev->global.alloc((size_t)np + 1));
  LB_TRY(dev->start.alloc(ncell + 1));
  LB_TRY(hipMemsetAsync(ctr, 0, RT_LBC_WORDS * sizeof(uint32_t), s));
  LB_TRY(hipMemsetAsync(count + np, 0, sizeof(uint32_t), s));
  p.count = count;
  p.off = off;
  p.ctr = ctr;
  p.big = big;
  p.global = dev->global;
  if (p.proven && p.kind == RT_LB_POINT) {
    // the nearest shadow-ray origin's distance from the light (band widths)
    LB_TRY(rmin.alloc(1));
    LB_TRY(hipMemsetAsync(rmin, 0x7f, sizeof(uint32_t), s));  // 0x7f7f7f7f: a large float
    if (np) hipLaunchKernelGGL(rmin_kernel, gp, bk, 0, s, p, rmin.get());
    LB_TRY(hipGetLastError());
    uint32_t rb = 0;
    LB_TRY(hipMemcpyAsync(&rb, rmin, sizeof rb, hipMemcpyDeviceToHost, s));
    LB_TRY(hipStreamSynchronize(s));
    float rf;
    std::memcpy(&rf, &rb, sizeof rf);
    p.rmin_o = (double)rf;
  }
  if (np) hipLaunchKernelGGL(count_kernel, gp, bk, 0, s, p);
  LB_TRY(hipGetLastError());
  hipLaunchKernelGGL(big_count_kernel, dim3(2048), bk, 0, s, p);
  LB_TRY(hipGetLastError());
  // (not with_tmp: its headroom is the candidate lists', these sizes are the build's own)
  LB_TRY(rocprim::exclusive_scan(nullptr, tb, p.count, p.off, 0u, (size_t)np + 1, rocprim::plus<uint32_t>(), s));
  LB_TRY(tmp.alloc(tb + 16));
  LB_TRY(rocprim::exclusive_scan(tmp.get(), tb, p.count, p.off, 0u, (size_t)np + 1, rocprim::plus<uint32_t>(), s));
  LB_TRY(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, s));
  if (np) {
    LB_TRY(hipMemcpyAsync(&last_off, off + np - 1, sizeof last_off, hipMemcpyDeviceToHost, s));
    LB_TRY(hipMemcpyAsync(&last_cnt, count + np - 1, sizeof last_cnt, hipMemcpyDeviceToHost, s));
  }
  LB_TRY(hipStreamSynchronize(s));
  total = (uint64_t)last_off + last_cnt;  // the 32-bit scan wrapped if the true total is >= 2^32
  {
    // a wrapped scan would show as offsets going down: check the exact sum on the host side
    // through the per-prim maximum (each count <= ncell < 2^31) and np
    if ((uint64_t)np * (uint64_t)ncell >= (1ull << 32)) {
      // possible overflow: recount in 64 bits
      unsigned long long sum = 0;
      std::vector<uint32_t> hcnt(np);
      LB_TRY(hipMemcpy(hcnt.data(), count, (size_t)np * sizeof(uint32_t), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < np; i++) sum += hcnt[i];
      total = sum;
    }
  }
  if (total >= (1ull << 31) || (in->max_entries && total > in->max_entries)) {
    snprintf(err, errlen, "light buffer of %llu entries", (unsigned long long)total);
    return 1;
  }
  dev->entries = total;
  dev->cells = ncell;
  dev->nglobal = hc[RT_LBC_GLOBAL];
  dev->never = hc[RT_LBC_NEVER];
  dev->band = hc[RT_LBC_BAND];
  LB_TRY(dev->prim.alloc(total + 1));
  LB_TRY(dev->rec.alloc((total + 1) * 3));
  if (total) {
    LB_TRY(k0.alloc(total));
    LB_TRY(k1.alloc(total));
    LB_TRY(v0.alloc(total));
    p.keys = k0;
    p.vals = v0;
    hipLaunchKernelGGL(emit_kernel, gp, bk, 0, s, p);
    LB_TRY(hipGetLastError());
    if (const uint32_t nbig = hc[RT_LBC_BIG]) {
      hipLaunchKernelGGL(big_emit_kernel, dim3(nbig < 4096 ? nbig : 4096), bk, 0, s, p);
      LB_TRY(hipGetLastError());
    }
    int bits = 32;
    while ((1ull << (bits - 32)) <= ncell) bits++;
    size_t sb = 0;
    LB_TRY(rocprim::radix_sort_pairs(nullptr, sb, p.keys, k1.get(), p.vals, dev->prim.get(), (size_t)total, 0, bits, s));
    if (sb > tb) {
      LB_TRY(tmp.alloc(sb + 16));
      tb = sb;
    }
    sb = tb;
    LB_TRY(rocprim::radix_sort_pairs(tmp.get(), sb, p.keys, k1.get(), p.vals, dev->prim.get(), (size_t)total, 0, bits,
                                     s));
    hipLaunchKernelGGL(rec_kernel, dim3((uint32_t)((total + 255) / 256)), bk, 0, s, k1.get(), dev->prim.get(), p.tri,
                       (uint32_t)total, dev->rec.get());
    LB_TRY(hipGetLastError());
    hipLaunchKernelGGL(start_kernel, dim3((uint32_t)((ncell + 256) / 256)), bk, 0, s, k1.get(), (uint32_t)total,
                       (uint32_t)ncell, dev->start.get());
    LB_TRY(hipGetLastError());
  } else {
    LB_TRY(hipMemsetAsync(dev->start, 0, (ncell + 1) * sizeof(uint32_t), s));
  }
  LB_TRY(hipMemcpyAsync(hc + RT_LBC_OVERFLOW, ctr + RT_LBC_OVERFLOW, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  LB_TRY(hipStreamSynchronize(s));
  if (hc[RT_LBC_OVERFLOW]) {
    snprintf(err, errlen, "light buffer emission disagreed with its count");
    return -1;
  }
  out->start = dev->start;
  out->rec = dev->rec;
  out->global = dev->global;
  out->nglobal = hc[RT_LBC_GLOBAL];
  return 0;
}

extern "C" int rt_lightbuf_build(const LBParams* in, RtLightBuf* out, LBDevice** devp, hipStream_t s,
                                 char* err, size_t errlen) {
  rtl::BP p{};
  uint64_t ncell = 0;
  *devp = nullptr;
  if (const int r = lb_derive_grid(in, p, out, ncell, err, errlen)) return r;
  LBDevice* dev = new LBDevice();
  const int rc = lb_build(in, p, ncell, out, dev, s, err, errlen);
  if (rc) {
    delete dev;
    std::memset(out, 0, sizeof *out);
  } else {
    *devp = dev;
  }
  return rc;
}
