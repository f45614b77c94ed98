// rt_paths.hip -- the kernels of the path export (include/rt_hip.h
// rt_hip_path_records): the kept ray batch's chains of hit records written out
// as a CSR offset per ray and, per path vertex, an rt_gsample, the vertex's
// coef and its shaded term.  A translation unit of its own: it reads the hit
// buffers the trace and shade passes of rt_render.hip left and shares no code
// with them, so theirs stays as it is.  A ray's chain is the one
// rays_fold_kernel walks, under its loop condition (csrc/rt_rays.h): from
// last[i], while the index is a record's and its slot lies in the buffers,
// along hit_prev -- deepest vertex first, so the export stores in reverse.
// Three launches, none waiting for another workgroup (PathArgs, rt_kernels.h);
// the blocks, the scratch words, the chunks and a record's address are
// csrc/rt_path_items.h; the launches csrc/rt_paths.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernels.h"
#include "rt_path_items.h"

static_assert(RT_REC_REGIONS == RT_HIT_REGIONS, "rt_path_items.h addresses the regions of rt_kernels.h");
static_assert(RT_PATH_BLOCK % 64u == 0 && RT_PATH_CHUNK % 64u == 0 && RT_PATH_CHUNK <= 1024u, "whole waves");

namespace rtp {

// exclusive scan of one value per thread over a block of THREADS threads
// (whole waves; sh: THREADS / 64 words); *sum = the block's total.  The wave
// scan by __shfl_up plus LDS of csrc/rt_scan.h block_excl_scan.
template <uint32_t THREADS>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* sh, uint32_t* sum) {
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  uint32_t inc = x;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(inc, o, 64);
    if ((int)lane >= o) inc += y;
  }
  if (lane == 63u) sh[wv] = inc;
  __syncthreads();
  uint32_t before = 0, tot = 0;
  for (uint32_t k = 0; k < THREADS / 64u; k++) {
    const uint32_t s = sh[k];
    if (k < wv) before += s;
    tot += s;
  }
  __syncthreads();
  *sum = tot;
  return before + inc - x;
}

// does index r name a record the buffers hold (rays_fold_kernel's condition)
__device__ __forceinline__ bool rec_held(const PathArgs& a, uint32_t r) {
  return r != RT_NO_REC && rt_path_slot(r) < a.hit_cap;
}

// 1. Lengths: lane = ray.  The chain's length, bounded by RT_MAX_BOUNCES steps
// so that a damaged link cannot spin, to offsets[i]; the block's total to btot.
__global__ __launch_bounds__(RT_PATH_BLOCK) void path_lengths_kernel(PathArgs a) {
  __shared__ uint32_t sh[RT_PATH_BLOCK / 64u];
  const unsigned long long i = (unsigned long long)blockIdx.x * RT_PATH_BLOCK + threadIdx.x;
  uint32_t len = 0;
  if (i < a.n) {
    uint32_t r = a.last[i];
    while (rec_held(a, r) && len < (uint32_t)RT_MAX_BOUNCES) {
      len++;
      r = a.hit_prev[rt_path_rec_addr(r, a.hit_cap)];
    }
    a.offsets[i] = len;
  }
  uint32_t tot;
  block_excl_scan<RT_PATH_BLOCK>(len, sh, &tot);
  if (threadIdx.x == 0) a.btot[blockIdx.x] = tot;
}

// 2. Block totals: one workgroup turns btot into the blocks' bases in place,
// RT_PATH_CHUNK of them per step with a running carry, and writes the total
// of all to offsets[n].
__global__ __launch_bounds__(RT_PATH_CHUNK) void path_totals_kernel(PathArgs a) {
  __shared__ uint32_t sh[RT_PATH_CHUNK / 64u];
  uint32_t carry = 0;
  const uint32_t chunks = rt_path_chunks(a.nblocks);
  for (uint32_t c = 0; c < chunks; c++) {
    const uint32_t b = c * RT_PATH_CHUNK + threadIdx.x;  // (nblocks <= 2^24: no wrap)
    const uint32_t x = b < a.nblocks ? a.btot[b] : 0u;
    uint32_t tot;
    const uint32_t before = block_excl_scan<RT_PATH_CHUNK>(x, sh, &tot);
    if (b < a.nblocks) a.btot[b] = carry + before;
    carry += tot;
  }
  if (threadIdx.x == 0) a.offsets[a.n] = carry;
}

// 3. Write: the block's lengths scanned onto its base are the rays' offsets;
// each lane then walks its chain again and stores the record `step` links from
// the deepest as vertex len - 1 - step, if that vertex lies below cap: the
// rt_gsample as five 8-byte stores (prim obj | queries dist | P.x P.y | P.z
// N.x | N.y N.z), then coef, then the term's three words.
__global__ __launch_bounds__(RT_PATH_BLOCK) void path_write_kernel(PathArgs a) {
  __shared__ uint32_t sh[RT_PATH_BLOCK / 64u];
  const unsigned long long i = (unsigned long long)blockIdx.x * RT_PATH_BLOCK + threadIdx.x;
  const uint32_t len = i < a.n ? a.offsets[i] : 0u;
  uint32_t tot;
  const uint32_t off = a.btot[blockIdx.x] + block_excl_scan<RT_PATH_BLOCK>(len, sh, &tot);
  if (i >= a.n) return;
  a.offsets[i] = off;
  if (!a.records && !a.coef && !a.terms) return;
  uint32_t r = a.last[i];
  for (uint32_t step = 0; step < len && rec_held(a, r); step++) {
    const size_t at = rt_path_rec_addr(r, a.hit_cap);
    const uint32_t v = len - 1u - step;
    const unsigned long long j = (unsigned long long)off + v;
    if (j < a.cap) {
      const float4 h1 = a.hit[2 * at + 1];
      if (a.records) {
        const float4 h0 = a.hit[2 * at];
        uint2* o = a.records + 5 * j;
        o[0] = make_uint2((uint32_t)RT_PATH_PRIM_D, __float_as_uint(h1.w));
        o[1] = make_uint2(v, 0u);
        o[2] = make_uint2(__float_as_uint(h0.x), __float_as_uint(h0.y));
        o[3] = make_uint2(__float_as_uint(h0.z), __float_as_uint(h0.w));
        o[4] = make_uint2(__float_as_uint(h1.x), __float_as_uint(h1.y));
      }
      if (a.coef) a.coef[j] = h1.z;
      if (a.terms) {
        const float4 tm = a.hit_term[at];
        float* t = a.terms + 3 * j;
        t[0] = tm.x;
        t[1] = tm.y;
        t[2] = tm.z;
      }
    }
    r = a.hit_prev[at];
  }
}

}  // namespace rtp

extern "C" hipError_t rt_launch_path_lengths(const PathArgs* a, hipStream_t stream) {
  if (a->nblocks == 0 || a->nblocks != rt_path_blocks(a->n)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rtp::path_lengths_kernel, dim3(a->nblocks), dim3(RT_PATH_BLOCK), 0, stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_path_totals(const PathArgs* a, hipStream_t stream) {
  if (a->nblocks == 0 || a->nblocks != rt_path_blocks(a->n)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rtp::path_totals_kernel, dim3(1), dim3(RT_PATH_CHUNK), 0, stream, *a);
  return hipGetLastError();
}

extern "C" hipError_t rt_launch_path_write(const PathArgs* a, hipStream_t stream) {
  if (a->nblocks == 0 || a->nblocks != rt_path_blocks(a->n)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rtp::path_write_kernel, dim3(a->nblocks), dim3(RT_PATH_BLOCK), 0, stream, *a);
  return hipGetLastError();
}
