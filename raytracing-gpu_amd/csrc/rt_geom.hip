// rt_geom.hip -- geometry updates on the device (rt_hip_set_triangles,
// include/rt_hip.h): the triangles' part of rt_flatten (host/accel.c) for
// triangles that are in device memory already.
//
//   flatten    rt_triangle records (18 floats) -> v0 / e1 / e2 of the
//              prim-order records, the normalised normal rows, the vertex boxes.
//              Pure streaming, 72 B in and 96 B out per triangle: a workgroup
//              moves its 256 triangles' contiguous span through LDS, so every
//              global load and store of a wave is a run of consecutive words
//              (the 72-byte record stride never reaches memory).
//   scene box  exact min / max over every prim's vertex box: per lane, across
//              the wave, across the workgroup, then one workgroup over the
//              partial boxes.  rt_min_f / rt_max_f (host/rt_minmax.h, shared
//              with rt_flatten) are order-independent down to the sign of a
//              zero, so the result is rt_flatten's bit for bit for finite input.
//   zero risk  the per-object flag of host/rt_zero_risk.h from the normal
//              rows, stamped into float 11 of the objects' records.
//
// The arithmetic is the reference's (csrc/rt_device.h twins; the build's
// -ffp-contract=off and correctly rounded divide / sqrt make the normal rows
// bit-identical to rt_v_normalize's).  Vector stores only.
#include "rt_geom.h"

#include "rt_device.h"
#include "rt_kernels.h"
#include "../host/rt_minmax.h"
#include "../host/rt_zero_risk.h"

namespace rtg {

constexpr int kBlock = 256;
constexpr int kInStride = 19;  // 18 floats + 1: the lanes' records start in distinct LDS banks

// One workgroup: triangles [blockIdx.x * 256, + 256) of the range.
__global__ __launch_bounds__(kBlock) void k_flatten(const float* __restrict__ src, uint32_t first, uint32_t count,
                                                    float* __restrict__ rec, float* __restrict__ nrm,
                                                    float* __restrict__ pbox) {
  __shared__ float s_in[kBlock * kInStride];
  __shared__ float s_rec[kBlock * 9];
  __shared__ float s_nrm[kBlock * 9];
  __shared__ float s_box[kBlock * 6];
  const uint32_t t0 = blockIdx.x * (uint32_t)kBlock;
  const uint32_t nt = count - t0 < (uint32_t)kBlock ? count - t0 : (uint32_t)kBlock;  // (t0 < count: the grid)
  const float* in = src + (size_t)t0 * 18;
  for (uint32_t j = threadIdx.x; j < nt * 18; j += kBlock) s_in[(j / 18) * kInStride + j % 18] = in[j];
  __syncthreads();
  if (threadIdx.x < nt) {
    const float* r = &s_in[threadIdx.x * kInStride];
    const rt::f3 v0{r[0], r[1], r[2]}, v1{r[3], r[4], r[5]}, v2{r[6], r[7], r[8]};
    const rt::f3 e1 = rt::sub(v1, v0), e2 = rt::sub(v2, v0);
    float* o = &s_rec[threadIdx.x * 9];
    o[0] = v0.x, o[1] = v0.y, o[2] = v0.z;
    o[3] = e1.x, o[4] = e1.y, o[5] = e1.z;
    o[6] = e2.x, o[7] = e2.y, o[8] = e2.z;
    float* n = &s_nrm[threadIdx.x * 9];
    for (int k = 0; k < 3; k++) {
      const rt::f3 nn = rt::normalize(rt::f3{r[9 + 3 * k], r[10 + 3 * k], r[11 + 3 * k]});
      n[3 * k] = nn.x, n[3 * k + 1] = nn.y, n[3 * k + 2] = nn.z;
    }
    float* b = &s_box[threadIdx.x * 6];
    b[0] = rt_min_f(v0.x, rt_min_f(v1.x, v2.x)), b[3] = rt_max_f(v0.x, rt_max_f(v1.x, v2.x));
    b[1] = rt_min_f(v0.y, rt_min_f(v1.y, v2.y)), b[4] = rt_max_f(v0.y, rt_max_f(v1.y, v2.y));
    b[2] = rt_min_f(v0.z, rt_min_f(v1.z, v2.z)), b[5] = rt_max_f(v0.z, rt_max_f(v1.z, v2.z));
  }
  __syncthreads();
  const size_t p0 = (size_t)first + t0;
  // records: 12 words per prim, words 9..11 (prim, object, flags) stay
  float* orec = rec + p0 * 12;
  for (uint32_t j = threadIdx.x; j < nt * 12; j += kBlock) {
    const uint32_t k = j % 12;
    if (k < 9) orec[j] = s_rec[(j / 12) * 9 + k];
  }
  float* onrm = nrm + p0 * 9;
  for (uint32_t j = threadIdx.x; j < nt * 9; j += kBlock) onrm[j] = s_nrm[j];
  float* obox = pbox + p0 * 6;
  for (uint32_t j = threadIdx.x; j < nt * 6; j += kBlock) obox[j] = s_box[j];
}

struct Box {
  float lo[3], hi[3];
};

__device__ __forceinline__ Box box_empty() {
  return Box{{__FLT_MAX__, __FLT_MAX__, __FLT_MAX__}, {-__FLT_MAX__, -__FLT_MAX__, -__FLT_MAX__}};
}

// The workgroup's box in thread 0: across each wave by shuffles, across the
// waves through LDS.
__device__ __forceinline__ Box box_reduce_block(Box b) {
  __shared__ float s_part[kBlock / 64][6];
  for (int a = 0; a < 3; a++)
    for (int d = 32; d > 0; d >>= 1) {
      b.lo[a] = rt_min_f(b.lo[a], __shfl_xor(b.lo[a], d));
      b.hi[a] = rt_max_f(b.hi[a], __shfl_xor(b.hi[a], d));
    }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; a++) s_part[wave][a] = b.lo[a], s_part[wave][3 + a] = b.hi[a];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBlock / 64; w++)
      for (int a = 0; a < 3; a++) {
        b.lo[a] = rt_min_f(b.lo[a], s_part[w][a]);
        b.hi[a] = rt_max_f(b.hi[a], s_part[w][3 + a]);
      }
  return b;
}

// n boxes of 6 floats (lo.xyz hi.xyz) -> one per workgroup, grid-stride: a
// wave's six loads cover 64 consecutive boxes, every cache line used whole
__global__ __launch_bounds__(kBlock) void k_box(const float* __restrict__ in, uint32_t n, float* __restrict__ out) {
  Box b = box_empty();
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    const float* q = in + 6 * i;
    for (int a = 0; a < 3; a++) {
      b.lo[a] = rt_min_f(b.lo[a], q[a]);
      b.hi[a] = rt_max_f(b.hi[a], q[3 + a]);
    }
  }
  b = box_reduce_block(b);
  if (threadIdx.x == 0)
    for (int a = 0; a < 3; a++) out[6 * blockIdx.x + a] = b.lo[a], out[6 * blockIdx.x + 3 + a] = b.hi[a];
}

__global__ void k_flag_clear(uint32_t* __restrict__ objflag, uint32_t o0, uint32_t o1) {
  const uint32_t o = o0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (o <= o1) objflag[o] = 0u;
}

// prims [p0, p1): an object whose triangle can interpolate a zero normal
__global__ __launch_bounds__(kBlock) void k_flag_eval(const float4* __restrict__ rec, const float* __restrict__ nrm,
                                                      uint32_t p0, uint32_t p1, uint32_t* __restrict__ objflag,
                                                      uint32_t o0, uint32_t o1) {
  const size_t p = (size_t)p0 + (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= p1) return;
  float n[9];
  for (int k = 0; k < 9; k++) n[k] = nrm[9 * p + k];
  if (!rt_zero_risk_rows(n)) return;
  const uint32_t o = __float_as_uint(rec[3 * p + 2].z);
  if (o >= o0 && o <= o1) atomicOr(&objflag[o], 1u);
}

__global__ __launch_bounds__(kBlock) void k_flag_stamp(float4* __restrict__ rec, uint32_t p0, uint32_t p1,
                                                       const uint32_t* __restrict__ objflag, uint32_t o0,
                                                       uint32_t o1) {
  const size_t p = (size_t)p0 + (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= p1) return;
  float* q2 = (float*)&rec[3 * p + 2];
  const uint32_t o = __float_as_uint(q2[2]);
  if (o < o0 || o > o1) return;
  q2[3] = __uint_as_float(objflag[o] ? RT_REC_ZERO_RISK : 0u);
}

}  // namespace rtg

static unsigned geom_blocks(size_t n) { return (unsigned)((n + rtg::kBlock - 1) / rtg::kBlock); }

extern "C" hipError_t rt_geom_flatten(const float* d_src, uint32_t first, uint32_t count, float4* rec,
                                      float* nrm, float* pbox, hipStream_t s) {
  if (!count) return hipSuccess;
  if (!d_src || !rec || !nrm || !pbox) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rtg::k_flatten, dim3(geom_blocks(count)), dim3(rtg::kBlock), 0, s, d_src, first, count,
                     (float*)rec, nrm, pbox);
  return hipGetLastError();
}

extern "C" hipError_t rt_geom_scene_box(const float* pbox, uint32_t nprim, float* d_box, hipStream_t s) {
  if (!nprim || !pbox || !d_box) return hipErrorInvalidValue;
  unsigned nb = geom_blocks(nprim);
  if (nb > RT_GEOM_BOX_BLOCKS) nb = RT_GEOM_BOX_BLOCKS;
  hipLaunchKernelGGL(rtg::k_box, dim3(nb), dim3(rtg::kBlock), 0, s, pbox, nprim, d_box);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rtg::k_box, dim3(1), dim3(rtg::kBlock), 0, s, (const float*)d_box, (uint32_t)nb,
                     d_box + 6 * RT_GEOM_BOX_BLOCKS);
  return hipGetLastError();
}

extern "C" hipError_t rt_geom_zero_risk(float4* rec, const float* nrm, uint32_t p0, uint32_t p1,
                                        uint32_t* objflag, uint32_t o0, uint32_t o1, hipStream_t s) {
  if (p1 <= p0) return hipSuccess;
  if (!rec || !nrm || !objflag || o1 < o0) return hipErrorInvalidValue;
  const uint32_t n = p1 - p0;
  hipLaunchKernelGGL(rtg::k_flag_clear, dim3(geom_blocks((size_t)o1 - o0 + 1)), dim3(rtg::kBlock), 0, s, objflag,
                     o0, o1);
  hipLaunchKernelGGL(rtg::k_flag_eval, dim3(geom_blocks(n)), dim3(rtg::kBlock), 0, s, (const float4*)rec, nrm, p0,
                     p1, objflag, o0, o1);
  hipLaunchKernelGGL(rtg::k_flag_stamp, dim3(geom_blocks(n)), dim3(rtg::kBlock), 0, s, rec, p0, p1,
                     (const uint32_t*)objflag, o0, o1);
  return hipGetLastError();
}
