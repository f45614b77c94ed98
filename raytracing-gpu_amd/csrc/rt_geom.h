// rt_geom.h -- geometry updates on the device (rt_geom.hip): what rt_flatten
// (host/accel.c) derives from a scene's triangles, derived from triangles
// that already sit in device memory; internal, not the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// workgroups of the scene-box reduction's first pass; its buffer holds
// 6 floats (lo.xyz hi.xyz) per workgroup and the result behind them
#define RT_GEOM_BOX_BLOCKS 1024
#define RT_GEOM_BOX_FLOATS (6 * (RT_GEOM_BOX_BLOCKS + 1))

// Triangles [first, first + count) from d_src (count records of rt_triangle
// layout: vertex[3], normal[3], 18 floats): floats 0..8 of the prim-order
// records (v0, e1, e2; floats 9..11 stay), the normalised normal rows (9
// floats per prim) and the vertex boxes (6 floats per prim, lo.xyz hi.xyz).
// The caller has checked first + count against the buffers.  Asynchronous.
extern "C" hipError_t rt_geom_flatten(const float* d_src, uint32_t first, uint32_t count, float4* rec,
                                      float* nrm, float* pbox, hipStream_t s);

// The exact min / max over the nprim (> 0) vertex boxes into
// d_box[6 * RT_GEOM_BOX_BLOCKS ..] (lo.xyz hi.xyz); d_box holds
// RT_GEOM_BOX_FLOATS floats.  Asynchronous.
extern "C" hipError_t rt_geom_scene_box(const float* pbox, uint32_t nprim, float* d_box, hipStream_t s);

// The zero-normal risk flag (record float 11) of the prims [p0, p1), which
// are all the triangles of the objects [o0, o1]: an object's records are
// flagged iff one of its normal rows can interpolate a zero normal
// (host/rt_zero_risk.h).  objflag: one word per object.  Asynchronous.
extern "C" hipError_t rt_geom_zero_risk(float4* rec, const float* nrm, uint32_t p0, uint32_t p1,
                                        uint32_t* objflag, uint32_t o0, uint32_t o1, hipStream_t s);
