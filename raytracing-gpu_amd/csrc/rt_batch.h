// rt_batch.h -- what the batches that count into the batch stats block share
// on the host: occlusion batches (rt_occl.cpp), ambient occlusion (rt_ao.cpp)
// and direct light for records (rt_dlight.cpp).  To the context each of them
// is the same operation: it counts into d_occl_stats, sets last_occl, uses the
// stack spill area and the item counters in stream order, and leaves the kept
// frame, the lists, the overlap state and the render's counters as they are.
// The refusals they word alike, the launch sequence (batch_begin, the caller's
// argument block and own checks, batch_run) and what rt_hip_stats reads
// afterwards (occl_stats) are here, once; csrc/rt_batch.cpp.
#pragma once
#include "rt_ctx.h"

// The refusals: nothing of the context has changed when one of them returns.
// `things`: what the batch holds ("rays", "records"); `noun` with its article
// `a`: "an " "occlusion batch", "" "direct light".
int batch_refuse_ctx(const rt_hip_ctx* c);  // null or broken
int batch_refuse_size(size_t n, const char* things);
int batch_refuse_mode(const rt_hip_ctx* c, unsigned flags, const char* a, const char* noun);  // flags, policy, counting pass

// Batches over rt_gsample records with k rays each by ambient occlusion's rule
// (rt_ao.cpp, rt_gather.cpp): the sizes (k, m, n k, the item count), and the
// records and table in device memory.
int ao_refuse(const rt_hip_ctx* c, size_t n, unsigned k, unsigned m);                // rt_ao.cpp
int ao_refuse_ptrs(const void* d_samples, size_t n, const float* d_table);          // rt_ao.cpp

// A launch worked out by batch_begin: the caller copies `walk` into its
// argument block, checks the pointers only its kernel follows, and runs it.
struct BatchLaunch {
  hipStream_t s;
  int kind, dacc, grid;  // RT_BATCH_*, RT_ACCEL_*_D, one-wave workgroups
  bool octree;           // dacc == RT_ACCEL_OCTREE_D
  uint32_t walk;         // RT_RAYS_WALK_EXACT, RT_RAYS_WALK_PACKET or 0: the per-lane walk
  KParams p;
};
// For `nitems` > 0 work items of a batch of `kind` (flags: RT_RAYS_PACKET or
// 0): the device, the stream, FLAT or octree, the scene's parameters, the walk
// (with the exact walk's bounds built), the stats block, the kernel's grid and
// the pointers every kind's kernel follows (`noun` names the batch if one is
// missing).  lbuf: the kernel scans the light buffers -- built first, as a
// render builds them, and p.lbuf set.
int batch_begin(rt_hip_ctx* c, void* stream, unsigned flags, int kind, uint32_t nitems, bool lbuf, const char* noun,
                BatchLaunch* b);
// The item counters and the stats block zeroed, the kernel launched with
// `args` (the kind's block, rt_kernels.h), and the context told what
// rt_hip_stats reads next.
int batch_run(rt_hip_ctx* c, const BatchLaunch& b, const void* args);

// A _host wrapper's ends.  Nothing to do: nothing launched, nothing written.
static inline int batch_host_none(rt_stats* st) {
  if (st) std::memset(st, 0, sizeof *st);
  return RT_OK;
}
// After its last copy was queued with result rc: the stats (which synchronise),
// and the context's stream once more whatever happened: the wrapper's buffers go.
static inline int batch_host_end(rt_hip_ctx* c, int rc, rt_stats* st) {
  rt_stats tmp;
  if (!rc) rc = rt_hip_stats(c, st ? st : &tmp);
  (void)hipStreamSynchronize(c->stream);
  return rc;
}
