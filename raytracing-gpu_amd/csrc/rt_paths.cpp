// rt_paths.cpp -- host side of the path export (include/rt_hip.h
// rt_hip_path_records, rt_hip_path_records_host): the refusals, the three
// launches of csrc/rt_paths.hip over the kept batch's hit-record buffers (the
// views of c->last_p, which rt_hip_trace_rays left), and the host wrapper.
// The call reads the context's buffers only: which batch's paths they hold,
// and who takes them away, is rt_hip_ctx::paths (csrc/rt_ctx.h).  The blocks
// and the scratch words are csrc/rt_path_items.h.
#include "rt_batch.h"  // the refusals every batch words alike
#include "rt_path_items.h"

static_assert(RT_PATH_PRIM == (int)RT_PATH_PRIM_D, "rt_hip.h states the exported records' prim");
static_assert(sizeof(rt_gsample) == 5 * sizeof(uint2), "an exported record is five 8-byte stores");

// The refusals: nothing of the context has changed, nothing is written when
// one of them returns.  (offsets, records: device pointers, or the host wrapper's)
static int paths_refuse(const rt_hip_ctx* c, size_t n, const unsigned* offsets, const void* records) {
  if (int rc = batch_refuse_ctx(c)) return rc;
  if (!c->paths.valid) {
    if (!c->paths.taken_by)
      return rt_set_error(RT_EINVAL, "no ray batch with colours traced yet: no paths to export");
    return rt_set_error(RT_EINVAL, "the last ray batch's paths are gone: %s took the hit records", c->paths.taken_by);
  }
  if (n != c->paths.n) return rt_set_error(RT_EINVAL, "%zu rays asked, the kept batch traced %zu", n, c->paths.n);
  if (!offsets) return rt_set_error(RT_EINVAL, "null path offsets");
  if ((uintptr_t)records & 7) return rt_set_error(RT_EINVAL, "path records must be 8-byte aligned");
  return RT_OK;
}

extern "C" int rt_hip_path_records(rt_hip_ctx* c, size_t n, unsigned* d_offsets, size_t cap, void* d_records,
                                   float* d_coef, float* d_terms, void* stream) {
  int rc = paths_refuse(c, n, d_offsets, d_records);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (s != c->paths.stream)
    return rt_set_error(RT_EINVAL, "the path export runs on the stream of the batch it exports");
  HIP_TRY(hipSetDevice(c->device));
  const KParams& lp = c->last_p;
  PathArgs a;
  std::memset(&a, 0, sizeof a);
  a.hit = lp.hit;
  a.hit_prev = lp.hit_prev;
  a.hit_term = lp.hit_term;
  a.last = lp.last;
  a.hit_cap = lp.hit_cap;
  a.n = n;
  a.nblocks = rt_path_blocks(n);
  a.cap = cap;
  a.offsets = d_offsets;
  a.records = (uint2*)d_records;
  a.coef = d_coef;
  a.terms = d_terms;
  // every device pointer the kernels will follow must exist and be the
  // buffer the batch wrote, whole (a null or stale one would fault the card,
  // not fail the call)
  if (n == 0 || n > RT_RAYS_MAX || !a.hit || a.hit != c->d_hit.get() || a.hit_prev != c->d_hit_prev.get() ||
      a.hit_term != c->d_hit_term.get() || a.last != c->d_last.get() || !c->d_last.holds(n) ||
      (size_t)a.hit_cap != c->hit_cap() || a.hit_cap == 0)
    return rt_set_error(RT_EHIP, "path export: the kept batch's hit buffers are missing");
  const size_t words = rt_path_scratch_words(n);
  HIP_TRY(c->d_path_tot.grow(words, words));
  a.btot = c->d_path_tot;
  if (!a.btot || a.nblocks == 0) return rt_set_error(RT_EHIP, "path export: scratch missing");
  HIP_TRY(rt_launch_path_lengths(&a, s));
  HIP_TRY(rt_launch_path_totals(&a, s));
  HIP_TRY(rt_launch_path_write(&a, s));
  return RT_OK;
}

extern "C" int rt_hip_path_records_host(rt_hip_ctx* c, size_t n, unsigned* h_offsets, size_t cap,
                                        rt_gsample* h_records, float* h_coef, float* h_terms) {
  int rc = paths_refuse(c, n, h_offsets, h_records);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const bool any = h_records || h_coef || h_terms;
  if (!any) cap = 0;
  DevBuf<uint32_t> d_off;
  DevBuf<rt_gsample> d_rec;
  DevBuf<float> d_coef, d_terms;
  if (d_off.alloc(n + 1) != hipSuccess || (h_records && d_rec.alloc(cap) != hipSuccess) ||
      (h_coef && d_coef.alloc(cap) != hipSuccess) || (h_terms && d_terms.alloc(3 * cap) != hipSuccess))
    return rt_set_error(RT_EHIP, "hipMalloc path records");
  // on the batch's stream, as the device call asks
  hipStream_t s = c->paths.stream;
  rc = rt_hip_path_records(c, n, d_off.get(), cap, h_records ? (void*)d_rec.get() : nullptr,
                           h_coef ? d_coef.get() : nullptr, h_terms ? d_terms.get() : nullptr, s);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(h_offsets, d_off, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const size_t have = std::min<size_t>(h_offsets[n], cap);  // the vertices written
  if (have) {
    if (h_records) HIP_TRY(hipMemcpyAsync(h_records, d_rec, have * sizeof(rt_gsample), hipMemcpyDeviceToHost, s));
    if (h_coef) HIP_TRY(hipMemcpyAsync(h_coef, d_coef, have * sizeof(float), hipMemcpyDeviceToHost, s));
    if (h_terms) HIP_TRY(hipMemcpyAsync(h_terms, d_terms, 3 * have * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));  // the buffers above go
  return RT_OK;
}
