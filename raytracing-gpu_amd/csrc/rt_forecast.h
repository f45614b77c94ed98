// rt_forecast.h -- the list-size forecast of the per-rank candidate lists
// (cand_prepare, rt_lists.cpp): which builds run without a host wait, how
// many kept entries the compaction is sized for, and when a late read-back
// may overwrite what is known.  Plain C++ (no HIP): cand_prepare polls the
// events and makes the launches, and tells this what arrived;
// tests/native/forecast_table.cpp drives it on the CPU.
#pragma once
#include <cstdint>
#include <cstring>

#include "rt_counters.h"
#include "rt_hip.h"

// The sizes of one list build, which are deterministic for its (camera
// frame, rank, nranks): a later build of the same frame sizes its buffers and
// launches from them instead of reading its own back (async_lists).
struct ListShape {
  int valid = 0;
  rt_frame frame{};
  int rank = -1, nranks = 0;
  uint32_t total = 0, nglobal = 0;           // entries, global prims
  uint32_t nbig = 0, nitems = 0, over = 0;   // the big-emission launch shape
  bool same(const rt_frame* f, int r, int n) const {
    return valid && rank == r && nranks == n && std::memcmp(&frame, f, sizeof *f) == 0;
  }
  // the same image size and rank split (the same tiles), any camera
  bool same_grid(const rt_frame* f, int r, int n) const {
    return valid && rank == r && nranks == n && frame.width == f->width && frame.height == f->height;
  }
  void set(const rt_frame* f, int r, int n) {
    valid = 1;
    frame = *f;
    rank = r;
    nranks = n;
  }
  // a build's counters (rt_counters.h RtCandCtr); RT_CC_OVERFLOW: it outgrew the sizes it was given
  void set_sizes(const uint32_t ctr[RT_CC_BUILD_WORDS]) {
    total = ctr[RT_CC_TOTAL], nglobal = ctr[RT_CC_GLOBAL], nbig = ctr[RT_CC_BIG];
    nitems = ctr[RT_CC_ITEMS], over = ctr[RT_CC_ITEMS_OVER];
  }
  bool same_sizes(const uint32_t ctr[RT_CC_BUILD_WORDS]) const {
    return !ctr[RT_CC_OVERFLOW] && total == ctr[RT_CC_TOTAL] && nglobal == ctr[RT_CC_GLOBAL] &&
           nbig == ctr[RT_CC_BIG] && nitems == ctr[RT_CC_ITEMS] && over == ctr[RT_CC_ITEMS_OVER];
  }
};

// How one frame's lists are built.  Asynchronous (no host wait) for a frame
// whose lists were built before with a read-back -- its sizes are
// deterministic -- and, with headroom, for a new camera of the same size and
// rank split (an animation's next frame, a panned view): the last build's
// sizes + 1/4 size the buffers and launches, every kernel checks its counts
// on the device, and a frame past them is reported (RT_EHITBUF via ctr[RT_CC_OVERFLOW],
// rt_hip_stats / the frame check) and built again with a read-back.  The
// first frame of a size or split, the compatibility mode and cand_verify's
// rebuild (every footprint kept) read their sizes back.
struct ListPlan {
  bool async = false;      // built from `shape`; otherwise the build reads its sizes back
  bool estimated = false;  // the known frame is another camera of this grid: `shape` has headroom
  ListShape shape;
};

// The kept entries compacted before the sort (the refinement drops ~55 % of
// them on C5): an asynchronous build takes the kept count of the same
// frame's earlier build; a fresh frame (a new camera: the build read its
// total back anyway) reads its own back after the compaction's scan -- one
// more short host wait instead of sorting the dropped entries (sorting them
// all measured lists 1.96 vs 1.83 / 1.85 ms on C5, profiles/r08_compact/).
// For a new camera the last frame's kept count + 1/16: the scatter writes the
// unused tail as dropped, and a count past it sets ctr[RT_CC_OVERFLOW].
struct ListCompaction {
  bool known = false;  // to `cap` entries, from an earlier build's kept count
  bool fresh = false;  // to the build's total; the caller reads the kept count back (record_kept)
  uint32_t cap = 0;
  explicit operator bool() const { return known || fresh; }
};

struct ListForecast {
  // the frame (camera frame, rank, nranks) whose per-rank lists were last
  // built with a read-back, and their sizes: the same frame's lists are
  // deterministic, so they are rebuilt without reading the total back
  ListShape known;
  // the entries the refinement kept (start[ntiles]) in the last build of
  // kept_for's frame, read back without waiting: the same frame's
  // asynchronous builds compact the entries to that many before the sort
  // instead of sorting the dropped ones too
  ListShape kept_for;
  uint32_t kept = 0;
  int kept_ready = 0;    // kept holds kept_for's count
  ListShape kept_pend;   // the frame whose kept count is on its way (the late read-back)
  int kept_pending = 0;
  int snap_pending = 0;  // the late read-back also brings the last estimated-shape build's counters

  // A setting that changes the lists: no earlier build's sizes or kept count
  // apply any more (the read-backs on their way are discarded too)
  void reset() {
    known.valid = kept_for.valid = 0;
    kept_pending = snap_pending = 0;
  }

  // The last estimated-shape build's counters have arrived: the next
  // estimate starts from them
  void absorb_snapshot(const uint32_t ctr[RT_CC_BUILD_WORDS]) {
    if (!snap_pending) return;
    if (ctr[RT_CC_OVERFLOW]) {  // that frame outgrew its estimate (reported): the next build reads back
      known.valid = kept_for.valid = 0;
      kept_pending = 0;
    } else if (known.valid) {
      // the counters are those of the frame the snapshot was taken for
      // (kept_pend: set with snap_pending), not of the read-back frame known
      // still names: that one rendered again must not match them as its own
      // exact shape -- it is one more new camera, sized with headroom
      known.set(&kept_pend.frame, kept_pend.rank, kept_pend.nranks);
      known.set_sizes(ctr);
    }
    snap_pending = 0;
  }

  // The kept count of the last build of this size and split has arrived
  void absorb_kept(uint32_t count) {
    if (!kept_pending) return;
    kept = count;
    kept_for = kept_pend;
    kept_ready = 1;
    kept_pending = 0;
  }

  ListPlan plan(const rt_frame* f, int rank, int nranks, bool async_lists, bool store_fp, bool compat) const {
    ListPlan p;
    const bool exact = known.same(f, rank, nranks);
    p.estimated = !exact && known.same_grid(f, rank, nranks);
    p.async = async_lists && !store_fp && !compat && (exact || p.estimated);
    p.shape = known;
    if (p.estimated) {
      p.shape.total = known.total + known.total / 4 + 4096;
      p.shape.nglobal = known.nglobal + known.nglobal / 4 + 64;
      p.shape.nbig = known.nbig + known.nbig / 4 + 64;
      p.shape.nitems = known.nitems + known.nitems / 4 + 64;
    }
    return p;
  }

  // A read-back build's sizes size this frame's later builds (never the compatibility mode's)
  void record_build(const ListShape& sizes, const rt_frame* f, int rank, int nranks, bool compat) {
    known = sizes;
    known.valid = 0;
    if (!compat) known.set(f, rank, nranks);
  }

  // `total`: the entries the build emitted (a read-back build's own count, an
  // asynchronous build's plan.shape.total)
  ListCompaction compaction(const ListPlan& p, const rt_frame* f, int rank, int nranks, uint32_t total,
                            bool refine, bool store_fp, bool compat) const {
    ListCompaction k;
    const bool kept_same = kept_for.same(f, rank, nranks);
    k.known = p.async && refine && kept_ready && (kept_same || kept_for.same_grid(f, rank, nranks)) &&
              kept <= total && total > 0;
    k.fresh = !p.async && !compat && !store_fp && refine && total > 0;
    // (fewer kept than last time -- never expected -- leave a tail the scatter writes as dropped)
    k.cap = total;
    if (k.known) {
      k.cap = kept_same ? kept : kept + kept / 16 + 4096;
      if (k.cap > total) k.cap = total;
    }
    return k;
  }

  // A fresh frame's kept count, read back synchronously after its compaction
  void record_kept(uint32_t count, const rt_frame* f, int rank, int nranks) {
    kept = count;
    kept_ready = 1;
    kept_for.set(f, rank, nranks);
  }

  // Whether to ask for this frame's kept count -- and after an estimated-shape build its counters --
  // for the later builds, read back without waiting (kept_now: record_kept has just taken it)
  bool wants_late_readback(const ListPlan& p, const rt_frame* f, int rank, int nranks, bool refine, bool compat,
                           bool kept_now) const {
    return refine && !compat && !kept_now && (!kept_for.same(f, rank, nranks) || p.estimated) &&
           !(kept_pending && kept_pend.same(f, rank, nranks));
  }
  // (the count in hand, if any, stays usable -- for this size and split --
  // until this one arrives: the host runs frames ahead of the device)
  void late_readback_requested(const ListPlan& p, const rt_frame* f, int rank, int nranks) {
    kept_pend.set(f, rank, nranks);
    kept_pending = 1;
    snap_pending = p.estimated ? 1 : 0;
  }
};
