// rt_overlap.h -- which stream a frame's candidate-list build goes to
// (cand_prepare, rt_lists.cpp).  Frame k+1's lists need the camera, the
// triangles, the list buffers frame k's trace kernel reads and the item
// clocks it writes -- nothing of frame k's shade, fixup, fold or assemble.  So
// a render whose caller streams frames builds its lists on the context's side
// stream, beside the previous frame's shade pass: the side stream waits for
// the event recorded right after that frame's trace launch (ev_lists_free),
// and the caller's stream waits for the build's end (ev_lists_done) before it
// zeroes the frame counters and launches the trace.  Fork and join both
// happen inside the one rt_hip_render call: when it returns, everything later
// on the caller's stream is ordered after the build.
//
// What a build writes while the previous frame may still run:
//   keys / vals / keys2 / cand, start, skip bounds, work order, the counter
//   block and its snapshot, the scans' temporaries, the partition counts
//     read by that frame's trace only (before ev_lists_free), with one
//     exception: fold_kernel reads the asynchronous build's overflow flag
//     (KParams::list_flag).  Every asynchronous build therefore copies the
//     flag into one of two words of its own, alternated per build, and the
//     frame's fold reads that word (flag_slot): build k+1 writes the other.
//   the pinned words behind ev_kept
//     ordered by that event on whichever stream the build ran.
// Readers between two renders (rt_hip_stats, the frame check, a relight, the
// G-buffer read, rt_hip_cand_tile_entries) run on the render's stream after
// its join, and the next build starts only in the next rt_hip_render.
//
// Plain C++ (no HIP): cand_prepare and the render make the launches and tell
// this what happened; tests/native/overlap_order.cpp drives it on the CPU.
#pragma once

struct ListOverlap {
  int enabled = 1;      // rt_hip_set_overlap_lists (A/B runs, tests)
  // ev_lists_free marks the end of the last kernel that reads the list
  // buffers: set by a render's trace launch, cleared by anything else that
  // builds, routes or consumes lists on a caller's stream
  int free_marked = 0;
  int in_flight = 0;    // a build is on the side stream and no caller's stream waits for it yet
  unsigned flag_next = 0;  // the word the next asynchronous build's flag goes to
  unsigned long long side_builds = 0;  // rt_hip_overlap_builds

  // The rank's own asynchronous build of a render, whose buffers all hold
  // already (`fits`: nothing is allocated or freed), goes to the side stream
  // once a trace has marked the buffers free.  A read-back build, the first
  // frame, a frame whose buffers must grow, consumed lists, the compatibility
  // mode and rt_hip_cand_verify stay on the caller's stream.
  bool side(bool from_render, bool async, bool compat, bool fits) const {
    return enabled && free_marked && from_render && async && !compat && fits;
  }
  // the word of this build's overflow flag (its frame's fold reads it)
  unsigned flag_slot() {
    const unsigned s = flag_next;
    flag_next ^= 1u;
    return s;
  }
  void forked() {
    in_flight = 1;
    side_builds++;
  }
  void joined() { in_flight = 0; }
  void trace_launched() { free_marked = 1; }  // ev_lists_free recorded behind it
  // lists built, routed or consumed outside a render's own build: the event
  // no longer marks their last reader
  void lists_touched() { free_marked = 0; }
  void set_enabled(bool on) {
    enabled = on ? 1 : 0;
    free_marked = 0;  // the next build runs on the caller's stream
  }
};
