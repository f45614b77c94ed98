// overlap_order.cpp -- the rule that sends a frame's candidate-list build to
// the context's side stream (csrc/rt_overlap.h ListOverlap), driven on the CPU
// the way cand_prepare and the render drive it.  Every sequence of up to six
// calls -- a render whose build may overlap, a render whose build reads its
// sizes back (the first frame of a size, buffers that grow), a reader between
// two renders, lists built outside a render (produce / consume, the
// compatibility mode, cand_verify), the switch, a setting that changes the
// lists, each optionally followed by the destroy -- is turned into the
// launches it makes on the caller's stream and the side stream with their
// event edges, and the order is checked:
//   * a build writes the list buffers only after every earlier trace (their
//     reader) and every earlier build has ended;
//   * a frame's fold reads its build's overflow flag from a place that no
//     other build writes before the fold has ended, and that its own build
//     has written before it starts;
//   * between two calls, and at the destroy, no build is in flight on the
//     side stream; the builds counted are the ones that went there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_overlap.h"

enum Op { RENDER, RENDER_READBACK, READER, OUTSIDE, SWITCH, CHANGED, NOPS };
static const char* const kOpName[NOPS] = {"render", "render-readback", "reader", "outside", "switch", "changed"};

enum Place { NONE = -1, WORD0 = 0, WORD1 = 1, SNAPSHOT = 2 };

struct Node {
  uint64_t before = 0;   // the nodes that have ended when this one starts
  bool writes_lists = false, reads_lists = false;
  bool writes[3] = {false, false, false};  // the two flag words, the counters' snapshot
  Place reads = NONE;
  bool build = false;
};

struct Model {
  std::vector<Node> n;
  int main_last = -1, side_last = -1;  // the last launch on each stream
  int ev_free = -1, flag_of_last = NONE;
  ListOverlap ov;
  unsigned long long side_expected = 0;

  int launch(bool side, int extra_dep) {
    Node x;
    int& last = side ? side_last : main_last;
    for (int d : {last, extra_dep})
      if (d >= 0) x.before |= n[(size_t)d].before | (1ull << d);
    n.push_back(x);
    last = (int)n.size() - 1;
    return last;
  }
  void join_main(int dep) {  // hipStreamWaitEvent on the caller's stream: a marker node
    launch(false, dep);
  }

  void build(bool from_render, bool async) {
    const bool side = ov.side(from_render, async, false, true);
    if (side) {
      ov.forked();
      side_expected++;
    } else if (!from_render) {
      ov.lists_touched();
    }
    const int b = launch(side, side ? ev_free : -1);
    n[(size_t)b].writes_lists = n[(size_t)b].build = true;
    flag_of_last = NONE;
    if (async) {
      n[(size_t)b].writes[SNAPSHOT] = true;  // bounds_kernel's copy of the counters
      flag_of_last = SNAPSHOT;
      if (ov.enabled) {
        const unsigned w = ov.flag_slot();
        n[(size_t)b].writes[w] = true;
        flag_of_last = (Place)w;
      }
    }
    if (side) {
      join_main(b);
      ov.joined();
    }
  }

  void render(bool async) {
    build(true, async);
    const int t = launch(false, -1);  // the trace
    n[(size_t)t].reads_lists = true;
    if (ov.enabled) {
      ev_free = t;
      ov.trace_launched();
    } else {
      ov.lists_touched();
    }
    const int f = launch(false, -1);  // shade, fixup, fold
    n[(size_t)f].reads = (Place)flag_of_last;
  }

  void apply(Op op) {
    switch (op) {
      case RENDER: render(true); break;
      case RENDER_READBACK: render(false); break;
      case READER: launch(false, -1); break;
      case OUTSIDE: build(false, false); { const int t = launch(false, -1); n[(size_t)t].reads_lists = true; } break;
      case SWITCH: ov.set_enabled(!ov.enabled); break;
      case CHANGED: ov.joined(); break;  // (lists_changed waits for the side stream first when in_flight)
      default: break;
    }
  }
};

static int fail(const std::vector<Op>& seq, const char* what, int a, int b) {
  std::fprintf(stderr, "FAIL %s (nodes %d, %d) after:", what, a, b);
  for (Op o : seq) std::fprintf(stderr, " %s", kOpName[o]);
  std::fprintf(stderr, "\n");
  return 1;
}

static int check(const Model& m, const std::vector<Op>& seq) {
  const int N = (int)m.n.size();
  if (N > 63) return fail(seq, "too many nodes", N, 0);
  for (int j = 0; j < N; j++) {
    const Node& w = m.n[(size_t)j];
    for (int i = 0; i < j; i++) {
      const Node& e = m.n[(size_t)i];
      const bool ordered = (w.before >> i) & 1;
      if (w.writes_lists && (e.reads_lists || e.writes_lists) && !ordered) return fail(seq, "lists written early", i, j);
      if (e.reads != NONE && w.writes[e.reads] && !ordered) return fail(seq, "flag overwritten under its fold", i, j);
      if (w.reads != NONE && e.writes[w.reads] && !ordered) return fail(seq, "flag read before it was written", i, j);
    }
    if (w.reads != NONE) {  // the word's last writer is the frame's own build
      int last = -1, own = -1;
      for (int i = 0; i < j; i++) {
        if (m.n[(size_t)i].writes[w.reads]) last = i;
        if (m.n[(size_t)i].build) own = i;
      }
      if (last != own) return fail(seq, "flag is another build's", last, j);
    }
  }
  if (m.ov.in_flight) return fail(seq, "a build in flight between two calls", 0, 0);
  if (m.ov.side_builds != m.side_expected) return fail(seq, "side builds miscounted", 0, 0);
  return 0;
}

int main() {
  unsigned long long cases = 0, side = 0;
  std::vector<Op> seq;
  for (int len = 1; len <= 6; len++) {
    std::vector<int> ix((size_t)len, 0);
    for (;;) {
      seq.clear();
      Model m;
      for (int k = 0; k < len; k++) {
        seq.push_back((Op)ix[(size_t)k]);
        m.apply(seq.back());
        if (check(m, seq)) return 1;  // (every prefix may be followed by the destroy)
      }
      cases++;
      side += m.ov.side_builds;
      int k = len - 1;
      while (k >= 0 && ++ix[(size_t)k] == NOPS) ix[(size_t)k--] = 0;
      if (k < 0) break;
    }
  }
  {  // the plain stream of frames: every build after the first frame's goes to the side stream
    Model m;
    m.render(false);
    for (int k = 0; k < 5; k++) m.render(true);
    if (m.ov.side_builds != 5) return fail({}, "a stream of frames: side builds", (int)m.ov.side_builds, 5);
    Model off;
    off.ov.set_enabled(false);
    off.render(false);
    for (int k = 0; k < 5; k++) off.render(true);
    if (off.ov.side_builds != 0) return fail({}, "switched off: side builds", (int)off.ov.side_builds, 0);
  }
  if (!side) return fail({}, "no sequence overlapped", 0, 0);
  std::printf("overlap order ok (%llu sequences, %llu side builds)\n", cases, side);
  return 0;
}
