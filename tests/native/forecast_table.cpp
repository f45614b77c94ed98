// forecast_table.cpp -- the list-size forecast (csrc/rt_forecast.h) driven
// through scripted frame sequences on the CPU, every decision checked against
// a table (tests/test_host.py::test_list_forecast_table builds it with
// g++ -fsanitize=address,undefined; no GPU, no HIP).
//
// The expected values were derived by reading cand_prepare as it stood
// before the forecast was moved out of it (rt_lists.cpp at 76f7450, lines
// 639-810; "L650" below is a line of that file), not by running this code.
// Its decisions, in the order step() below makes them:
//   L650-668  the counters' snapshot, if pending and arrived: ctr[7] set ->
//             known, kept_for invalid, kept_pending = 0; else if known.valid
//             -> known = kept_pend's frame with ctr's sizes; snap_pending = 0
//   L678-687  exact = known.same(f); est = !exact && known.same_grid(f);
//             async = async_lists && !store_fp && !compat && (exact || est);
//             est sizes: total + total/4 + 4096, the other three + 1/4 + 64
//   L688-696  a read-back build writes its sizes into known, then known.set(f)
//             (!compat) or known.valid = 0 (compat)
//   L701-706  the kept count, if pending and arrived: kept, kept_for =
//             kept_pend, kept_ready = 1, kept_pending = 0
//   L715-719  compact_known = async && refine && kept_ready && (kept_for.same
//             || kept_for.same_grid) && kept <= total && total > 0;
//             compact_fresh = !async && !compat && !store_fp && refine && total > 0
//   L739-743  cap = total; known: kept_same ? kept : kept + kept/16 + 4096,
//             clipped to total
//   L752-762  fresh: the kept count read synchronously -> kept, kept_ready,
//             kept_for.set(f), kept_now
//   L778-793  request if refine && !compat && !kept_now && (!kept_same || est)
//             && !(kept_pending && kept_pend.same(f)); with the snapshot iff
//             est; then kept_pend.set(f), kept_pending = 1, snap_pending = est
#include <cstdio>
#include <cstring>

#include "rt_forecast.h"

enum Mode { READBACK, EXACT, ESTIMATED };
enum Compact { NONE, KNOWN, FRESH };
enum Request { NO_REQUEST, KEPT_ONLY, KEPT_AND_SNAPSHOT };

static rt_frame frame(int w, int h, float px) {
  rt_frame f;
  std::memset(&f, 0, sizeof f);  // compared bytewise: no stray padding
  f.u.x = 1.0f;
  f.v.y = 1.0f;
  f.C.z = 50.0f;
  f.position.x = px;
  f.width = w;
  f.height = h;
  return f;
}

// one frame as cand_prepare sees it
struct Step {
  const char* what;
  const rt_frame* f;
  int rank, nranks;
  bool async_lists, store_fp, refine, compat;
  bool arrived;           // hipEventQuery(ev_kept) == hipSuccess
  uint32_t h_kept[9];     // what the late read-back has written: [0] kept, [1..8] ctr[0..7]
  ListShape built;        // the sizes a read-back build finds
  uint32_t kept_sync;     // the kept count a fresh compaction reads back
  // expected
  Mode mode;
  uint32_t total, nglobal, nbig, nitems;  // the shape to size by (EXACT / ESTIMATED)
  Compact compact;
  uint32_t cap;
  Request request;
};

static ListShape sizes(uint32_t total, uint32_t nglobal, uint32_t nbig, uint32_t nitems) {
  ListShape s;
  s.total = total, s.nglobal = nglobal, s.nbig = nbig, s.nitems = nitems, s.over = 0;
  return s;
}

static int failures = 0;
#define EXPECT(cond, ...)                                     \
  do {                                                        \
    if (!(cond)) {                                            \
      std::fprintf(stderr, "%s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                      \
      std::fprintf(stderr, "\n");                             \
      failures++;                                             \
    }                                                         \
  } while (0)

// cand_prepare's use of the forecast (poll, plan, build, poll, compact,
// request), with the device's part scripted
static void step(ListForecast& fc, const Step& st) {
  if (fc.snap_pending && st.arrived) fc.absorb_snapshot(st.h_kept + 1);
  const ListPlan plan = fc.plan(st.f, st.rank, st.nranks, st.async_lists, st.store_fp, st.compat);
  const Mode mode = !plan.async ? READBACK : plan.estimated ? ESTIMATED : EXACT;
  EXPECT(mode == st.mode, "%s: mode %d, expected %d", st.what, mode, st.mode);
  uint32_t total = st.built.total;
  if (plan.async) {
    total = plan.shape.total;
    EXPECT(plan.shape.total == st.total && plan.shape.nglobal == st.nglobal && plan.shape.nbig == st.nbig &&
               plan.shape.nitems == st.nitems,
           "%s: shape %u %u %u %u", st.what, plan.shape.total, plan.shape.nglobal, plan.shape.nbig, plan.shape.nitems);
  } else {
    fc.record_build(st.built, st.f, st.rank, st.nranks, st.compat);
  }
  if (fc.kept_pending && st.arrived) fc.absorb_kept(st.h_kept[0]);
  const ListCompaction k = fc.compaction(plan, st.f, st.rank, st.nranks, total, st.refine, st.store_fp, st.compat);
  const Compact compact = k.known ? KNOWN : k.fresh ? FRESH : NONE;
  EXPECT(!(k.known && k.fresh), "%s: both compactions", st.what);
  EXPECT(compact == st.compact, "%s: compaction %d, expected %d", st.what, compact, st.compact);
  if (compact != NONE) EXPECT(k.cap == st.cap, "%s: cap %u, expected %u", st.what, k.cap, st.cap);
  bool kept_now = false;
  if (k.fresh) {
    fc.record_kept(st.kept_sync, st.f, st.rank, st.nranks);
    kept_now = true;
  }
  Request req = NO_REQUEST;
  if (fc.wants_late_readback(plan, st.f, st.rank, st.nranks, st.refine, st.compat, kept_now)) {
    fc.late_readback_requested(plan, st.f, st.rank, st.nranks);
    req = plan.estimated ? KEPT_AND_SNAPSHOT : KEPT_ONLY;
  }
  EXPECT(req == st.request, "%s: request %d, expected %d", st.what, req, st.request);
}

int main() {
  const rt_frame A = frame(480, 270, 0.0f), B = frame(480, 270, 1.5f), C = frame(64, 36, 0.0f);
  const ListShape szA = sizes(100000, 40, 500, 2000), szB = sizes(104000, 44, 520, 2100), szC = sizes(900, 3, 7, 20);
  const uint32_t keptA = 45000, keptB = 47000;
  // B's late read-back as it lands in h_kept: its kept count, its counters
  // ([1] globals, [2] big, [4] items, [5] over, [6] entries, [7] outgrown)
#define H_B(over) {keptB, 0, 44, 520, 0, 2100, 0, 104000, over}
#define H_NONE {0, 0, 0, 0, 0, 0, 0, 0, 0}
  const ListShape none = sizes(0, 0, 0, 0);
  // the usual modes: async_lists, !store_fp, refine, !compat
#define ON true, false, true, false

  {  // ---- the main sequence: A, A, B, (B's snapshot arrives) A, (flag set) B
    ListForecast fc;
    const Step s[] = {
        // L678: known invalid -> neither exact nor est -> read-back; L719: fresh, cap = the total (L739);
        // L778: kept_now -> no request
        {"first A", &A, 0, 1, ON, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH, 100000, NO_REQUEST},
        // L678: known.same(A) -> exact, known's sizes as they are; L716: kept_same -> known, L741: cap = kept;
        // L778: kept_same && !est -> no request
        {"A again", &A, 0, 1, ON, false, H_NONE, none, 0, EXACT, 100000, 40, 500, 2000, KNOWN, 45000, NO_REQUEST},
        // L679: same_grid -> est; L683-686: 100000 + 25000 + 4096, 40 + 10 + 64, 500 + 125 + 64, 2000 + 500 + 64;
        // L717: kept_for (A) same grid, 45000 <= 129096 -> known; L741: 45000 + 2812 + 4096 (< total: not clipped);
        // L778: !kept_same, nothing pending -> request, L786: with the snapshot (est)
        {"B, same size and split", &B, 0, 1, ON, false, H_NONE, none, 0, ESTIMATED, 129096, 114, 689, 2564, KNOWN,
         51908, KEPT_AND_SNAPSHOT},
        // L650: arrived, L655: flag clear, known valid -> known = B with B's counters; so (L678) A is not exact but
        // (L679) est from B's: 104000 + 26000 + 4096, 44 + 11 + 64, 520 + 130 + 64, 2100 + 525 + 64 (the 42b85d1 case);
        // L701: kept = 47000 for B; L717: same grid -> known, L741: 47000 + 2937 + 4096; L778: !kept_same, the
        // pending one has landed -> request with the snapshot
        {"A after B's snapshot", &A, 0, 1, ON, true, H_B(0), none, 0, ESTIMATED, 134096, 119, 714, 2689, KNOWN, 54033,
         KEPT_AND_SNAPSHOT},
        // L650: arrived, L652: flag set -> known and kept_for invalid, kept_pending = 0; L678: read-back;
        // L701: nothing pending; L719: fresh; L778: kept_now -> no request
        {"B after an outgrown estimate", &B, 0, 1, ON, true, H_B(1), szB, keptB, READBACK, 0, 0, 0, 0, FRESH, 104000,
         NO_REQUEST},
    };
    for (int i = 0; i < 3; i++) step(fc, s[i]);
    EXPECT(fc.snap_pending && fc.kept_pending && fc.kept_pend.same(&B, 0, 1), "B's request not recorded");
    step(fc, s[3]);
    EXPECT(fc.known.same(&B, 0, 1) && fc.known.total == 104000 && fc.known.nglobal == 44 && fc.known.nbig == 520 &&
               fc.known.nitems == 2100 && fc.known.over == 0,
           "known is not B with B's counters");
    EXPECT(fc.kept == keptB && fc.kept_for.same(&B, 0, 1), "kept is not B's");
    step(fc, s[4]);
    EXPECT(fc.known.same(&B, 0, 1) && fc.known.total == 104000 && fc.kept == keptB && fc.kept_for.same(&B, 0, 1) &&
               !fc.kept_pending && !fc.snap_pending,
           "after the read-back of B");
  }
  {  // ---- the snapshot has not arrived when A returns; B asked twice
    ListForecast fc;
    const Step s[] = {
        {"first A", &A, 0, 1, ON, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH, 100000, NO_REQUEST},
        {"B", &B, 0, 1, ON, false, H_NONE, none, 0, ESTIMATED, 129096, 114, 689, 2564, KNOWN, 51908, KEPT_AND_SNAPSHOT},
        // L650 / L701: not arrived -> nothing absorbed; L678: known is still A's own read-back -> exact;
        // L741: kept_for is A -> cap = kept; L778: kept_same && !est -> no request, B's stays pending
        {"A before B's snapshot", &A, 0, 1, ON, false, H_B(0), none, 0, EXACT, 100000, 40, 500, 2000, KNOWN, 45000,
         NO_REQUEST},
        // L679: est from A's sizes again; L778: !kept_same but L779: kept_pend is B and pending -> no second request
        {"B again, still pending", &B, 0, 1, ON, false, H_B(0), none, 0, ESTIMATED, 129096, 114, 689, 2564, KNOWN, 51908,
         NO_REQUEST},
    };
    for (const Step& st : s) {
      step(fc, st);
      if (&st != &s[0])
        EXPECT(fc.kept_pending && fc.snap_pending && fc.kept_pend.same(&B, 0, 1) && fc.known.same(&A, 0, 1) &&
                   fc.kept == keptA,
               "%s: the pending request was touched", st.what);
    }
  }
  {  // ---- another size, another rank split: L679 same_grid fails -> read-back
    ListForecast fc;
    const Step s[] = {
        {"first A", &A, 0, 1, ON, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH, 100000, NO_REQUEST},
        {"C, another size", &C, 0, 1, ON, false, H_NONE, szC, 400, READBACK, 0, 0, 0, 0, FRESH, 900, NO_REQUEST},
        // (L693: known is C now)
        {"A as rank 1 of 4", &A, 1, 4, ON, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH, 100000, NO_REQUEST},
        {"A as rank 0 of 4", &A, 0, 4, ON, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH, 100000, NO_REQUEST},
        {"A as rank 0 of 4 again", &A, 0, 4, ON, false, H_NONE, none, 0, EXACT, 100000, 40, 500, 2000, KNOWN, 45000,
         NO_REQUEST},
    };
    for (const Step& st : s) step(fc, st);
  }
  {  // ---- reset() (a setting that changes the lists) with a request in flight
    ListForecast fc;
    const Step s[] = {
        {"first A", &A, 0, 1, ON, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH, 100000, NO_REQUEST},
        {"B", &B, 0, 1, ON, false, H_NONE, none, 0, ESTIMATED, 129096, 114, 689, 2564, KNOWN, 51908, KEPT_AND_SNAPSHOT},
        // lists_changed: known, kept_for invalid, both pending flags 0 -> L650 / L701 do not look at the arrival;
        // L678: read-back; the sizes are the build's own (szC here: the setting changed the lists), not h_kept's
        {"A after reset", &A, 0, 1, ON, true, H_B(0), szC, 400, READBACK, 0, 0, 0, 0, FRESH, 900, NO_REQUEST},
    };
    step(fc, s[0]);
    step(fc, s[1]);
    fc.reset();
    step(fc, s[2]);
    EXPECT(fc.known.same(&A, 0, 1) && fc.known.total == 900 && fc.kept == 400 && fc.kept_for.same(&A, 0, 1),
           "the arrival after reset() was not ignored");
  }
  {  // ---- the modes: each of compat, store_fp, async_lists = 0 forces a read-back (L680)
    ListForecast fc;
    const Step s[] = {
        {"first A", &A, 0, 1, ON, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH, 100000, NO_REQUEST},
        // store_fp (cand_verify's rebuild): L680 read-back, L693 known = A again; L719 no fresh compaction
        // (store_fp), L716 none known (!async); L778: kept_same && !est -> no request
        {"A, every footprint kept", &A, 0, 1, true, true, true, false, false, H_NONE, szA, 0, READBACK, 0, 0, 0, 0, NONE, 0,
         NO_REQUEST},
        {"A, still exact", &A, 0, 1, ON, false, H_NONE, none, 0, EXACT, 100000, 40, 500, 2000, KNOWN, 45000, NO_REQUEST},
        // async_lists = 0: L680 read-back; L719 fresh; kept_now -> no request
        {"A, async_lists off", &A, 0, 1, false, false, true, false, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH,
         100000, NO_REQUEST},
        // refinement off: L680 still exact; L716 / L719 no compaction; L778 no request
        {"A, refinement off", &A, 0, 1, true, false, false, false, false, H_NONE, none, 0, EXACT, 100000, 40, 500, 2000,
         NONE, 0, NO_REQUEST},
        // compat: L680 read-back, L695 known.valid = 0; L719 no compaction (compat); L778 no request (compat)
        {"A, compatibility mode", &A, 0, 1, true, false, true, true, false, H_NONE, szA, 0, READBACK, 0, 0, 0, 0, NONE, 0,
         NO_REQUEST},
    };
    for (const Step& st : s) step(fc, st);
    EXPECT(!fc.known.valid, "compat left known valid");
    // L678: known invalid -> the next build of A reads back
    const Step after = {"A after compat", &A, 0, 1, ON, false, H_NONE, szA, keptA, READBACK, 0, 0, 0, 0, FRESH, 100000,
                        NO_REQUEST};
    step(fc, after);
  }
  {  // ---- the compaction's cap clipped to the total (L742): the kept count in hand is another camera's of the
     // grid and near A's exact total (state as L701-706 leave it when B's count lands during a build of A)
    ListForecast fc;
    fc.known = szA;
    fc.known.set(&A, 0, 1);
    fc.kept_for.set(&B, 0, 1);
    fc.kept = 98000;
    fc.kept_ready = 1;
    // 98000 + 6125 + 4096 > 100000 -> 100000; L778: !kept_same -> request, exact shape -> the kept count only
    const Step st = {"A, B's kept count", &A, 0, 1, ON, false, H_NONE, none, 0, EXACT, 100000, 40, 500, 2000, KNOWN,
                     100000, KEPT_ONLY};
    step(fc, st);
    // L718: a kept count past the total -> no compaction from it
    fc.kept = 100001;
    fc.kept_pending = 0;
    const Step st2 = {"A, a kept count past its total", &A, 0, 1, ON, false, H_NONE, none, 0, EXACT, 100000, 40, 500,
                      2000, NONE, 0, KEPT_ONLY};
    step(fc, st2);
  }
  // the size comparison rt_hip_cand_produce makes of a slice's counters (rt_lists.cpp at 76f7450, L915-916)
  {
    const uint32_t same[8] = {9, 40, 500, 9, 2000, 0, 100000, 0}, outgrown[8] = {9, 40, 500, 9, 2000, 0, 100000, 1};
    const uint32_t other[8] = {9, 40, 500, 9, 2001, 0, 100000, 0};
    EXPECT(szA.same_sizes(same) && !szA.same_sizes(outgrown) && !szA.same_sizes(other), "same_sizes");
  }
  if (failures) {
    std::fprintf(stderr, "%d forecast decisions differ from the table\n", failures);
    return 1;
  }
  std::printf("list forecast table ok\n");
  return 0;
}
