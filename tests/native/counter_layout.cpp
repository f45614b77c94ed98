// counter_layout.cpp -- the numbers behind the names of csrc/rt_counters.h,
// pinned on the CPU (tests/test_counter_layout.py builds it plain and with
// g++ -fsanitize=address,undefined; no GPU, no HIP).
//
// The tables below are literal.  They were copied by reading the last commit
// that spelled the words by number (985109c): rt_hip_stats' 23 `out->x = h[n]`
// lines, shade_stat_slot's set, fold_kernel's frame check, the comment at
// CandParams::ctr with d_cand_ctr's `+ 8` / `+ 16` / 32, and rt_lightbuf_build's
// hc[0..4] (csrc/rt_lightbuf.hip; the emission's overflow flag is set in
// csrc/rt_lightbuf_geom.h row_entries).  The kernels' assembly says the device
// side kept its numbers; this says the names mean what the numbers meant.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "rt_counters.h"

static int failures = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
      failures++;                                        \
    }                                                    \
  } while (0)

#define MEMBER(m) #m, offsetof(rt_stats, m)
struct StatRow {
  uint32_t slot, named;  // the number then, the name's value now
  const char* member;
  size_t offset;         // of the rt_stats member the slot filled
  bool shade;            // in shade_stat_slot's set {1, 10, 11, 15, 16, 18..21}
  uint32_t flag;         // the bit fold_kernel raised on a non-zero count
};
static const StatRow kStats[] = {
    {0, RT_ST_CLOSEST, MEMBER(closest), false, 0},
    {1, RT_ST_SHADOW, MEMBER(shadow), true, 0},
    {2, RT_ST_PIXELS, MEMBER(pixels), false, 0},
    {3, RT_ST_NODE_VISITS, MEMBER(node_visits), false, 0},
    {4, RT_ST_TRI_TESTS, MEMBER(tri_tests), false, 0},
    {5, RT_ST_DEPTH_OVERFLOW, MEMBER(depth_overflow), false, 2},
    {6, RT_ST_ZERO_NORMAL, MEMBER(zero_normal), false, 4},
    {7, RT_ST_HITS, MEMBER(hits), false, 0},
    {8, RT_ST_CLOSEST_NODE_LANES, MEMBER(closest_node_lanes), false, 0},
    {9, RT_ST_CLOSEST_TRI_LANES, MEMBER(closest_tri_lanes), false, 0},
    {10, RT_ST_SHADOW_NODE_LANES, MEMBER(shadow_node_lanes), true, 0},
    {11, RT_ST_SHADOW_TRI_LANES, MEMBER(shadow_tri_lanes), true, 0},
    {12, RT_ST_CYCLES_CAMERA, MEMBER(cycles_camera), false, 0},
    {13, RT_ST_CYCLES_CAND, MEMBER(cycles_cand), false, 0},
    {14, RT_ST_CYCLES_SECONDARY, MEMBER(cycles_secondary), false, 0},
    {15, RT_ST_CYCLES_SHADOW, MEMBER(cycles_shadow), true, 0},
    {16, RT_ST_CYCLES_SHADOW_DIRECTIONAL, MEMBER(cycles_shadow_directional), true, 0},
    {17, RT_ST_STACK_SPILLS, MEMBER(stack_spills), false, 0},
    {18, RT_ST_SHADOW_ZERO_RISK, MEMBER(shadow_zero_risk), true, 4},
    {19, RT_ST_SHADOW_NODE_VISITS, MEMBER(shadow_node_visits), true, 0},
    {20, RT_ST_SHADOW_TRI_TESTS, MEMBER(shadow_tri_tests), true, 0},
    {21, RT_ST_SHADOW_UNPROVEN, MEMBER(shadow_unproven), true, 8},
    {22, RT_ST_CLOSEST_UNPROVEN, MEMBER(closest_unproven), false, 8},
};
// the members rt_hip_stats derives instead (camera = 4 * pixels, the hit
// regions' counters, the context's list counts, the off-box queue's count)
static const struct {
  const char* member;
  size_t offset;
} kDerived[] = {{MEMBER(camera)},     {MEMBER(hit_records)}, {MEMBER(cand_prims)},
                {MEMBER(cand_entries)}, {MEMBER(cand_global)}, {MEMBER(shadow_deferred)}};

static size_t member_offset(uint32_t slot) {
  static const rt_stats st{};
  return (size_t)((const char*)&(st.*rt_stat_member[slot]) - (const char*)&st);
}

static void render_stats() {
  const size_t nmember = sizeof(rt_stats) / sizeof(unsigned long long);
  static_assert(sizeof(rt_stats) % sizeof(unsigned long long) == 0, "rt_stats is 64-bit words");
  CHECK(RT_NSTATS == 23 && sizeof kStats / sizeof *kStats == 23, "RT_NSTATS = %u", (unsigned)RT_NSTATS);
  CHECK(RT_STAT_SETS == 8 && RT_STAT_STRIDE == 32, "%d copies, %d apart", RT_STAT_SETS, RT_STAT_STRIDE);
  CHECK(RT_FRAME_HITBUF == 1 && RT_FRAME_DEPTH == 2 && RT_FRAME_ZERO == 4 && RT_FRAME_UNPROVEN == 8 &&
            RT_FRAME_LISTS == 16,
        "frame-check bits");
  int filled[64] = {};
  CHECK(nmember <= 64, "%zu members", nmember);
  for (const StatRow& r : kStats) {
    CHECK(r.named == r.slot, "%s: slot %u is now %u", r.member, r.slot, r.named);
    CHECK(member_offset(r.slot) == r.offset, "slot %u fills offset %zu, not %s at %zu", r.slot, member_offset(r.slot),
          r.member, r.offset);
    CHECK(rt_stat_shade_side(r.slot) == r.shade, "slot %u (%s): shade side %d", r.slot, r.member, (int)!r.shade);
    CHECK(rt_stat_frame_flag(r.slot) == r.flag, "slot %u (%s): flag %u, was %u", r.slot, r.member,
          rt_stat_frame_flag(r.slot), r.flag);
    filled[member_offset(r.slot) / sizeof(unsigned long long)]++;
  }
  for (uint32_t k = RT_NSTATS; k < 32; k++)  // the unused words of a copy belong to neither pass
    CHECK(!rt_stat_shade_side(k) && !rt_stat_frame_flag(k), "word %u past the slots", k);
  // no member twice, and the unfilled ones exactly the derived ones
  for (const auto& d : kDerived) {
    CHECK(filled[d.offset / sizeof(unsigned long long)] == 0, "%s is filled from a slot", d.member);
    filled[d.offset / sizeof(unsigned long long)] = -1;
  }
  for (size_t m = 0; m < nmember; m++)
    CHECK(filled[m] == 1 || filled[m] == -1, "rt_stats word %zu: filled %d times", m, filled[m]);
  CHECK(nmember == 23 + sizeof kDerived / sizeof *kDerived, "%zu members", nmember);
  // what rt_hip_stats' loop does, on distinct values
  rt_stats out;
  std::memset(&out, 0, sizeof out);
  for (uint32_t k = 0; k < RT_NSTATS; k++) out.*rt_stat_member[k] = 1000 + k;
  CHECK(out.closest == 1000 && out.shadow == 1001 && out.pixels == 1002 && out.hits == 1007 &&
            out.shadow_zero_risk == 1018 && out.shadow_unproven == 1021 && out.closest_unproven == 1022,
        "table loop");
  CHECK(out.camera == 0 && out.hit_records == 0 && out.shadow_deferred == 0, "derived members untouched");
}

static void cand_counters() {
  // rt_cand.h at 985109c: "[1] global prims, [2] big footprints, [3] list
  // length, [4] big emission items (item_kernel), [5] 1 = more than item_cap
  // items, [6] the entry total, [7] 1 = an entry past key_cap"; [0] zeroed only
  CHECK(RT_CC_RESERVED == 0 && RT_CC_GLOBAL == 1 && RT_CC_BIG == 2 && RT_CC_LIST == 3 && RT_CC_ITEMS == 4 &&
            RT_CC_ITEMS_OVER == 5 && RT_CC_TOTAL == 6 && RT_CC_OVERFLOW == 7,
        "build words");
  CHECK(RT_CC_BUILD_WORDS == 8 && RT_CAND_CTR_SAVED_VALID == 8 && RT_CAND_CTR_SNAPSHOT == 16 &&
            RT_CAND_CTR_BLOCK == 32,
        "block map");
  // h_kept: [0] kept, [1..8] the counters (9 words); h_rstart: nranks + 1
  // starts, then the counters (nranks + 9 words)
  CHECK(RT_KEPT_COUNT == 0 && RT_KEPT_CTR == 1 && RT_KEPT_WORDS == 9, "h_kept");
  for (int n : {1, 4, 8, 256})
    CHECK(rt_rstart_ctr(n) == n + 1 && rt_rstart_words(n) == n + 9, "h_rstart for %d ranks", n);
}

static void lightbuf_counters() {
  // rt_lightbuf.hip at 985109c: "[0] big prims, [1] global prims, [2] never
  // accepted, [3] band, [4] emission overflow", hc[5]
  CHECK(RT_LBC_BIG == 0 && RT_LBC_GLOBAL == 1 && RT_LBC_NEVER == 2 && RT_LBC_BAND == 3 && RT_LBC_OVERFLOW == 4 &&
            RT_LBC_WORDS == 5,
        "light-buffer words");
}

int main() {
  render_stats();
  cand_counters();
  lightbuf_counters();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("counter layout ok\n");
  return 0;
}
