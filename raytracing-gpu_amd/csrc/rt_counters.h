// rt_counters.h -- the words that carry facts from the kernels to the host,
// each layout named once: the render statistics (KParams::stats), the
// candidate-list build's counter block (CandParams::ctr, d_cand_ctr) and the
// light-buffer build's counters (rtl::BP::ctr).  Plain C++ (no HIP): the
// kernels, the host layer, rt_forecast.h and tests/native/counter_layout.cpp
// (which pins every number below) include it.
#pragma once
#include <cstdint>

#include "rt_hip.h"

// ---- per-frame check bits (fold_kernel -> rt_hip_frame_check)
#define RT_FRAME_HITBUF 1u     // hit records past a region's capacity
#define RT_FRAME_DEPTH 2u      // bounce limit or traversal stack overflow
#define RT_FRAME_ZERO 4u       // zero interpolated normal (closest or shadow)
#define RT_FRAME_UNPROVEN 8u   // shadow or reflection queries the exact modes could not prove or decide
#define RT_FRAME_LISTS 16u     // asynchronous list build overflow

// ---- render statistics: X(slot, rt_stats member, the pass that adds to it,
// the frame-check bit a non-zero count raises or 0), in slot order.  A shade
// pass adds to the SHADE slots only (the shadow queries, their lane work and
// clocks, their wave-distinct record fetches); a relight zeroes exactly those
// and keeps the trace's (csrc/rt_recolour.h).
#define RT_STAT_TRACE 1
#define RT_STAT_SHADE 2
#define RT_STAT_LIST(X)                                                 \
  X(CLOSEST, closest, TRACE, 0u)                                        \
  X(SHADOW, shadow, SHADE, 0u)                                          \
  X(PIXELS, pixels, TRACE, 0u)                                          \
  X(NODE_VISITS, node_visits, TRACE, 0u)                                \
  X(TRI_TESTS, tri_tests, TRACE, 0u)                                    \
  X(DEPTH_OVERFLOW, depth_overflow, TRACE, RT_FRAME_DEPTH)              \
  X(ZERO_NORMAL, zero_normal, TRACE, RT_FRAME_ZERO)                     \
  X(HITS, hits, TRACE, 0u)                                              \
  X(CLOSEST_NODE_LANES, closest_node_lanes, TRACE, 0u)                  \
  X(CLOSEST_TRI_LANES, closest_tri_lanes, TRACE, 0u)                    \
  X(SHADOW_NODE_LANES, shadow_node_lanes, SHADE, 0u)                    \
  X(SHADOW_TRI_LANES, shadow_tri_lanes, SHADE, 0u)                      \
  X(CYCLES_CAMERA, cycles_camera, TRACE, 0u)                            \
  X(CYCLES_CAND, cycles_cand, TRACE, 0u)                                \
  X(CYCLES_SECONDARY, cycles_secondary, TRACE, 0u)                      \
  X(CYCLES_SHADOW, cycles_shadow, SHADE, 0u)                            \
  X(CYCLES_SHADOW_DIRECTIONAL, cycles_shadow_directional, SHADE, 0u)    \
  X(STACK_SPILLS, stack_spills, TRACE, 0u)                              \
  X(SHADOW_ZERO_RISK, shadow_zero_risk, SHADE, RT_FRAME_ZERO)           \
  X(SHADOW_NODE_VISITS, shadow_node_visits, SHADE, 0u)                  \
  X(SHADOW_TRI_TESTS, shadow_tri_tests, SHADE, 0u)                      \
  X(SHADOW_UNPROVEN, shadow_unproven, SHADE, RT_FRAME_UNPROVEN)         \
  X(CLOSEST_UNPROVEN, closest_unproven, TRACE, RT_FRAME_UNPROVEN)

enum RtStat : uint32_t {
#define X(slot, member, pass, flag) RT_ST_##slot,
  RT_STAT_LIST(X)
#undef X
      RT_NSTATS
};

// the counters are kept in RT_STAT_SETS copies RT_STAT_STRIDE words apart,
// wave b adding to copy b % 8 (its XCD's): every wave of a launch flushes
// its counters with a few 64-bit atomics, and on a small frame (C1: 4,096
// waves of one work item each) one copy queued them for most of the kernel;
// rt_hip_stats sums the copies
#define RT_STAT_SETS 8
#define RT_STAT_STRIDE 32
static_assert(RT_NSTATS <= RT_STAT_STRIDE, "stat copies overlap");

// whether a shade pass adds to slot k (k < 32)
constexpr bool rt_stat_shade_side(uint32_t k) {
#define X(slot, member, pass, flag) (RT_STAT_##pass == RT_STAT_SHADE ? 1u << RT_ST_##slot : 0u) |
  return ((RT_STAT_LIST(X) 0u) >> k) & 1u;
#undef X
}

// the frame-check bit slot k raises when it is not zero
constexpr uint32_t rt_stat_frame_flag(uint32_t k) {
#define X(slot, member, pass, flag) (k == RT_ST_##slot ? flag : 0u) |
  return RT_STAT_LIST(X) 0u;
#undef X
}

// the rt_stats member slot k fills (rt_hip_stats; the members no slot fills
// are derived there: camera, hit_records, cand_*, shadow_deferred)
inline constexpr unsigned long long rt_stats::*rt_stat_member[RT_NSTATS] = {
#define X(slot, member, pass, flag) &rt_stats::member,
    RT_STAT_LIST(X)
#undef X
};

// ---- candidate-list counters: the RT_CAND_CTR_BLOCK words of d_cand_ctr.
// Words [0, RT_CC_BUILD_WORDS) are one build's counters (CandParams::ctr),
// zeroed by quick_kernel; the build's kernels read them on the device and a
// read-back build copies them to the host in one piece.
enum RtCandCtr : uint32_t {
  RT_CC_RESERVED = 0,    // zeroed with the others, never written or read
  RT_CC_GLOBAL = 1,      // global prims (every camera ray tests them)
  RT_CC_BIG = 2,         // big footprints
  RT_CC_LIST = 3,        // list length
  RT_CC_ITEMS = 4,       // big emission items (item_kernel)
  RT_CC_ITEMS_OVER = 5,  // 1 = more than item_cap items (big_kernel emits instead)
  RT_CC_TOTAL = 6,       // the entry total
  RT_CC_OVERFLOW = 7,    // 1 = an entry past key_cap, or a count past the sizes the build was given
  RT_CC_BUILD_WORDS = 8
};
// [RT_CAND_CTR_SAVED_VALID]: a list's valid count saved from a buffer about to
// be reused (no build writes it); [RT_CAND_CTR_SNAPSHOT, + RT_CC_BUILD_WORDS):
// the last asynchronous build's counters, copied by bounds_kernel
constexpr uint32_t RT_CAND_CTR_SAVED_VALID = 8, RT_CAND_CTR_SNAPSHOT = 16, RT_CAND_CTR_BLOCK = 32;
static_assert(RT_CAND_CTR_SAVED_VALID >= RT_CC_BUILD_WORDS && RT_CAND_CTR_SNAPSHOT > RT_CAND_CTR_SAVED_VALID &&
                  RT_CAND_CTR_SNAPSHOT + RT_CC_BUILD_WORDS <= RT_CAND_CTR_BLOCK,
              "the block's regions overlap");
// The host copies of the build words: h_cand holds them alone; h_kept holds
// the kept count and then them; the partition's h_rstart holds nranks + 1
// offsets and then them (part_scatter_kernel writes that tail).
constexpr uint32_t RT_KEPT_COUNT = 0, RT_KEPT_CTR = 1, RT_KEPT_WORDS = RT_KEPT_CTR + RT_CC_BUILD_WORDS;
constexpr int rt_rstart_ctr(int nranks) { return nranks + 1; }
constexpr int rt_rstart_words(int nranks) { return rt_rstart_ctr(nranks) + (int)RT_CC_BUILD_WORDS; }

// ---- light-buffer build counters (rtl::BP::ctr, rt_lightbuf.hip; row_entries
// of rt_lightbuf_geom.h sets RT_LBC_OVERFLOW)
enum RtLbCtr : uint32_t {
  RT_LBC_BIG = 0,       // big-footprint prims (counted and emitted row-wise by a workgroup)
  RT_LBC_GLOBAL = 1,    // global prims (every shadow ray of the light tests them)
  RT_LBC_NEVER = 2,     // prims never accepted
  RT_LBC_BAND = 3,      // band prims
  RT_LBC_OVERFLOW = 4,  // 1 = the emission disagreed with the count pass (nothing written out of bounds)
  RT_LBC_WORDS = 5
};
