// rt_push_plan.h -- which stack slot each child of a packet-walk interior
// node goes to, as a function of wave-uniform bytes alone, so that the eight
// pushes of stage_push_children (csrc/rt_walk_wave.h) are one vector step:
// lane k (k < 8) handles push-order key k.
//
// A node lists its children in octant order: child c is the c-th set bit of
// `mask`.  The walk pushes them far to near in the order of the wave's
// majority ray octant `dm`: key j = 7 .. 0 visits octant j ^ dm, so the
// nearest wanted child ends on top of the stack.  Serially that is
//
//   for (j = 7; j >= 0; --j) {
//     o = j ^ dm;                     if (!(mask >> o & 1)) continue;
//     c = popc(mask & ((1 << o) - 1)); if (!(hitmask >> c & 1)) continue;
//     if (sp < cap) stack[sp++] = child c; else overflow++;
//   }
//
// and in one step, for lane k: the child of key k (rt_push_lane), whether it
// is pushed (rt_push_wanted), and, with B = the ballot of the pushing lanes,
// its slot sp + rt_push_rank(B, k) -- the pushes of the keys above k come
// first.  A lane stores only while its slot is below cap; rt_push_commit
// gives the stored pushes and the rest, which overflowed.
//
// Plain C++ (no HIP types): the kernels and tests/native/push_plan.cpp, which
// compares it with the loop above over every input, include it.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_PUSH_FN __host__ __device__ inline
#else
#define RT_PUSH_FN static inline
#endif

RT_PUSH_FN uint32_t rt_push_popc8(uint32_t x) {  // of the low 8 bits
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x & 0xffu);
#else
  x &= 0xffu;
  x = (x & 0x55u) + ((x >> 1) & 0x55u);
  x = (x & 0x33u) + ((x >> 2) & 0x33u);
  return (x + (x >> 4)) & 0x0fu;
#endif
}

struct RtPushLane {
  uint32_t child;    // index of the key's child among the node's children (<= 8; a child only if present)
  uint32_t present;  // 1 = the node has a child in the key's octant
};

// key k (only its low three bits count) of a node with child octants `mask`
RT_PUSH_FN RtPushLane rt_push_lane(uint32_t mask, uint32_t dm, uint32_t k) {
  const uint32_t o = (k ^ dm) & 7u;
  RtPushLane p;
  p.child = rt_push_popc8(mask & ((1u << o) - 1u));
  p.present = (mask >> o) & 1u;
  return p;
}

// hitmask: bit c = some lane wants child c (a lane may pass any word whose
// bit p.child says so for its own child)
RT_PUSH_FN bool rt_push_wanted(RtPushLane p, uint32_t hitmask) {
  return p.present != 0 && ((hitmask >> p.child) & 1u) != 0;
}

// pushes that come before key k's: the wanted keys above it.  B: bit j = key
// j is pushed (j < 8)
RT_PUSH_FN uint32_t rt_push_rank(uint32_t B, uint32_t k) { return rt_push_popc8((B & 0xffu) >> ((k & 7u) + 1u)); }

// the pushes of B that fit a stack holding sp of cap entries (the lanes with
// sp + rank < cap stored theirs); *overflow = the ones that did not
RT_PUSH_FN uint32_t rt_push_commit(uint32_t B, int sp, int cap, uint32_t* overflow) {
  const uint32_t n = rt_push_popc8(B), room = (uint32_t)(cap - sp);
  const uint32_t stored = n < room ? n : room;
  *overflow = n - stored;
  return stored;
}
