// push_plan.cpp -- the packet walk's one-step child push of
// csrc/rt_push_plan.h against the serial far-to-near loop it replaced, on the
// CPU (tests/test_push_plan.py builds it plain and with g++
// -fsanitize=address,undefined; no GPU, no HIP).
//
// Exhaustive: every child mask (256), every subset of its children wanted,
// every near octant dm (8) and every room 0 .. 8 left on the stack, at the
// bottom of the stack and against its top.  Both sides push into a stack of
// kCap + 8 guarded entries; the stacks, sp and the overflow count must agree,
// and nothing may be written at or past kCap.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rt_push_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
      failures++;                                                \
    }                                                            \
  } while (0)

static const int kCap = 96;  // kStack2 of csrc/rt_walk_wave.h
static const uint8_t kEmpty = 0xee;

static uint32_t popc(uint32_t x) {
  uint32_t n = 0;
  for (; x; x &= x - 1) n++;
  return n;
}

// the loop of stage_push_children before the vector push, literally; a stack
// entry is the child index it holds
static void serial_push(uint32_t mask, uint32_t hitmask, uint32_t dm, int& sp, uint8_t* stack, uint32_t& overflow) {
  for (int j = 7; j >= 0; --j) {
    uint32_t o = (uint32_t)j ^ dm;
    if (!(mask & (1u << o))) continue;
    uint32_t c = popc(mask & ((1u << o) - 1u));
    if (!(hitmask & (1u << c))) continue;
    if (sp < kCap) {
      stack[sp] = (uint8_t)c;
      sp++;
    } else {
      overflow++;
    }
  }
}

// the vector step as the kernel runs it: the 64 lanes in lockstep, first the
// ballot, then every lane's store
static void vector_push(uint32_t mask, uint32_t hitmask, uint32_t dm, int& sp, uint8_t* stack, uint32_t& overflow) {
  RtPushLane pl[64];
  bool push[64];
  uint32_t B = 0;
  for (uint32_t lane = 0; lane < 64; lane++) {
    pl[lane] = rt_push_lane(mask, dm, lane);
    // a lane knows only whether its own child is wanted
    const uint32_t own = ((hitmask >> pl[lane].child) & 1u) << pl[lane].child;
    push[lane] = lane < 8 && rt_push_wanted(pl[lane], own);
    if (push[lane]) B |= 1u << lane;
  }
  for (uint32_t lane = 0; lane < 64; lane++) {
    const int slot = sp + (int)rt_push_rank(B, lane);
    if (push[lane] && slot < kCap) {
      CHECK(stack[slot] == kEmpty, "mask %02x hit %02x dm %u sp %d: slot %d written twice", mask, hitmask, dm, sp, slot);
      stack[slot] = (uint8_t)pl[lane].child;
    }
  }
  uint32_t over = 0;
  sp += (int)rt_push_commit(B, sp, kCap, &over);
  overflow += over;
}

int main() {
  long cases = 0;
  for (uint32_t mask = 0; mask < 256; mask++) {
    const uint32_t cnt = popc(mask);
    for (uint32_t hitmask = 0; hitmask < (1u << cnt); hitmask++)
      for (uint32_t dm = 0; dm < 8; dm++)
        for (int room = 0; room <= 8; room++) {
          uint8_t a[kCap + 8], b[kCap + 8];
          std::memset(a, kEmpty, sizeof a);
          std::memset(b, kEmpty, sizeof b);
          int spa = kCap - room, spb = spa;
          uint32_t ova = 0, ovb = 0;
          serial_push(mask, hitmask, dm, spa, a, ova);
          vector_push(mask, hitmask, dm, spb, b, ovb);
          cases++;
          CHECK(spa == spb && ova == ovb, "mask %02x hit %02x dm %u room %d: sp %d / %d, overflow %u / %u", mask, hitmask,
                dm, room, spa, spb, ova, ovb);
          CHECK(std::memcmp(a, b, sizeof a) == 0, "mask %02x hit %02x dm %u room %d: stacks differ", mask, hitmask, dm,
                room);
          CHECK(ova == popc(hitmask) - (uint32_t)(spa - (kCap - room)), "mask %02x hit %02x room %d: %u lost", mask,
                hitmask, room, ova);
          for (int g = kCap; g < kCap + 8; g++) CHECK(b[g] == kEmpty, "write past the stack at %d", g);
          if (room == 8) {  // the same node on an empty stack: the same children from slot 0
            uint8_t e[kCap + 8];
            std::memset(e, kEmpty, sizeof e);
            int spe = 0;
            uint32_t ove = 0;
            vector_push(mask, hitmask, dm, spe, e, ove);
            CHECK(ove == 0 && spe == (int)popc(hitmask) && std::memcmp(e, a + kCap - 8, 8) == 0,
                  "mask %02x hit %02x dm %u on an empty stack", mask, hitmask, dm);
          }
        }
  }
  // the nearest wanted child ends on top: key 0's octant is dm itself
  {
    uint8_t s[kCap + 8];
    std::memset(s, kEmpty, sizeof s);
    int sp = 3;
    uint32_t ov = 0;
    vector_push(0xffu, 0xffu, 5u, sp, s, ov);
    CHECK(sp == 11 && s[10] == 5 && s[3] == (5 ^ 7), "full node, dm 5: top %d bottom %d", s[10], s[3]);
  }
  CHECK(cases == 472392, "%ld cases", cases);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("push plan ok (%ld cases)\n", cases);
  return 0;
}
