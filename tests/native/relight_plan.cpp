// relight_plan.cpp -- the relight bookkeeping (csrc/rt_relight.h) driven
// through scripted edits on the CPU, every answer checked against a table
// (tests/test_relight_host.py builds it plain and with
// g++ -fsanitize=address,undefined; no GPU, no HIP).
//
// The expected values follow from the rules in include/rt_hip.h
// (rt_hip_set_lights, rt_hip_relight), not from running this code:
//   * a casting light (type 1 directional, 2 point) is clean iff its index is
//     below 32, a shade pass of the kept records wrote its bit, and its
//     (type, v) is bitwise what it was then; index >= 32: always dirty;
//     ambient (0) and specular-type (3) lights never query;
//   * a buffer is rebuilt for a casting light at a new index or whose
//     (type, v) changed, released for an old casting light that changed or
//     went; a colour never enters;
//   * path: no dirty light -> recolour; dirty and clean casting lights ->
//     partial; every casting light dirty -> full.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rt_relight.h"

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

static RelightLight L(uint32_t type, float x, float y, float z) {
  const float v[3] = {x, y, z};
  return RelightLight(type, v);
}

typedef std::vector<RelightLight> Table;

// the `spheres` shape: ambient, directional, four point lights (5 casting)
static Table spheres() {
  return Table{L(0, 0, 0, 0), L(1, 0.5f, -1, 0.25f), L(2, 3, 4, 5), L(2, -3, 4, 5), L(2, 3, 4, -5), L(2, -3, 4, -5)};
}

static std::string bits(const std::vector<uint8_t>& v) {
  std::string s;
  for (uint8_t b : v) s += b ? '1' : '0';
  return s;
}

struct Expect {
  const char* rebuild;  // per new light
  const char* release;  // per old light
  RelightPath path;
  uint32_t dirty, clean, high, casting;
};

static void edit(const char* what, RelightPlan& plan, Table& table, const Table& now, const Expect& e) {
  std::vector<uint8_t> rebuild, release;
  plan.set_lights(table, now, rebuild, release);
  table = now;
  const RelightWork w = plan.work(table);
  CHECK(bits(rebuild) == e.rebuild, "%s: rebuild %s, expected %s", what, bits(rebuild).c_str(), e.rebuild);
  CHECK(bits(release) == e.release, "%s: release %s, expected %s", what, bits(release).c_str(), e.release);
  CHECK(w.path == e.path, "%s: path %d, expected %d", what, (int)w.path, (int)e.path);
  CHECK(w.dirty == e.dirty, "%s: dirty %#x, expected %#x", what, w.dirty, e.dirty);
  CHECK(w.clean == e.clean, "%s: clean %#x, expected %#x", what, w.clean, e.clean);
  CHECK(w.high == e.high, "%s: high %u, expected %u", what, w.high, e.high);
  CHECK(w.casting == e.casting, "%s: casting %u, expected %u", what, w.casting, e.casting);
  CHECK(w.queried() == (uint32_t)__builtin_popcount(e.dirty) + e.high, "%s: queried %u", what, w.queried());
}

static void same_work(const char* what, const RelightPlan& plan, const Table& t, RelightPath path, uint32_t dirty,
                      uint32_t clean, uint32_t high) {
  const RelightWork w = plan.work(t);
  CHECK(w.path == path && w.dirty == dirty && w.clean == clean && w.high == high,
        "%s: path %d dirty %#x clean %#x high %u", what, (int)w.path, w.dirty, w.clean, w.high);
}

int main() {
  const uint32_t C5 = 0x3e;  // spheres' casting lights 1..5

  {  // a fresh context: nothing written, every casting light dirty -> full
    RelightPlan plan;
    same_work("fresh", plan, spheres(), RT_RELIGHT_FULL, C5, 0, 0);
    // the first relight (or a keep-visibility render) writes every bit
    plan.masks_written();
    same_work("after a relight", plan, spheres(), RT_RELIGHT_RECOLOUR, 0, C5, 0);
  }

  {  // colour-only edits: the table's (type, v) is unchanged -> nothing rebuilt, recolour
    RelightPlan plan;
    Table t = spheres();
    plan.masks_written();
    edit("colour only", plan, t, spheres(), {"000000", "000000", RT_RELIGHT_RECOLOUR, 0, C5, 0, 5});
    // ... also before any mask exists: nothing rebuilt, but the relight queries everything
    RelightPlan cold;
    Table u = spheres();
    edit("colour only, no masks", cold, u, spheres(), {"000000", "000000", RT_RELIGHT_FULL, C5, 0, 0, 5});
  }

  {  // a moved light: its buffer only, partial
    RelightPlan plan;
    Table t = spheres(), n = spheres();
    plan.masks_written();
    n[5] = L(2, -3 + 0.75f, 4, -5);
    edit("light 5 moved", plan, t, n, {"000001", "000001", RT_RELIGHT_PARTIAL, 1u << 5, C5 & ~(1u << 5), 0, 5});
    // moved back before any relight: the bit stays cleared (the masks were
    // not rewritten; "has not changed since" is not tracked through a round trip)
    edit("light 5 moved back", plan, t, spheres(),
         {"000001", "000001", RT_RELIGHT_PARTIAL, 1u << 5, C5 & ~(1u << 5), 0, 5});
    plan.masks_written();
    same_work("relit", plan, t, RT_RELIGHT_RECOLOUR, 0, C5, 0);
    // -0.0f is another bit pattern than 0.0f
    n = spheres();
    n[0] = L(0, -0.0f, 0, 0);
    edit("ambient's unused v changed", plan, t, n, {"000000", "000000", RT_RELIGHT_RECOLOUR, 0, C5, 0, 5});
  }

  {  // type changes
    RelightPlan plan;
    Table t = spheres(), n = spheres();
    plan.masks_written();
    n[1] = L(2, 0.5f, -1, 0.25f);  // directional -> point, same v
    edit("directional -> point", plan, t, n, {"010000", "010000", RT_RELIGHT_PARTIAL, 1u << 1, C5 & ~2u, 0, 5});
    plan.masks_written();
    n[2].type = 0;  // point -> ambient: its buffer goes, nothing to query
    edit("point -> ambient", plan, t, n, {"000000", "001000", RT_RELIGHT_RECOLOUR, 0, C5 & ~4u, 0, 4});
    n[2].type = 2;  // and back: a new buffer, dirty (its bit was cleared by the change)
    edit("ambient -> point", plan, t, n, {"001000", "000000", RT_RELIGHT_PARTIAL, 1u << 2, C5 & ~4u, 0, 5});
    plan.masks_written();
    n[3].type = 3;  // point -> specular-type: never queries
    edit("point -> specular type", plan, t, n, {"000000", "000100", RT_RELIGHT_RECOLOUR, 0, C5 & ~8u, 0, 4});
  }

  {  // append, remove (later indices shift), insert
    RelightPlan plan;
    Table t = spheres(), n = spheres();
    plan.masks_written();
    n.push_back(L(2, 0, 9, 0));
    edit("append", plan, t, n, {"0000001", "000000", RT_RELIGHT_PARTIAL, 1u << 6, C5, 0, 6});
    plan.masks_written();
    n.erase(n.begin() + 2);  // 3 -> 2, 4 -> 3, 5 -> 4, 6 -> 5: every shifted index differs from its old light
    edit("remove light 2", plan, t, n, {"001111", "0011111", RT_RELIGHT_PARTIAL, 0x3c, 0x02, 0, 5});
    plan.masks_written();
    n.insert(n.begin(), L(0, 0, 0, 0));  // a second ambient in front: everything shifts up
    // new index 1 is the old ambient (not casting): nothing built for it
    edit("insert in front", plan, t, n, {"0011111", "011111", RT_RELIGHT_FULL, 0x7c, 0, 0, 5});
    plan.masks_written();
    n.pop_back();
    edit("remove the last", plan, t, n, {"000000", "0000001", RT_RELIGHT_RECOLOUR, 0, 0x3c, 0, 4});
  }

  {  // 0 lights, and back
    RelightPlan plan;
    Table t = spheres();
    plan.masks_written();
    edit("n = 0", plan, t, Table{}, {"", "011111", RT_RELIGHT_RECOLOUR, 0, 0, 0, 0});
    plan.masks_written();
    edit("back from 0", plan, t, spheres(), {"011111", "", RT_RELIGHT_FULL, C5, 0, 0, 5});
    RelightPlan cold;
    same_work("no lights, no masks", cold, Table{}, RT_RELIGHT_RECOLOUR, 0, 0, 0);
    Table amb{L(0, 0, 0, 0), L(3, 1, 1, 1)};
    same_work("no casting light, no masks", cold, amb, RT_RELIGHT_RECOLOUR, 0, 0, 0);
  }

  {  // 33 and more lights: index >= 32 is always dirty
    Table t = spheres();
    for (int k = 0; k < 28; k++) t.push_back(L(2, (float)k, 8, 1));  // 34 lights, indices 32, 33 casting
    RelightPlan plan;
    same_work("34 lights, fresh", plan, t, RT_RELIGHT_FULL, 0xfffffffeu, 0, 2);
    plan.masks_written();
    same_work("34 lights, written", plan, t, RT_RELIGHT_PARTIAL, 0, 0xfffffffeu, 2);
    Table n = t;
    std::string none(34, '0');
    edit("34 lights, colour only", plan, t, n, {none.c_str(), none.c_str(), RT_RELIGHT_PARTIAL, 0, 0xfffffffeu, 2, 33});
    n[33] = L(2, 100, 8, 1);
    std::string r33 = none;
    r33[33] = '1';
    edit("light 33 moved", plan, t, n, {r33.c_str(), r33.c_str(), RT_RELIGHT_PARTIAL, 0, 0xfffffffeu, 2, 33});
    n[31] = L(2, 100, 8, 2);
    std::string r31 = none;
    r31[31] = '1';
    edit("light 31 moved", plan, t, n, {r31.c_str(), r31.c_str(), RT_RELIGHT_PARTIAL, 1u << 31, 0x7ffffffeu, 2, 33});
    // the extra lights ambient: nothing past 31 casts -> recolour
    Table a = spheres();
    for (int k = 0; k < 28; k++) a.push_back(L(0, 0, 0, 0));
    RelightPlan p2;
    p2.masks_written();
    same_work("34 lights, extras ambient", p2, a, RT_RELIGHT_RECOLOUR, 0, C5, 0);
    // exactly 33, the 33rd casting, the first 32 not: every casting light dirty -> full
    Table b;
    for (int k = 0; k < 32; k++) b.push_back(L(0, 0, 0, 0));
    b.push_back(L(1, 0, -1, 0));
    same_work("33 lights, only the last casts", p2, b, RT_RELIGHT_FULL, 0, 0, 1);
  }

  {  // every invalidating event ends in the same call: all bits cleared.  The
     // events: a render without keep-visibility, rt_hip_set_exact_shadows,
     // rt_hip_set_light_buffers, rt_hip_set_lightbuf_entry_cap,
     // rt_hip_set_cull_slack, a hit-buffer reallocation
    const char* events[] = {"render without keep-visibility", "set_exact_shadows", "set_light_buffers",
                            "set_lightbuf_entry_cap", "set_cull_slack", "hit buffers reallocated"};
    for (const char* ev : events) {
      RelightPlan plan;
      Table t = spheres();
      plan.masks_written();
      same_work(ev, plan, t, RT_RELIGHT_RECOLOUR, 0, C5, 0);
      plan.invalidate();
      same_work(ev, plan, t, RT_RELIGHT_FULL, C5, 0, 0);
      CHECK(plan.current == 0, "%s: bits %#x left", ev, plan.current);
      // a render with keep-visibility, or the relight that follows, restores them
      plan.masks_written();
      same_work(ev, plan, t, RT_RELIGHT_RECOLOUR, 0, C5, 0);
    }
    // a moved light, then an invalidating event, then the relight: one state
    RelightPlan plan;
    Table t = spheres(), n = spheres();
    plan.masks_written();
    n[2] = L(2, 3, 4, 6);
    edit("moved", plan, t, n, {"001000", "001000", RT_RELIGHT_PARTIAL, 4, C5 & ~4u, 0, 5});
    plan.invalidate();
    same_work("moved + invalidated", plan, t, RT_RELIGHT_FULL, C5, 0, 0);
  }

  if (failures) {
    std::printf("%d relight plan checks failed\n", failures);
    return 1;
  }
  std::printf("relight plan table ok\n");
  return 0;
}
