// rt_relight.h -- the bookkeeping of rt_hip_relight (rt_hip.cpp): which of the
// kept hit records' unshadowed-light mask bits (lights 0..31, KParams::hit_lit)
// are current, and from that which lights' buffers an edit of the light table
// rebuilds, which lights the next relight must query (the dirty ones) and
// which of its three paths runs.  Plain C++ (no HIP): rt_hip.cpp makes the
// builds and launches and tells this what happened;
// tests/native/relight_plan.cpp drives it on the CPU.
//
// A shadow-casting light (directional or point) is clean -- its stored bit
// decides, no query -- if and only if its index is below 32, a shade pass of
// the kept records wrote its bit, and its (type, v) has not changed since.
// Lights from index 32 up have no bit: always dirty.  Ambient and
// specular-type lights never query.  Colours and materials touch nothing here:
// a shadow decision does not depend on them (cpu/light.c:24-31).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

// A light's shadow-relevant part, compared bitwise (-0.0f != 0.0f, NaN == the
// same NaN: an equal bit pattern asks the same queries).
struct RelightLight {
  uint32_t type = 0;
  uint32_t v[3] = {0, 0, 0};
  RelightLight() = default;
  RelightLight(uint32_t t, const float lv[3]) : type(t) { std::memcpy(v, lv, sizeof v); }
  bool casts() const { return type == 1 || type == 2; }
  bool same(const RelightLight& o) const { return type == o.type && std::memcmp(v, o.v, sizeof v) == 0; }
};

enum RelightPath {
  RT_RELIGHT_RECOLOUR = 0,  // no light dirty: recolour_kernel, no query
  RT_RELIGHT_PARTIAL = 1,   // some casting lights dirty, some clean: shade_kernel's relight instantiation
  RT_RELIGHT_FULL = 2       // every casting light dirty: today's shade kernel, writing the masks
};

// What the next relight does under a light table.
struct RelightWork {
  RelightPath path = RT_RELIGHT_RECOLOUR;
  uint32_t dirty = 0;     // lights 0..31 to query
  uint32_t clean = 0;     // casting lights 0..31 decided by their stored bit
  uint32_t high = 0;      // casting lights of index >= 32 (always queried)
  uint32_t casting = 0;   // casting lights in all
  uint32_t queried() const { return (uint32_t)__builtin_popcount(dirty) + high; }
};

struct RelightPlan {
  // bit li: the mask bit of light li is current for the kept records (it
  // means nothing for a light that does not cast shadows: to become casting
  // its type changes, which clears it)
  uint32_t current = 0;

  // The events that clear every bit: a render without keep-visibility (new
  // records, no masks), a setting that changes shadow decisions' provenance
  // (rt_hip_set_exact_shadows, rt_hip_set_light_buffers,
  // rt_hip_set_lightbuf_entry_cap, rt_hip_set_cull_slack), a reallocation of
  // the hit buffers (the mask buffer goes with them).
  void invalidate() { current = 0; }
  // A relight, or a render with keep-visibility: the shade pass (or the
  // recolour, which keeps them) left every bit of lights 0..31 current.
  void masks_written() { current = 0xffffffffu; }

  // rt_hip_set_lights: the table `was` becomes `now`.  rebuild[li] = light
  // li's buffer must be built (a casting light at a new index or whose
  // (type, v) changed); a casting light that is unchanged keeps its buffer, an
  // index that no longer casts or no longer exists gives its buffer up
  // (release[li], li over the old table).  The bits of changed and removed
  // indices are cleared.
  void set_lights(const std::vector<RelightLight>& was, const std::vector<RelightLight>& now,
                  std::vector<uint8_t>& rebuild, std::vector<uint8_t>& release) {
    rebuild.assign(now.size(), 0);
    release.assign(was.size(), 0);
    for (size_t li = 0; li < now.size(); li++) {
      const bool changed = li >= was.size() || !now[li].same(was[li]);
      if (changed && li < 32) current &= ~(1u << li);
      if (changed && now[li].casts()) rebuild[li] = 1;
      if (changed && li < was.size() && was[li].casts()) release[li] = 1;
    }
    for (size_t li = now.size(); li < was.size(); li++) {
      if (li < 32) current &= ~(1u << li);
      if (was[li].casts()) release[li] = 1;
    }
  }

  RelightWork work(const std::vector<RelightLight>& table) const {
    RelightWork w;
    for (size_t li = 0; li < table.size(); li++) {
      if (!table[li].casts()) continue;
      w.casting++;
      if (li >= 32)
        w.high++;
      else if ((current >> li) & 1u)
        w.clean |= 1u << li;
      else
        w.dirty |= 1u << li;
    }
    if (!w.dirty && !w.high)
      w.path = RT_RELIGHT_RECOLOUR;
    else if (w.clean)
      w.path = RT_RELIGHT_PARTIAL;
    else
      w.path = RT_RELIGHT_FULL;
    return w;
  }
};
