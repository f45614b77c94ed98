// zero_risk_twin.cpp -- host/rt_zero_risk.h on the CPU (tests/test_geometry_host.py):
// the header the host flatten (host/accel.c) and the device geometry update
// (csrc/rt_geom.hip) share, included here as the device file includes it.  A
// fixed table for the predicate and for every Voronoi region of
// origin_tri_dist2, and rt_flatten flagging the same objects (host/accel.c is
// linked in).  Stand-alone; built plain and with AddressSanitizer + UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

extern "C" {
#include "rt_internal.h"
}
#include "rt_zero_risk.h"

static int failures = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      failures++;                             \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
    }                                         \
  } while (0)

struct Rows {
  const char* name;
  float n[9];
  int risk;
};

static const float kNaN = std::numeric_limits<float>::quiet_NaN();

// the triangle (1, 0, d), (-1, 0, d), (0, 1, d) passes the origin at distance
// d (the point (0, 0, d) of its first edge): the threshold is d^2 < 1e-10
static const Rows kRows[] = {
    {"all +z (the clean triangle)", {0, 0, 1, 0, 0, 1, 0, 0, 1}, 0},
    {"n1 = -z (passes through zero on u = 1/2)", {0, 0, 1, 0, 0, -1, 0, 0, 1}, 1},
    {"n1 = -z, n2 = -z", {0, 0, 1, 0, 0, -1, 0, 0, -1}, 1},
    {"below the threshold: 0.99e-5", {1, 0, 0.99e-5f, -1, 0, 0.99e-5f, 0, 1, 0.99e-5f}, 1},
    {"above the threshold: 1.01e-5", {1, 0, 1.01e-5f, -1, 0, 1.01e-5f, 0, 1, 1.01e-5f}, 0},
    {"below, from the other side", {1, 0, -0.99e-5f, -1, 0, -0.99e-5f, 0, 1, -0.99e-5f}, 1},
    {"above, from the other side", {1, 0, -1.01e-5f, -1, 0, -1.01e-5f, 0, 1, -1.01e-5f}, 0},
    {"a NaN row (normalize of a zero vn) is never zero", {0, 0, 1, kNaN, kNaN, kNaN, 0, 0, -1}, 0},
    {"one NaN component", {0, 0, 1, 0, 0, -1, 0, kNaN, 1}, 0},
};

struct Region {
  const char* name;
  double a[3], b[3], c[3], d2;
};

static const Region kRegions[] = {
    {"vertex A", {1, 1, 0}, {3, 1, 0}, {1, 3, 0}, 2.0},
    {"vertex B", {3, 1, 0}, {1, 1, 0}, {1, 3, 0}, 2.0},
    {"vertex C", {3, 1, 0}, {1, 3, 0}, {1, 1, 0}, 2.0},
    {"edge AB", {-1, 1, 0}, {1, 1, 0}, {0, 3, 0}, 1.0},
    {"edge AC", {-1, 1, 0}, {0, 3, 0}, {1, 1, 0}, 1.0},
    {"edge BC", {0, 3, 0}, {-1, 1, 0}, {1, 1, 0}, 1.0},
    {"edge AB, off centre", {-1, 2, 0}, {3, 2, 0}, {0, 5, 0}, 4.0},
    {"interior", {-1, -1, 2}, {1, -1, 2}, {0, 1, 2}, 4.0},
    {"interior, tilted plane x + z = 2", {2, -3, 0}, {2, 3, 0}, {-2, 0, 4}, 2.0},
};

static rt_triangle tri(float x, const float n1z) {
  rt_triangle t;
  std::memset(&t, 0, sizeof t);
  t.vertex[0] = rt_vec3{x - 2, 0, 0};
  t.vertex[1] = rt_vec3{x + 2, 0, 0};
  t.vertex[2] = rt_vec3{x - 2, 2, 0};
  t.normal[0] = rt_vec3{0, 0, 1};
  t.normal[1] = rt_vec3{0, 0, n1z};
  t.normal[2] = rt_vec3{0, 0, 1};
  return t;
}

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  for (const Rows& r : kRows) {
    CHECK(rt_zero_risk_rows(r.n) == r.risk, "%s: header says %d", r.name, rt_zero_risk_rows(r.n));
    CHECK(rt_tri_normal_can_vanish(r.n) == r.risk, "%s: accel.c says %d", r.name, rt_tri_normal_can_vanish(r.n));
  }
  for (const Region& g : kRegions) {
    const double d2 = origin_tri_dist2(g.a, g.b, g.c);
    CHECK(std::fabs(d2 - g.d2) <= 1e-12, "%s: %.17g, expected %.17g", g.name, d2, g.d2);
  }
  // rt_flatten flags an object iff one of its triangles is risky: object 0
  // clean, object 1 = A risky + B clean, object 2 = B clean + B clean, object 3
  // empty, object 4 risky alone
  std::vector<rt_triangle> t0{tri(0, 1)}, t1{tri(10, -1), tri(20, 1)}, t2{tri(30, 1), tri(40, 1)}, t4{tri(50, -1)};
  rt_object obj[5];
  std::memset(obj, 0, sizeof obj);
  obj[0].triangles = t0.data(), obj[0].triangle_count = 1;
  obj[1].triangles = t1.data(), obj[1].triangle_count = 2;
  obj[2].triangles = t2.data(), obj[2].triangle_count = 2;
  obj[4].triangles = t4.data(), obj[4].triangle_count = 1;
  rt_scene s;
  std::memset(&s, 0, sizeof s);
  s.objects = obj;
  s.object_count = 5;
  rt_flat_scene f;
  const int rc = rt_flatten(&s, RT_ACCEL_FLAT, &f);
  CHECK(rc == RT_OK, "rt_flatten: %d (%s)", rc, rt_last_error());
  if (rc == RT_OK) {
    const int want[6] = {0, 1, 1, 0, 0, 1};
    CHECK(f.ntri == 6 && f.nrec == 6, "%zu triangles, %zu records", f.ntri, f.nrec);
    size_t p = 0;
    for (size_t o = 0; o < s.object_count && f.ntri == 6; o++) {
      int risk = 0;
      for (unsigned k = 0; k < obj[o].triangle_count; k++) risk |= rt_zero_risk_rows(f.nrm + 9 * (p + k));
      for (unsigned k = 0; k < obj[o].triangle_count; k++, p++) {
        const uint32_t flag = bits(f.tri[RT_TRI_FLOATS * p + 11]);
        CHECK(flag == (uint32_t)(want[p] ? RT_REC_ZERO_RISK_BIT : 0), "prim %zu: flag %u", p, flag);
        CHECK((int)flag == risk, "prim %zu: flag %u, the header over the object's rows says %d", p, flag, risk);
        CHECK(bits(f.tri[RT_TRI_FLOATS * p + 10]) == (uint32_t)o, "prim %zu: object word", p);
      }
    }
    // the boxes a geometry update keeps: each prim's exact vertex min / max
    CHECK(f.pbox != nullptr, "rt_flatten(FLAT) keeps the prims' boxes");
    if (f.pbox) {
      CHECK(f.pbox[0] == -2 && f.pbox[1] == 0 && f.pbox[3] == 2 && f.pbox[4] == 2, "prim 0's box");
      CHECK(f.pbox[6 * 5] == 48 && f.pbox[6 * 5 + 3] == 52, "prim 5's box");
    }
    CHECK(f.scene_lo[0] == -2 && f.scene_hi[0] == 52 && f.scene_hi[1] == 2, "scene box");
    rt_flat_free(&f);
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("zero risk twin ok\n");
  return 0;
}
