// lightbuf_geom.cpp -- the light buffers' contract between build and query on
// the CPU: the footprint geometry (csrc/rt_lightbuf_geom.h), the grid and the
// survey (csrc/rt_lightbuf_host.cpp) and the query's cell map
// (csrc/rt_lightbuf_cell.h) against the reference's float Moller-Trumbore test
// (host/rt_mt.h).  tests/test_lightbuf_geom.py builds it plain and with
// g++ -fsanitize=address,undefined; no GPU, no librtgpu.so.
//
// A deterministic set of triangles (integer LCG, no file input) in a box of
// 40 units: small ones, slivers, triangles whose plane holds the directional
// light's direction to within 1e-7 of |a| (candidates for `never`), triangles
// whose plane passes within 1e-3 of the point light (candidates for the band
// and the global list), middle-sized ones and a few that span the box (more
// than kSmallCells cells).  One directional and one point light; LBParams
// from lb_fill over the triangles' own extent with the default slack, at
// lb_fill's target_cells and at 16 times as many; both footprint modes.
// For each of the eight builds:
//   1. every triangle's rows: the counts of row_entries<false> add up to the
//      entries row_entries<true> writes (through the emission's own loop and
//      bounds check, over host memory), every cell is below the cell count,
//      no key is NaN, no row at or past foot_rows is asked for;
//   2. rt_lightbuf_survey_host at stride 1 gives the same totals;
//   3. soundness: eight shadow rays leave every triangle (hit points
//      (float)(v0 + u e1 + v e2), directions as the shade pass forms them);
//      every triangle mt_exact accepts for a ray is global, or listed in the
//      query's first cell with a key no larger than the query's limit, or
//      (point light) listed in its second cell -- and is never `never`.
//      Every accepted pair is checked, in both modes;
//   4. the set is not vacuous (the thresholds at the end of run()).
// A second pass puts every row of tests/light_edges_util.py's light table
// (kRows; positions scaled by 5 to this box) in the lights' place, adds the
// integer lattice of the box to the origins, and applies checks 1-3 to every
// row; non-vacuity is per row: where the reference accepts pairs, at least
// 1,000 accepted and at least 50 found through a cell (first and second cell
// counted apart: around a light inside the geometry nearly every pair is a
// global one); exactly 0 accepted under the tiny, denormal and huge
// directions and the point lights 1e9 and 3e38 away; every triangle `never`
// under the tiny and denormal directions in proven mode; and the zero vector
// refused by lb_geom_host with its message.  The five point lights on the
// lattice run once more over triangles on the lattice (the faces of the box in
// squares of 4: edges and vertices exactly in the cube map's face boundaries
// and on the origins).  A third pass: +-inf and NaN in one
// component, both kinds of light, refused with a reason of their own (host
// only: nothing of it goes near a device).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "rt_lightbuf_cell.h"
#include "rt_lightbuf_geom.h"
#include "rt_mt.h"

static int failures = 0;
#define CHECK(cond, ...)                                           \
  do {                                                             \
    if (!(cond)) {                                                 \
      if (failures < 20) {                                         \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
        std::printf(__VA_ARGS__);                                  \
        std::printf("\n");                                         \
      }                                                            \
      failures++;                                                  \
    }                                                              \
  } while (0)

struct Lcg {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 32);
  }
  double uni() { return next() * (1.0 / 4294967296.0); }  // [0, 1)
  double sym() { return 2.0 * uni() - 1.0; }              // [-1, 1)
  double log_between(double a, double b) { return a * std::pow(b / a, uni()); }
};

static const double kBox = 20.0;                          // triangles start in [-kBox, kBox]^3
static const float kDirLight[3] = {0.37f, -0.81f, 0.45f};  // l.v of the directional light: rays leave along -l.v
static const float kPointLight[3] = {3.5f, 6.25f, -2.75f};

static double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void unit(double* v) {
  const double l = std::sqrt(dot(v, v));
  for (int a = 0; a < 3; a++) v[a] /= l;
}
static void random_dir(Lcg& g, double* v) {
  do {
    for (int a = 0; a < 3; a++) v[a] = g.sym();
  } while (dot(v, v) < 0.01);
  unit(v);
}
// a unit vector perpendicular to the unit vector a
static void random_perp(Lcg& g, const double* a, double* b) {
  do {
    random_dir(g, b);
    const double ab = dot(a, b);
    for (int k = 0; k < 3; k++) b[k] -= ab * a[k];
  } while (dot(b, b) < 0.04);
  unit(b);
}
static void box_point(Lcg& g, double* x) {
  for (int a = 0; a < 3; a++) x[a] = kBox * g.sym();
}

// one record: v0, e1, e2 and the three words the device keeps (unused here)
static void push(std::vector<float4>& tri, const double* v0, const double* e1, const double* e2) {
  tri.push_back(float4{(float)v0[0], (float)v0[1], (float)v0[2], (float)e1[0]});
  tri.push_back(float4{(float)e1[1], (float)e1[2], (float)e2[0], (float)e2[1]});
  tri.push_back(float4{(float)e2[2], 0.0f, 0.0f, 0.0f});
}

static void scaled_pair(Lcg& g, double l1, double l2, double* e1, double* e2) {
  random_dir(g, e1);
  random_dir(g, e2);
  for (int a = 0; a < 3; a++) {
    e1[a] *= l1;
    e2[a] *= l2;
  }
}

static std::vector<float4> make_triangles(int n) {
  std::vector<float4> tri;
  Lcg g{0x11B0FULL};
  const double dl[3] = {-(double)kDirLight[0], -(double)kDirLight[1], -(double)kDirLight[2]};
  double dh[3] = {dl[0], dl[1], dl[2]};
  unit(dh);
  for (int i = 0; i < n; i++) {
    const uint32_t kind = g.next() % 100u;
    double v0[3], e1[3], e2[3];
    if (kind < 30) {  // small
      box_point(g, v0);
      scaled_pair(g, g.log_between(0.05, 1.5), g.log_between(0.05, 1.5), e1, e2);
    } else if (kind < 42) {  // slivers: a long side and a very short one
      box_point(g, v0);
      scaled_pair(g, g.log_between(1.0, 15.0), g.log_between(1e-4, 1e-2), e1, e2);
    } else if (kind < 60) {
      // edge-on to the directional light: e1 along the rays, e2 tilted out of
      // a plane holding them so that |a| = |d . (e1 x e2)| is 0 .. 2e-7
      box_point(g, v0);
      double b[3], c[3];
      random_perp(g, dh, b);
      c[0] = dh[1] * b[2] - dh[2] * b[1];
      c[1] = dh[2] * b[0] - dh[0] * b[2];
      c[2] = dh[0] * b[1] - dh[1] * b[0];
      const double l1 = g.log_between(0.05, 2.0), l2 = g.log_between(0.05, 2.0);
      const double dlen = std::sqrt(dot(dl, dl)), tilt = 2e-7 * g.uni() / (dlen * l1 * l2);
      const double th = 6.283185307179586 * g.uni();
      for (int a = 0; a < 3; a++) {
        e1[a] = l1 * dh[a];
        e2[a] = l2 * (std::cos(th) * dh[a] + std::sin(th) * b[a]) + l2 * tilt * c[a];
      }
    } else if (kind < 80) {
      // the plane within 1e-3 of the point light: spanned by a and b, at
      // delta along their normal, the first corner s along a from the foot point
      double a[3], b[3], nrm[3];
      random_dir(g, a);
      random_perp(g, a, b);
      nrm[0] = a[1] * b[2] - a[2] * b[1];
      nrm[1] = a[2] * b[0] - a[0] * b[2];
      nrm[2] = a[0] * b[1] - a[1] * b[0];
      const double delta = 1e-3 * g.sym(), s = g.log_between(0.3, 12.0), t = 1.5 * g.sym();
      const double th1 = 6.283185307179586 * g.uni(), th2 = th1 + 0.3 + 2.5 * g.uni();
      const double l1 = g.log_between(0.05, 3.0), l2 = g.log_between(0.05, 3.0);
      for (int k = 0; k < 3; k++) {
        v0[k] = (double)kPointLight[k] + delta * nrm[k] + s * a[k] + t * b[k];
        e1[k] = l1 * (std::cos(th1) * a[k] + std::sin(th1) * b[k]);
        e2[k] = l2 * (std::cos(th2) * a[k] + std::sin(th2) * b[k]);
      }
    } else if (kind < 96) {  // middle-sized: most of the accepted pairs
      box_point(g, v0);
      scaled_pair(g, g.log_between(2.0, 8.0), g.log_between(2.0, 8.0), e1, e2);
    } else {  // across the box: more than kSmallCells cells at 16 times lb_fill's cells
      box_point(g, v0);
      scaled_pair(g, g.log_between(30.0, 45.0), g.log_between(30.0, 45.0), e1, e2);
      for (int a = 0; a < 3; a++) v0[a] = 0.4 * v0[a] - (e1[a] + e2[a]) / 3.0;
    }
    if (i < 2) {
      // two that span the whole set's extent: their bounding rectangle is most
      // of any grid over it, more than kSmallCells cells of lb_fill's own
      const double s = i ? -1.0 : 1.0;
      const double w0[3] = {-44.0 * s, -40.0, -42.0 * s}, w1[3] = {90.0 * s, 6.0, 10.0 * s}, w2[3] = {8.0 * s, 84.0, 80.0 * s};
      for (int a = 0; a < 3; a++) {
        v0[a] = w0[a];
        e1[a] = w1[a];
        e2[a] = w2[a];
      }
    }
    push(tri, v0, e1, e2);
  }
  return tri;
}

// The kernels' parameter over host memory: row_entries<true> writes through it.
struct HostBP : rtl::LbGeom {
  unsigned long long* keys;
  uint32_t* vals;
  uint32_t* ctr;
};

struct Entry {
  uint32_t cell;
  float key;
};

static const int kRaysPerTri = 8;

// What the reference's test gives for a row's shadow rays.
enum Gives { kShadows, kNothing, kNoGrid };
struct Row {
  const char* name;  // tests/light_edges_util.py ROW_NAMES (tests/test_lightbuf_geom.py compares)
  uint32_t type;
  float v[3];  // geom_rows(): a direction as it is, a position times 5
  Gives gives;
  bool lattice;  // the table's on-the-lattice flag: run once more over the lattice triangles
};
static const Row kRows[] = {
    {"dir 0 -1 0", 1u, {0.0f, -1.0f, 0.0f}, kShadows, false},
    {"dir 1 0 0", 1u, {1.0f, 0.0f, 0.0f}, kShadows, false},
    {"dir 0 1 0 from below", 1u, {0.0f, 1.0f, 0.0f}, kShadows, false},
    {"dir -0 0 1", 1u, {-0.0f, 0.0f, 1.0f}, kShadows, false},
    {"dir 1 1 0", 1u, {1.0f, 1.0f, 0.0f}, kShadows, false},
    {"dir 1 -1 1", 1u, {1.0f, -1.0f, 1.0f}, kShadows, false},
    {"dir 1 1e-8 0", 1u, {1.0f, 9.99999994e-09f, 0.0f}, kShadows, false},
    {"dir 0.5 -0.25 0", 1u, {0.5f, -0.25f, 0.0f}, kShadows, false},
    {"dir 1e-20 0 0", 1u, {9.99999968e-21f, 0.0f, 0.0f}, kNothing, false},
    {"dir denormal", 1u, {3.00000065e-39f, 3.00000065e-39f, 0.0f}, kNothing, false},
    {"dir 1e30", 1u, {1.00000002e+30f, -1.00000002e+30f, 1.00000002e+30f}, kNothing, false},
    {"dir zero", 1u, {0.0f, 0.0f, 0.0f}, kNoGrid, false},
    {"point lattice centre", 2u, {0.0f, 0.0f, 0.0f}, kShadows, true},
    {"point wall vertex", 2u, {20.0f, 0.0f, 0.0f}, kShadows, true},
    {"point wall plane", 2u, {20.0f, 30.0f, 0.0f}, kShadows, true},
    {"point box corner", 2u, {-40.0f, -20.0f, -40.0f}, kShadows, true},
    {"point inside the closed box", 2u, {10.0f, -10.0f, 10.0f}, kShadows, true},
    {"point 1e6 0 0", 2u, {5000000.0f, 0.0f, 0.0f}, kShadows, false},
    {"point 1e6 1e6 1e6", 2u, {5000000.0f, 5000000.0f, 5000000.0f}, kShadows, false},
    {"point 0 1e9 0", 2u, {0.0f, 5e+09f, 0.0f}, kNothing, false},
    {"point 3e38", 2u, {3.00000001e+38f, 3.00000001e+38f, 3.00000001e+38f}, kNothing, false},
    {"point off the lattice", 2u, {20.0f, 40.0f, 60.0000038f}, kShadows, false},
};

static const char* g_tag = "row";  // what a row's lines start with: "row", or "lattice row" over the lattice triangles

static void run(const std::vector<float4>& tri, const std::vector<rt_vec3>& origins, const float sc[3], float sr,
                const float blo[3], const float bhi[3], uint32_t type, const float lv[3], int proven, uint32_t cell_mul,
                const Row* row = nullptr) {
  using namespace rtl;
  const uint32_t nprim = (uint32_t)(tri.size() / 3);
  char err[256] = {0};
  LBParams lp;
  lb_fill(lp, sc, sr, blo, bhi, 64.0f, type, lv, nprim, proven);  // 64: the default culling slack in ulps
  lp.tri = tri.data();
  lp.target_cells *= cell_mul;
  HostBP p{};
  RtLightBuf lb;
  uint64_t ncell = 0;
  const int gr = lb_geom_host(&lp, p, &lb, ncell, err, sizeof err);
  if (row && row->gives == kNoGrid) {  // no grid: the light's queries walk
    CHECK(gr == 1 && std::strcmp(err, "directional light with a zero vector") == 0 && lb.kind == RT_LB_NONE,
          "%s: lb_geom_host %d '%s' kind %u", row->name, gr, err, lb.kind);
    std::printf("%s %s | %s x%u: refused: %s\n", g_tag, row->name, proven ? "proven" : "slack", cell_mul, err);
    return;
  }
  CHECK(gr == 0, "lb_geom_host: %d %s", gr, err);
  if (gr) return;
  uint32_t ctr[RT_LBC_WORDS] = {};
  p.ctr = ctr;

  // ---- 1. every triangle's rows, counted and emitted
  std::vector<std::vector<Entry>> listed(nprim);  // per prim, by cell
  std::vector<char> is_global(nprim, 0), is_never(nprim, 0);
  unsigned long long entries = 0, n_never = 0, n_global = 0, n_band = 0, n_big = 0, band_entries = 0, max_count = 0;
  std::vector<unsigned long long> keys;
  std::vector<uint32_t> vals, counts;
  for (uint32_t prim = 0; prim < nprim; prim++) {
    Foot f;
    footprint(p, prim, f);
    if (f.never) {
      is_never[prim] = 1;
      n_never++;
      continue;
    }
    if (f.global) {
      is_global[prim] = 1;
      n_global++;
      continue;
    }
    n_band += f.band;
    n_big += foot_is_big(p, f);
    const uint32_t rows = foot_rows(p, f);
    counts.assign(rows, 0u);
    uint64_t c = 0;
    for (uint32_t r = 0; r < rows; r++) {
      counts[r] = row_entries<false>(p, f, prim, r, 0, 0);
      c += counts[r];
      if (f.band && r >= rows - 6u * p.n) band_entries += counts[r];
    }
    keys.assign(c + 1, ~0ull);  // one past the prim's range: must stay untouched
    vals.assign(c + 1, ~0u);
    p.keys = keys.data();
    p.vals = vals.data();
    uint64_t at = 0;
    for (uint32_t r = 0; r < rows; r++) {
      const uint32_t e = row_entries<true>(p, f, prim, r, at, c);
      CHECK(e == counts[r], "prim %u row %u of %u: counted %u, emitted %u", prim, r, rows, counts[r], e);
      at += e;
    }
    CHECK(at == c && ctr[RT_LBC_OVERFLOW] == 0 && keys[c] == ~0ull && vals[c] == ~0u,
          "prim %u: counted %llu, emitted %llu, overflow flag %u", prim, (unsigned long long)c, (unsigned long long)at,
          ctr[RT_LBC_OVERFLOW]);
    ctr[RT_LBC_OVERFLOW] = 0;
    listed[prim].reserve(c);
    for (uint64_t k = 0; k < c && k < at; k++) {
      const uint32_t cell = (uint32_t)(keys[k] >> 32);
      const float key = unorder((uint32_t)keys[k]);
      CHECK(cell < ncell, "prim %u entry %llu: cell %u of %llu", prim, (unsigned long long)k, cell,
            (unsigned long long)ncell);
      CHECK(key == key, "prim %u entry %llu: NaN key", prim, (unsigned long long)k);
      CHECK(vals[k] == prim, "prim %u entry %llu: prim slot %u", prim, (unsigned long long)k, vals[k]);
      listed[prim].push_back(Entry{cell, key});
    }
    std::sort(listed[prim].begin(), listed[prim].end(),
              [](const Entry& a, const Entry& b) { return a.cell != b.cell ? a.cell < b.cell : a.key < b.key; });
    entries += c;
    max_count = std::max<unsigned long long>(max_count, c);
  }

  // ---- 2. the survey's totals
  unsigned long long sv[RT_LBS_WORDS];
  const int sr_ = rt_lightbuf_survey_host(&lp, 1, sv, err, sizeof err);
  CHECK(sr_ == 0, "rt_lightbuf_survey_host: %d %s", sr_, err);
  CHECK(sv[RT_LBS_ENTRIES] == entries && sv[RT_LBS_NEVER] == n_never && sv[RT_LBS_GLOBAL] == n_global &&
            sv[RT_LBS_BAND] == n_band && sv[RT_LBS_BIG] == n_big && sv[RT_LBS_BAND_ENTRIES] == band_entries &&
            sv[RT_LBS_MAX_COUNT] == max_count && sv[RT_LBS_PRIMS] == nprim,
        "survey %llu %llu %llu %llu %llu %llu %llu, here %llu %llu %llu %llu %llu %llu %llu", sv[RT_LBS_ENTRIES],
        sv[RT_LBS_NEVER], sv[RT_LBS_GLOBAL], sv[RT_LBS_BAND], sv[RT_LBS_BIG], sv[RT_LBS_BAND_ENTRIES],
        sv[RT_LBS_MAX_COUNT], entries, n_never, n_global, n_band, n_big, band_entries, max_count);

  // ---- 3. soundness: every pair the float test accepts is where the query looks
  // the smallest key of prim j in `cell`; false: not listed there
  auto smallest_key = [&](uint32_t j, uint32_t cell, float& key) {
    const std::vector<Entry>& v = listed[j];
    auto it = std::lower_bound(v.begin(), v.end(), cell, [](const Entry& e, uint32_t c) { return e.cell < c; });
    if (it == v.end() || it->cell != cell) return false;
    key = it->key;
    return true;
  };
  unsigned long long accepted = 0, by_global = 0, by_second = 0, by_first = 0, tight = 0, missed = 0;
  float margin = __builtin_inff();  // the smallest limit - key of a pair found in the first cell
  const rt_vec3 lvv = {lv[0], lv[1], lv[2]};
  for (size_t oi = 0; oi < origins.size(); oi++) {
    const rt_vec3 o = origins[oi];
    // the shade pass's shadow direction (csrc/rt_shading.h:35 shadow_dir):
    // type == 1 ? scale(lv, -1.0f) : sub(lv, P)
    const rt_vec3 d = type == 1 ? rt_vec3{lv[0] * -1.0f, lv[1] * -1.0f, lv[2] * -1.0f}
                                : rt_vec3{lvv.x - o.x, lvv.y - o.y, lvv.z - o.z};
    CHECK(o.x >= lb.olo[0] && o.x <= lb.ohi[0] && o.y >= lb.olo[1] && o.y <= lb.ohi[1] && o.z >= lb.olo[2] &&
              o.z <= lb.ohi[2],
          "origin %zu outside the origin box", oi);
    uint32_t cell[2] = {0xffffffffu, 0xffffffffu};
    float lim = __builtin_inff();
    lbuf_cells(lb, o, d, cell, lim);
    CHECK((cell[0] == 0xffffffffu || cell[0] < ncell) && (cell[1] == 0xffffffffu || cell[1] < ncell),
          "origin %zu: cells %u %u of %llu", oi, cell[0], cell[1], (unsigned long long)ncell);
    for (uint32_t j = 0; j < nprim; j++) {
      float t, u, v;
      if (!mt_exact(o, d, (const float*)&tri[3 * (size_t)j], &t, &u, &v)) continue;
      accepted++;
      float key = 0.0f;
      bool found = false;
      if (is_global[j]) {
        by_global++;
        found = true;
      } else if (!is_never[j]) {
        if (cell[0] != 0xffffffffu && smallest_key(j, cell[0], key) && key <= lim) {
          by_first++;
          tight += key >= std::nextafterf(lim, -__builtin_inff());
          margin = std::fmin(margin, lim - key);
          found = true;
        } else if (type == 2 && cell[1] != 0xffffffffu && smallest_key(j, cell[1], key)) {
          by_second++;
          found = true;
        }
      }
      if (!found) {
        float k0 = __builtin_nanf("");
        const bool in0 = !is_never[j] && cell[0] != 0xffffffffu && smallest_key(j, cell[0], k0);
        if (missed < 5)
          std::printf("MISSED %s %s x%u: triangle %u%s, ray of triangle %zu origin (%.9g, %.9g, %.9g), cells %u %u, "
                      "%s key %.9g, limit %.9g, t %.9g u %.9g v %.9g\n",
                      type == 1 ? "dir" : "point", proven ? "proven" : "slack", cell_mul, j,
                      is_never[j] ? " (never)" : "", oi / kRaysPerTri, (double)o.x, (double)o.y, (double)o.z, cell[0],
                      cell[1], in0 ? "listed in the first cell with" : "not in the first cell,", (double)k0, (double)lim,
                      (double)t, (double)u, (double)v);
        missed++;
      }
    }
  }
  CHECK(missed == 0, "%llu accepted pairs are not where the query looks", missed);

  if (row) std::printf("%s %s | ", g_tag, row->name);
  std::printf("%s %s x%u: cells %llu entries %llu | accepted pairs %llu: global %llu, first cell %llu (%llu within a "
              "float step of the limit, nearest %.3g), second cell %llu | global %llu never %llu band %llu big %llu\n",
              type == 1 ? "dir" : "point", proven ? "proven" : "slack", cell_mul, (unsigned long long)ncell, entries,
              accepted, by_global, by_first, tight, (double)margin, by_second, n_global, n_never, n_band, n_big);
  // ---- 4. not vacuous
  if (row) {  // per row
    if (row->gives == kShadows) {
      CHECK(accepted >= 1000, "%s: %llu accepted pairs", row->name, accepted);
      CHECK(by_first + by_second >= 50, "%s: %llu + %llu pairs found through a cell", row->name, by_first, by_second);
    } else {
      CHECK(accepted == 0, "%s: %llu accepted pairs where the reference accepts none", row->name, accepted);
      // |a| <= |d| |e1 x e2| stays below 1e-7 for every triangle of the box
      if (proven && type == 1 && p.dlen < 1e-15)
        CHECK(n_never == nprim, "%s: %llu of %u triangles never", row->name, n_never, nprim);
    }
    return;
  }
  CHECK(accepted >= 1000, "%llu accepted pairs", accepted);
  if (proven && type == 1) CHECK(n_never >= 1, "no triangle is never accepted");
  if (proven && type == 2) CHECK(n_band >= 1, "no band triangle");
  CHECK(n_big >= 1, "no footprint of more than %u cells", kSmallCells);
  if (type == 2) CHECK(by_second >= 1, "no pair found through the second cell");
}

int main() {
  const std::vector<float4> tri = make_triangles(400);
  const uint32_t nprim = (uint32_t)(tri.size() / 3);
  // the triangles' box and the scene's centre and half extent, as rt_ctx.h scene_extent has them
  float sc[3], sr = 0.0f, blo[3], bhi[3];
  for (int a = 0; a < 3; a++) {
    float lo = 1e30f, hi = -1e30f;
    for (uint32_t i = 0; i < nprim; i++) {
      const float* r = (const float*)&tri[3 * (size_t)i];
      const float c[3] = {r[a], r[a] + r[3 + a], r[a] + r[6 + a]};
      for (float x : c) {
        lo = std::fmin(lo, x);
        hi = std::fmax(hi, x);
      }
    }
    blo[a] = lo;
    bhi[a] = hi;
    sc[a] = 0.5f * (lo + hi);
    sr = std::fmax(sr, 0.5f * (hi - lo));
  }
  // hit points: eight per triangle, (float)(v0 + u e1 + v e2)
  std::vector<rt_vec3> origins;
  Lcg g{0xA11CEull};
  for (uint32_t i = 0; i < nprim; i++) {
    const float* r = (const float*)&tri[3 * (size_t)i];
    for (int k = 0; k < kRaysPerTri; k++) {
      double u = g.uni(), v = g.uni();
      if (u + v > 1.0) {
        u = 1.0 - u;
        v = 1.0 - v;
      }
      origins.push_back(rt_vec3{(float)((double)r[0] + u * (double)r[3] + v * (double)r[6]),
                                (float)((double)r[1] + u * (double)r[4] + v * (double)r[7]),
                                (float)((double)r[2] + u * (double)r[5] + v * (double)r[8])});
    }
  }
  for (uint32_t type = 1; type <= 2; type++)
    for (int proven = 0; proven <= 1; proven++)
      for (uint32_t mul : {1u, 16u}) run(tri, origins, sc, sr, blo, bhi, type, type == 1 ? kDirLight : kPointLight, proven, mul);
  // ---- the light table: the same origins and the box's integer lattice (11^3 points, 4 apart)
  std::vector<rt_vec3> more = origins;
  for (int i = -5; i <= 5; i++)
    for (int j = -5; j <= 5; j++)
      for (int k = -5; k <= 5; k++) more.push_back(rt_vec3{4.0f * i, 4.0f * j, 4.0f * k});
  for (const Row& r : kRows) {
    std::printf("row %s | v = %.9g %.9g %.9g\n", r.name, (double)r.v[0], (double)r.v[1], (double)r.v[2]);
    for (int proven = 0; proven <= 1; proven++)
      for (uint32_t mul : {1u, 16u}) run(tri, more, sc, sr, blo, bhi, r.type, r.v, proven, mul, &r);
  }
  // ---- the point lights on the lattice over triangles on the lattice: the faces of the box
  // [-20, 20]^3 in squares of 4, the diagonals alternating (1,200 triangles), and the lattice origins
  // alone.  Edges and vertices lie exactly in the cube map's face boundaries |x| == |y| and on the
  // origins themselves, which the generated triangles above never do.
  {
    std::vector<float4> lat;
    for (int a = 0; a < 3; a++)
      for (int side = -1; side <= 1; side += 2)
        for (int i = 0; i < 10; i++)
          for (int j = 0; j < 10; j++) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            double q[4][3];
            for (int k = 0; k < 4; k++) {
              q[k][a] = 20.0 * side;
              q[k][b] = -20.0 + 4.0 * (i + (k == 1 || k == 2));
              q[k][c] = -20.0 + 4.0 * (j + (k >= 2));
            }
            const int t[2][2][3] = {{{0, 1, 2}, {0, 2, 3}}, {{0, 1, 3}, {1, 2, 3}}};
            for (int h = 0; h < 2; h++) {
              const int* w = t[(i + j) & 1][h];
              double e1[3], e2[3];
              for (int k = 0; k < 3; k++) {
                e1[k] = q[w[1]][k] - q[w[0]][k];
                e2[k] = q[w[2]][k] - q[w[0]][k];
              }
              push(lat, q[w[0]], e1, e2);
            }
          }
    const float c0[3] = {0.0f, 0.0f, 0.0f}, lo[3] = {-20.0f, -20.0f, -20.0f}, hi[3] = {20.0f, 20.0f, 20.0f};
    const std::vector<rt_vec3> lattice(more.begin() + (long)origins.size(), more.end());
    g_tag = "lattice row";
    for (const Row& r : kRows)
      if (r.lattice)
        for (int proven = 0; proven <= 1; proven++)
          for (uint32_t mul : {1u, 16u}) run(lat, lattice, c0, 20.0f, lo, hi, r.type, r.v, proven, mul, &r);
    g_tag = "row";
  }
  // ---- non-finite vectors: refused before any grid or cell is derived from them
  {
    const float bad[3] = {__builtin_inff(), -__builtin_inff(), __builtin_nanf("")};
    unsigned refused = 0;
    for (uint32_t type = 1; type <= 2; type++)
      for (int a = 0; a < 3; a++)
        for (float b : bad)
          for (int proven = 0; proven <= 1; proven++) {
            float lv[3] = {type == 1 ? kDirLight[0] : kPointLight[0], type == 1 ? kDirLight[1] : kPointLight[1],
                           type == 1 ? kDirLight[2] : kPointLight[2]};
            lv[a] = b;
            char err[256] = {0};
            LBParams lp;
            lb_fill(lp, sc, sr, blo, bhi, 64.0f, type, lv, nprim, proven);
            lp.tri = tri.data();
            HostBP p{};
            RtLightBuf lb;
            uint64_t ncell = 0;
            const int gr = lb_geom_host(&lp, p, &lb, ncell, err, sizeof err);
            CHECK(gr == 1 && std::strcmp(err, "light with a non-finite vector") == 0 && lb.kind == RT_LB_NONE,
                  "type %u component %d = %g: lb_geom_host %d '%s' kind %u", type, a, (double)b, gr, err, lb.kind);
            unsigned long long sv[RT_LBS_WORDS];
            CHECK(rt_lightbuf_survey_host(&lp, 1, sv, err, sizeof err) == -1, "the survey of a non-finite light");
            refused += gr == 1;
          }
    std::printf("non-finite vectors: %u of 36 refused\n", refused);
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("lightbuf geom ok\n");
  return 0;
}
