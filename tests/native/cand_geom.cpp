// cand_geom.cpp -- the proof geometry of the camera rays' candidate lists
// (csrc/rt_cand_geom.h) and its frame constants (csrc/rt_cand_host.cpp
// cand_params) on the CPU (tests/test_cand_geom.py builds it plain and with
// g++ -fsanitize=address,undefined; no GPU, no librtgpu.so).
//
// A deterministic set of triangles (integer LCG, no file input) in front of
// the synthetic scenes' camera (host/synth.c): small ones facing the eye,
// slivers, triangles whose plane passes within 1e-3 of the eye (some holding
// the eye's foot point: unbounded footprints) and a few of those large enough
// to cross the whole frame.  For every frame below, every rank split and
// every rank:
//   * the tiles raster() emits, raster_count() and the sum of row_ivs()'s
//     interval counts agree (rt_cand_survey_host returns -1 otherwise: the
//     device sizes its buffers from the counts and fills them from the
//     raster), and every emitted rank-local tile is below ntiles_local;
//   * the tiles emitted over the ranks of a split, mapped back by rt_tile_xy,
//     are the one-rank frame's tiles, each once (the multi-GPU exchange
//     routes whole-frame entries by that map);
//   * quick_class == Q_SAFE implies classify == SAFE without a leaf box
//     (survey slot 80), and Q_AWAY a footprint without a tile of the rank;
//   * tile_keep(p, rec, tx, ty) equals tile_keep(TileFrame, TileTri, tx, ty)
//     and is the same for the same (tx, ty) under every rank split;
//   * the set is not vacuous: all three classes, a footprint of more than
//     kSmallEntries tiles, an entry tile_keep drops and one it keeps.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_cand_geom.h"
#include "rt_hip.h"

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
  double uni() { return next() * (1.0 / 4294967296.0); }     // [0, 1)
  double sym() { return 2.0 * uni() - 1.0; }                 // [-1, 1)
  double log_between(double a, double b) { return a * std::pow(b / a, uni()); }
};

static const double kEye[3] = {0.0, 4.0, -20.0};  // host/synth.c: camera W H 0 4 -20 1 0 0 0 -1 0 70

static void unit(double* v) {
  const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  for (int a = 0; a < 3; a++) v[a] /= l;
}

static void random_dir(Lcg& g, double* v) {
  do {
    for (int a = 0; a < 3; a++) v[a] = g.sym();
  } while (v[0] * v[0] + v[1] * v[1] + v[2] * v[2] < 0.01);
  unit(v);
}

static void push(std::vector<float>& tri, const double* v0, const double* e1, const double* e2) {
  for (int a = 0; a < 3; a++) tri.push_back((float)v0[a]);
  for (int a = 0; a < 3; a++) tri.push_back((float)e1[a]);
  for (int a = 0; a < 3; a++) tri.push_back((float)e2[a]);
  for (int a = 0; a < 3; a++) tri.push_back(0.0f);  // the record's words (prim, object, flags)
}

// a point of the view cone at depth d in front of the eye (the camera looks along +z)
static void cone_point(Lcg& g, double d, double* x) {
  x[0] = kEye[0] + 0.8 * d * g.sym();
  x[1] = kEye[1] + 0.5 * d * g.sym();
  x[2] = kEye[2] + d;
}

// A triangle in a plane at distance delta from the eye, spanned by a forward
// direction a inside the view cone and a second direction b: its first
// corner s along a and t along b from the eye's foot point, sides of about
// `size`.  hold_eye: the foot point lies inside the triangle.
static void grazing(Lcg& g, std::vector<float>& tri, double delta, double size, bool hold_eye) {
  double a[3] = {0.6 * g.sym(), 0.35 * g.sym(), 1.0}, b[3], n[3];
  unit(a);
  do {
    random_dir(g, b);
    const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    for (int k = 0; k < 3; k++) b[k] -= ab * a[k];
  } while (b[0] * b[0] + b[1] * b[1] + b[2] * b[2] < 0.04);
  unit(b);
  n[0] = a[1] * b[2] - a[2] * b[1];
  n[1] = a[2] * b[0] - a[0] * b[2];
  n[2] = a[0] * b[1] - a[1] * b[0];
  double s = hold_eye ? -0.5 : g.log_between(0.5, 40.0), t = hold_eye ? -0.5 : 2.0 * g.sym();
  double v0[3], e1[3], e2[3];
  const double th1 = hold_eye ? 0.0 : 6.283185307179586 * g.uni(), th2 = th1 + (hold_eye ? 1.5707963267948966 : 0.3 + 2.5 * g.uni());
  const double l1 = hold_eye ? 3.0 : size * (0.5 + g.uni()), l2 = hold_eye ? 3.0 : size * (0.5 + g.uni());
  for (int k = 0; k < 3; k++) {
    v0[k] = kEye[k] + delta * n[k] + s * a[k] + t * b[k];
    e1[k] = l1 * (std::cos(th1) * a[k] + std::sin(th1) * b[k]);
    e2[k] = l2 * (std::cos(th2) * a[k] + std::sin(th2) * b[k]);
  }
  push(tri, v0, e1, e2);
}

static std::vector<float> make_triangles(int n) {
  std::vector<float> tri;
  Lcg g{0x5EEDull};
  for (int i = 0; i < n; i++) {
    const uint32_t kind = g.next() % 100u;
    double v0[3], e1[3], e2[3];
    if (kind < 45) {  // small, anywhere in (and a little around) the view cone
      cone_point(g, g.log_between(3.0, 80.0), v0);
      random_dir(g, e1);
      random_dir(g, e2);
      const double l1 = g.log_between(0.02, 0.4), l2 = g.log_between(0.02, 0.4);
      for (int a = 0; a < 3; a++) {
        e1[a] *= l1;
        e2[a] *= l2;
      }
      push(tri, v0, e1, e2);
    } else if (kind < 60) {  // slivers: a long side and a very short one
      cone_point(g, g.log_between(3.0, 80.0), v0);
      random_dir(g, e1);
      random_dir(g, e2);
      const double l1 = g.log_between(1.0, 30.0), l2 = g.log_between(1e-4, 1e-2);
      for (int a = 0; a < 3; a++) {
        e1[a] *= l1;
        e2[a] *= l2;
      }
      push(tri, v0, e1, e2);
    } else if (kind < 92) {  // grazing: the plane within 1e-3 of the eye
      grazing(g, tri, 1e-3 * g.sym(), g.log_between(0.03, 3.0), false);
    } else if (kind < 97) {  // grazing and holding the eye's foot point: unbounded
      grazing(g, tri, 3e-5 * g.sym(), 0.0, true);
    } else {  // grazing and large: across the whole frame
      grazing(g, tri, 1e-3 * g.sym(), g.log_between(100.0, 400.0), false);
    }
  }
  return tri;
}

// The frame of the synthetic camera (host/vecmath.c rt_frame_from_camera_any
// for u = (1, 0, 0), v = (0, -1, 0), fov 70: w = u x v = (0, 0, -1), C = pos +
// w L, L = (float)(W / (2 tan 35 deg)))
static rt_frame make_frame(int W, int H) {
  rt_frame f;
  const float L = (float)(W / 1.4004150764194193);
  f.u = rt_vec3{1.0f, 0.0f, 0.0f};
  f.v = rt_vec3{0.0f, -1.0f, 0.0f};
  f.position = rt_vec3{(float)kEye[0], (float)kEye[1], (float)kEye[2]};
  f.C = rt_vec3{f.position.x, f.position.y, f.position.z + -1.0f * L};
  f.width = W;
  f.height = H;
  return f;
}

struct FrameCase {
  int W, H, compat;
};

int main() {
  const int kTriangles = 1000;
  const std::vector<float> tri = make_triangles(kTriangles);
  const uint32_t nprim = (uint32_t)(tri.size() / 12);
  // the scene's centre and half extent, as rt_ctx.h scene_extent has them
  float sc[3], sr = 0.0f;
  for (int a = 0; a < 3; a++) {
    float lo = 1e30f, hi = -1e30f;
    for (uint32_t i = 0; i < nprim; i++) {
      const float* r = &tri[12 * (size_t)i];
      const float c[3] = {r[a], r[a] + r[3 + a], r[a] + r[6 + a]};
      for (float x : c) {
        lo = std::fmin(lo, x);
        hi = std::fmax(hi, x);
      }
    }
    sc[a] = 0.5f * (lo + hi);
    sr = std::fmax(sr, 0.5f * (hi - lo));
  }
  const FrameCase frames[] = {{64, 40, 0}, {474, 266, 0}, {266, 476, 0}, {474, 270, 1}};
  const int splits[] = {1, 2, 3, 8};
  for (const FrameCase& fc : frames) {
    const rt_frame f = make_frame(fc.W, fc.H);
    std::vector<CandParams> ps;  // [0]: the one-rank frame; then every rank of every split
    for (int n : splits)
      for (int r = 0; r < n; r++) {
        CandParams p;
        const int rc = cand_params(&f, sc, sr, 64.0f, 1.0, r, n, &p, fc.compat);
        CHECK(rc == RT_OK, "cand_params %dx%d rank %d of %d: %d", fc.W, fc.H, r, n, rc);
        p.nprim = nprim;
        ps.push_back(p);
      }
    if (failures) break;
    const int tiles_x = ps[0].tiles_x, tiles_y = ps[0].tiles_y;
    CHECK(tiles_x == (fc.W + 7) / 8 && tiles_y == (fc.H + 7) / 8 && ps[0].ntiles_local == tiles_x * tiles_y,
          "%dx%d: %d x %d tiles, %d local", fc.W, fc.H, tiles_x, tiles_y, ps[0].ntiles_local);
    const size_t ntiles = (size_t)tiles_x * (size_t)tiles_y;
    std::vector<signed char> ref(ntiles);  // the one-rank frame's entries of a triangle: -1 none, else tile_keep
    std::vector<int> seen(ntiles);         // times a split's ranks emitted the tile
    unsigned long long cls[3] = {0, 0, 0}, entries = 0, big = 0, kept = 0, dropped = 0, q_safe = 0, q_away = 0;
    for (uint32_t i = 0; i < nprim; i++) {
      const float* rec = &tri[12 * (size_t)i];
      std::fill(ref.begin(), ref.end(), (signed char)-1);
      int c0 = -1;
      size_t q = 0;
      for (int n : splits) {
        std::fill(seen.begin(), seen.end(), 0);
        for (int r = 0; r < n; r++, q++) {
          const CandParams& p = ps[q];
          rtc::Footprint fp;
          const int c = rtc::classify(p, rec, nullptr, fp);
          if (q == 0) {
            c0 = c;
            cls[c]++;
          }
          CHECK(c == c0, "prim %u: class %d at rank %d of %d, %d on one rank", i, c, r, n, c0);
          const int qc = rtc::quick_class(p, rec);
          if (q == 0) q_safe += qc == rtc::Q_SAFE;
          q_away += qc == rtc::Q_AWAY;
          // the fast path's proof must hold (rt_cand_survey_host [80]) ...
          CHECK(qc != rtc::Q_SAFE || c == rtc::SAFE, "prim %u: Q_SAFE but class %d (rank %d of %d)", i, c, r, n);
          // ... and the rank filter never drops a prim with a tile here (rt_cand_verify_host [5])
          CHECK(qc != rtc::Q_AWAY || c == rtc::SAFE || (c == rtc::FOOTPRINT && rtc::raster_count(p, fp) == 0),
                "prim %u: Q_AWAY but class %d with %u tiles (rank %d of %d)", i, c,
                c == rtc::FOOTPRINT ? rtc::raster_count(p, fp) : 0u, r, n);
          if (c != rtc::FOOTPRINT) continue;
          rtc::TileFrame tf;
          rtc::TileTri tt;
          rtc::tile_frame(p, tf);
          const bool tt_ok = rtc::tile_tri(p, rec, tt);
          unsigned long long v = 0;
          rtc::raster(p, fp, [&](uint32_t tl) {
            v++;
            CHECK(tl < (uint32_t)p.ntiles_local, "prim %u: local tile %u of %d (rank %d of %d)", i, tl, p.ntiles_local, r,
                  n);
            int tx = -1, ty = -1;
            rt_tile_xy(tl, (uint32_t)p.rank, (uint32_t)p.nranks, (uint32_t)p.blocks_x, (uint32_t)p.tb, &tx, &ty);
            CHECK(tx >= 0 && tx < tiles_x && ty >= 0 && ty < tiles_y, "prim %u: tile (%d, %d) off the %d x %d frame", i,
                  tx, ty, tiles_x, tiles_y);
            if (!(tx >= 0 && tx < tiles_x && ty >= 0 && ty < tiles_y)) return;
            const size_t g = (size_t)ty * (size_t)tiles_x + (size_t)tx;
            const bool keep = rtc::tile_keep(p, rec, tx, ty);
            const bool keep2 = !tt_ok || rtc::tile_keep(tf, tt, tx, ty);
            CHECK(keep == keep2, "prim %u tile (%d, %d): tile_keep %d, by parts %d", i, tx, ty, (int)keep, (int)keep2);
            if (q == 0) {
              ref[g] = keep ? 1 : 0;
              (keep ? kept : dropped)++;
            } else {
              CHECK(ref[g] == (keep ? 1 : 0), "prim %u tile (%d, %d): tile_keep %d at rank %d of %d, %d on one rank", i,
                    tx, ty, (int)keep, r, n, (int)ref[g]);
            }
            seen[g]++;
          });
          unsigned long long vi = 0;
          int r0, r1;
          if (rtc::raster_rows(p, fp, r0, r1))
            for (int ty = r0 >> 3; ty <= (r1 >> 3); ty++) {
              int x[6], fb[3];
              uint32_t cn[3];
              rtc::row_ivs(p, fp, ty, r0, r1, x, fb, cn);
              vi += cn[0] + cn[1] + cn[2];
            }
          const unsigned long long rcount = rtc::raster_count(p, fp);
          CHECK(v == rcount && v == vi, "prim %u rank %d of %d: raster %llu, raster_count %llu, row_ivs %llu", i, r, n, v,
                rcount, vi);
          if (q == 0) {
            entries += v;
            big += v > rtc::kSmallEntries;
          }
        }
        // the split's ranks partition the one-rank frame's tiles
        for (size_t g = 0; g < ntiles; g++)
          CHECK(seen[g] == (ref[g] >= 0 ? 1 : 0), "prim %u tile (%zu, %zu): emitted %d times by the %d ranks, %d on one", i,
                g % (size_t)tiles_x, g / (size_t)tiles_x, seen[g], n, ref[g] >= 0 ? 1 : 0);
      }
      if (failures) break;
    }
    std::printf("%dx%d%s: safe %llu footprint %llu global %llu | entries %llu, footprints over %u tiles %llu | "
                "tile_keep kept %llu dropped %llu | Q_SAFE %llu, Q_AWAY (all ranks) %llu\n",
                fc.W, fc.H, fc.compat ? " compat" : "", cls[rtc::SAFE], cls[rtc::FOOTPRINT], cls[rtc::GLOBAL], entries,
                rtc::kSmallEntries, big, kept, dropped, q_safe, q_away);
    // not vacuous
    CHECK(cls[rtc::SAFE] > 0 && cls[rtc::FOOTPRINT] > 0 && cls[rtc::GLOBAL] > 0, "a class is empty");
    CHECK(big > 0, "no footprint of more than %u tiles", rtc::kSmallEntries);
    CHECK(kept > 0 && dropped > 0, "tile_keep kept %llu, dropped %llu", kept, dropped);
    if (failures) break;
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("cand geom ok\n");
  return 0;
}
