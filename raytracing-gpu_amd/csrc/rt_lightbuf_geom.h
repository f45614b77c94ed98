// rt_lightbuf_geom.h -- the footprint geometry of the light buffers
// (rt_lightbuf.h, DESIGN.md §4 "Light buffers"): the error-bound constants,
// the build's geometry parameters (LbGeom), a triangle's footprint in a
// light's grid (Foot, footprint), the cells and keys of its rows (foot_rows,
// row_entries, cell_key, cell_overlaps, band_row), the size classes (foot_cells,
// foot_is_big) and the nearest shadow-ray origin (prim_rmin).  Double
// arithmetic, all of it __host__ __device__: no kernel, no thread index, no
// memory but its arguments.  The device build (rt_lightbuf.hip) and the host
// survey (rt_lightbuf_host.cpp) run this same code; a plain C++ compiler
// builds it too (tests/native/lightbuf_geom.cpp, -D__HIP_PLATFORM_AMD__ for
// the HIP headers' types).  The query's half of the contract -- the cells and
// the key limit a shadow ray looks up -- is rt_lightbuf_cell.h.
//
// Two ways to grow a triangle's footprint (LBParams::proven):
//
// * slack (default): a triangle is listed in every cell that a shadow ray
//   passing within the walk's slack of it can start from (the float rounding
//   of the query's own cell and key computations added as margins), and
//   skipped by a query only where it lies entirely behind the ray's origin by
//   more than twice that slack.  The walk tests a triangle when the ray
//   passes within the slack of the leaf box holding it, so both find every
//   hit within the slack of a triangle -- the same exactness class ("tested,
//   not proven", DESIGN.md §2 "Shadow rays").
//
// * proven: listed wherever a shadow ray of this light can make the
//   reference's float Moller-Trumbore test (cpu/hit.c:15-33) accept the
//   triangle.  tools/mt_bound.py bounds the float test: an accept implies the
//   exact line crosses the triangle's plane inside the expanded triangle
//     T_D = { v0 + U e1 + V e2 : U >= -du, V >= -dv, U + V <= 1 + dw },
//   du, dv, dw from the rounding errors E_sh, E_dq, E_a of s.h, d.q, a and a
//   lower bound a_lb of the float |a| (>= 1e-7 for any accept).
//   - A directional light's rays all have the direction d = -l.v exactly
//     (cpu/light.c:53): the exact a = -d.n is one number per triangle, so
//     a_lb = max(1e-7, |a| - E_a) and T_D are fixed (|S| = |o - v0| bounded
//     over the origin box, componentwise).  T_D's projection along the light
//     is the footprint; the crossing X has the origin's projection, and lies
//     at most derr = |d| E_eq / |a| behind it.  No ray accepts a triangle with
//     |a| + E_a < 1e-7: such triangles are listed nowhere.
//   - A point light's rays (P, l.v - P) (cpu/light.c:78) pass within dline of
//     the light.  A ray crossing the plane at X has cosine c >= (s_L - dline)
//     / (|X - l.v| + dline) with the plane (s_L = the light's distance from
//     it), and the bound at cosine c moves X at most h(c) from the triangle;
//     so X lies within r of it only if r <= g(r) = h(c(r)).  g is convex and
//     increasing, and the smallest R with g(R) <= R (iterated from 0) bounds
//     every crossing of rays at c >= c*, provided h(c*) < r(c*) (the r at
//     which c(r) = c*).  Rays at c < c* are accepted only from origins within
//     H_o(c*) of the plane, on lines nearly parallel to it (|s_o| bounded by
//     u, v in [0, 1] and |a_f| <= |a| + E_a), which needs s_L <= H_o(c*) +
//     Dmax c* + dline: for larger s_L there are none.  Triangles whose plane
//     passes that close to the light are listed, in addition, in the band of
//     cube-map cells within asin(c* + dline / rmin_o) of the great circle of
//     the plane through the light parallel to theirs (with the key that is
//     always tested).  The cone of directions to T's ball grown by R is the
//     footprint; keys as in slack mode with derr in place of the slack.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "rt_counters.h"
#include "rt_lightbuf.h"

namespace rtl {

#define RTL_FN __host__ __device__

constexpr double kEps = 0x1p-24;
constexpr double kInvSqrt3 = 0.57735026918962573;
constexpr double kSqrt3 = 1.7320508075688772;
constexpr double kAMin = 9.99999997e-08;   // (double)(float)1e-7, cpu/hit.c:7
constexpr double kCDot = 8.6, kCA = 7.2;   // tools/mt_bound.py C_DOT, C_A (Cauchy-Schwarz)
constexpr double kCW = 6.01, kCWA = 5.01;  // tools/mt_bound.py bound_cw (componentwise)
constexpr double kDMax = 1.0 + 4.0 * kEps;
constexpr uint32_t kSmallCells = 1024;  // more (or a band): counted and emitted by a workgroup
constexpr int kMaxRects = 6;

// The geometry of one light's build (lb_derive_grid, rt_lightbuf_host.cpp):
// the first members of the kernels' parameter (rtl::BP, rt_lightbuf.hip).
struct LbGeom {
  const float4* tri;
  uint32_t nprim, kind, proven;
  double lv[3];
  double u[3], v[3], w[3];  // DIR: the float axes, as doubles
  double u0, v0, cs, inv_cs;
  uint32_t nx, ny, n;       // DIR grid / POINT face side
  double slack, s1, dmax;
  double olo[3], ohi[3];    // the origin box (LBParams::box_lo/hi)
  double d[3], dlen;        // DIR: the rays' direction -l.v (float) and its length
  double skew;              // DIR: max |u.d^|, |v.d^| (the float axes vs the exact direction)
  double rmin_o;             // POINT proven: a lower bound of |o - l.v| over shadow-ray origins
};

struct Foot {
  int n;  // rects
  uint32_t face[kMaxRects];
  int x0[kMaxRects], x1[kMaxRects], y0[kMaxRects], y1[kMaxRects];
  double key;    // whole-triangle key (ascending = tested first)
  bool global;
  bool never;    // proven: no ray of the light can make the float test accept it
  // DIR per-cell refinement: the plane's depth over a cell column
  bool plane;
  double pn_u, pn_v, pn_w, pn_d;  // n.u, n.v, n.w, n.v0 of the triangle's plane
  double m;                       // footprint margin (world units)
  double kpad;                    // behind-origin tolerance of the keys (2 slack; proven: derr)
  // per rect: the triangle's image in the rect's coordinates (DIR: u, v;
  // POINT: the face's (s, t)) and its margin there, for the cell overlap
  // test of small footprints; tri_ok = 0: bounding rect only
  bool tri_ok[kMaxRects];
  double tx[kMaxRects][3], ty[kMaxRects][3], tm[kMaxRects];
  // POINT proven: also every cell whose directions x can have |x.bn| <= bB
  // |x|_inf-scaled (the band around the great circle of the plane through
  // the light parallel to the triangle)
  bool band;
  double bn[3], bB;
};

RTL_FN inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
RTL_FN inline double norm3(const double* a) { return sqrt(dot3(a, a)); }
RTL_FN inline void cross3d(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// float <-> bits, and a double rounded toward minus infinity to float: the
// device's intrinsics, and their plain C++ equals on the host
RTL_FN inline uint32_t float_bits(float f) {
#ifdef __HIP_DEVICE_COMPILE__
  return __float_as_uint(f);
#else
  uint32_t b;
  memcpy(&b, &f, sizeof b);
  return b;
#endif
}
RTL_FN inline float bits_float(uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __uint_as_float(b);
#else
  float f;
  memcpy(&f, &b, sizeof f);
  return f;
#endif
}
RTL_FN inline float float_rd(double x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __double2float_rd(x);
#else
  const float r = (float)x;
  return (double)r > x ? nextafterf(r, -__builtin_inff()) : r;
#endif
}

RTL_FN inline uint32_t orderable(float f) {
  const uint32_t b = float_bits(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
RTL_FN inline float unorder(uint32_t b) {
  return bits_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

RTL_FN inline int clampi(double x, int hi) {
  if (!(x > 0.0)) return 0;  // NaN -> 0
  if (x >= (double)hi) return hi;
  return (int)x;
}

RTL_FN inline void foot_init(Foot& f) {
  f.n = 0;
  f.global = false;
  f.never = false;
  f.plane = false;
  f.band = false;
  f.kpad = 0.0;
  f.m = 0.0;
  for (int q = 0; q < kMaxRects; q++) f.tri_ok[q] = false;
}

// DIR: rect and image of the points P[0..2] (the triangle, or T_D) projected
// on (u, v) with margin m; the plane of the triangle for the per-cell keys
RTL_FN inline void dir_rect(const LbGeom& p, const double P[3][3], const double* v0, const double* e1,
                                const double* e2, double m, Foot& f, double& hw) {
  double lu = 1e300, hu = -1e300, lvv = 1e300, hvv = -1e300;
  hw = -1e300;
  for (int k = 0; k < 3; k++) {
    const double a = dot3(P[k], p.u), b = dot3(P[k], p.v), c = dot3(P[k], p.w);
    lu = fmin(lu, a);
    hu = fmax(hu, a);
    lvv = fmin(lvv, b);
    hvv = fmax(hvv, b);
    hw = fmax(hw, c);
    f.tx[0][k] = a;
    f.ty[0][k] = b;
  }
  f.tri_ok[0] = true;
  f.tm[0] = m;
  f.n = 1;
  f.face[0] = 0;
  f.x0[0] = clampi(floor((lu - m - p.u0) * p.inv_cs - 0.01), (int)p.nx - 1);
  f.x1[0] = clampi(floor((hu + m - p.u0) * p.inv_cs + 0.01), (int)p.nx - 1);
  f.y0[0] = clampi(floor((lvv - m - p.v0) * p.inv_cs - 0.01), (int)p.ny - 1);
  f.y1[0] = clampi(floor((hvv + m - p.v0) * p.inv_cs + 0.01), (int)p.ny - 1);
  f.m = m;
  double n[3];
  cross3d(e1, e2, n);
  const double nl = norm3(n);
  f.pn_u = dot3(n, p.u);
  f.pn_v = dot3(n, p.v);
  f.pn_w = dot3(n, p.w);
  f.pn_d = dot3(n, v0);
  f.plane = nl > 0.0 && fabs(f.pn_w) > 0.05 * nl;
}

// POINT: the cube-map rects of the cone from the light around the ball
// (C, rb), widened by alpha, and the central projection of V grown by beta
// for the overlap test.  false: the cone is too wide (global list).
RTL_FN inline bool point_cone(const LbGeom& p, const double V[3][3], const double C[3], double rb, double& rmin,
                                  double grow, Foot& f) {
  const double D[3] = {C[0] - p.lv[0], C[1] - p.lv[1], C[2] - p.lv[2]};
  const double dc = norm3(D);
  if (!(dc > rb * 1.001 + 1e-9)) return false;
  rmin = dc - rb;
  const double alpha = 4.0 * kSqrt3 * kEps * p.dmax / rmin + 8.0 * kEps;
  const double th = asin(fmin(1.0, rb / dc)) + alpha + 1e-12;
  if (!(th < 1.2)) return false;
  double xlo[3], xhi[3];
  for (int a = 0; a < 3; a++) {
    const double ph = acos(fmax(-1.0, fmin(1.0, D[a] / dc)));
    xlo[a] = cos(fmin(3.141592653589793, ph + th)) - 1e-12;
    xhi[a] = cos(fmax(0.0, ph - th)) + 1e-12;
  }
  const double hn = 0.5 * (double)p.n;
  for (int a = 0; a < 3; a++)
    for (int sg = 0; sg < 2; sg++) {
      double alo = sg == 0 ? xlo[a] : -xhi[a], ahi = sg == 0 ? xhi[a] : -xlo[a];
      if (ahi < kInvSqrt3 * (1.0 - 1e-9)) continue;  // the cone never reaches this face's frustum
      alo = fmax(alo, kInvSqrt3 * (1.0 - 1e-9));    // directions on the face have |x_a| >= 1/sqrt 3
      const int j = (a + 1) % 3, k = (a + 2) % 3;
      const double slo = fmin(xlo[j] / alo, xlo[j] / ahi), shi = fmax(xhi[j] / alo, xhi[j] / ahi);
      const double tlo = fmin(xlo[k] / alo, xlo[k] / ahi), thi = fmax(xhi[k] / alo, xhi[k] / ahi);
      if (slo > 1.0 + 1e-9 || shi < -1.0 - 1e-9 || tlo > 1.0 + 1e-9 || thi < -1.0 - 1e-9) continue;
      const int q = f.n++;
      f.face[q] = (uint32_t)(2 * a + sg);
      // the triangle's central projection onto the face (valid when every
      // vertex lies well on the face's side), grown by the cone's widening
      // beta (grow / rmin + alpha) through the face map's Lipschitz bound
      {
        const double beta = grow / rmin + alpha;
        const double sgn = sg == 0 ? 1.0 : -1.0;
        double xamin = 1e300, smax = 1.0;
        bool ok = true;
        for (int v = 0; v < 3 && ok; v++) {
          const double X[3] = {V[v][0] - p.lv[0], V[v][1] - p.lv[1], V[v][2] - p.lv[2]};
          const double xl = norm3(X), xa = sgn * X[a];
          ok = xl > 0.0 && xa > 1e-3 * xl;
          if (!ok) break;
          xamin = fmin(xamin, xa / xl);
          f.tx[q][v] = X[j] / xa;
          f.ty[q][v] = X[k] / xa;
          smax = fmax(smax, fmax(fabs(f.tx[q][v]), fabs(f.ty[q][v])));
        }
        if (ok && xamin > 4.0 * beta) {
          f.tri_ok[q] = true;
          f.tm[q] = 2.0 * beta * (1.0 + smax + 2.0 * beta) / (xamin - 2.0 * beta) * 1.01 + 1e-9;
        }
      }
      f.x0[q] = clampi(floor((fmax(slo, -1.0) + 1.0) * hn - 0.01), (int)p.n - 1);
      f.x1[q] = clampi(floor((fmin(shi, 1.0) + 1.0) * hn + 0.01), (int)p.n - 1);
      f.y0[q] = clampi(floor((fmax(tlo, -1.0) + 1.0) * hn - 0.01), (int)p.n - 1);
      f.y1[q] = clampi(floor((fmin(thi, 1.0) + 1.0) * hn + 0.01), (int)p.n - 1);
    }
  return true;
}

// ---- slack-grown footprints (default) ----
RTL_FN inline void footprint_slack(const LbGeom& p, const double V[3][3], const double* v0, const double* e1,
                                const double* e2, Foot& f) {
  if (p.kind == RT_LB_DIR) {
    // the query's float projection of its origin is within 3 eps s1 of the
    // exact one; the triangle's points are within the slack of the ray
    const double m = p.slack + 3.0 * kEps * p.s1 * 1.01 + 1e-9 * p.s1;
    double hw;
    dir_rect(p, V, v0, e1, e2, m, f, hw);
    // skipped by a query when its deepest point, grown by the slack on both
    // sides (behind-origin tolerance of the walk) and the rounding of the
    // query's depth, lies below the origin: key = -(that bound)
    f.kpad = 2.0 * p.slack;
    f.key = -(hw + 2.0 * p.slack + 6.0 * kEps * p.s1 * 1.01 + 1e-9 * p.s1);
    return;
  }
  // POINT: the cone from the light around the triangle's bounding sphere
  // (grown by the slack), widened by the angle the rounding of the shadow
  // direction l.v - P can turn a ray's points as seen from the light
  double C[3];
  for (int a = 0; a < 3; a++) C[a] = (V[0][a] + V[1][a] + V[2][a]) / 3.0;
  double rb = 0.0;
  for (int k = 0; k < 3; k++) {
    const double d[3] = {V[k][0] - C[0], V[k][1] - C[1], V[k][2] - C[2]};
    rb = fmax(rb, norm3(d));
  }
  rb = rb * (1.0 + 1e-12) + p.slack + 1e-12;
  double rmin = 0.0;
  if (!point_cone(p, V, C, rb, rmin, p.slack, f)) {
    f.n = 0;
    f.global = true;
    return;
  }
  // a query toward the light stops once the triangle's nearest possible
  // point lies farther from the light than its origin (plus the slack)
  f.kpad = 2.0 * p.slack;
  f.key = rmin - 2.0 * p.slack - 1e-9 * p.dmax;
}

// ---- proven footprints (module comment) ----
RTL_FN inline void footprint_dir_proven(const LbGeom& p, const double* v0, const double* e1, const double* e2, Foot& f) {
  const double* d = p.d;
  double n[3];
  cross3d(e1, e2, n);
  const double A = fabs(dot3(n, d));  // |a| exact: a = e1.(d x e2) = -d.n, every ray alike
  double M[3], S[3];
  for (int i = 0; i < 3; i++) S[i] = fmax(fabs(p.olo[i] - v0[i]), fabs(p.ohi[i] - v0[i]));
  double Ea = 0.0;
  for (int i = 0; i < 3; i++) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    M[i] = fabs(d[j]) * fabs(e2[k]) + fabs(d[k]) * fabs(e2[j]);
    Ea += fabs(e1[i]) * M[i];
  }
  const double r1 = 1.0 + 1e-6;
  Ea *= kCWA * kEps * r1;
  if (A + Ea < kAMin * (1.0 - 1e-9)) {  // |a_f| < 1e-7 for every ray: rejected (cpu/hit.c:19)
    f.never = true;
    return;
  }
  const double alb = fmax(kAMin, A - Ea);
  const double rho = Ea / alb;
  if (!(rho < 0.5)) {
    f.global = true;
    return;
  }
  const double C[3] = {v0[0] + (e1[0] + e2[0]) / 3.0, v0[1] + (e1[1] + e2[1]) / 3.0, v0[2] + (e1[2] + e2[2]) / 3.0};
  const double ud[3] = {-d[0] / p.dlen, -d[1] / p.dlen, -d[2] / p.dlen};  // from X back toward the origin
  double du = 0.0, dv = 0.0, dw = 0.0, Eeq = 0.0;
  double P[3][3];
  // T_D with |S_i| <= the box bound, then again with the origins' own bound:
  // an accepting ray's origin o = X - t d (t >= 0) lies in the box, X in T_D
  // (every step valid for every accepting ray, so each bound is)
  for (int pass = 0; pass < 3; pass++) {
    double N[3], Esh = 0.0, Edq = 0.0;
    Eeq = 0.0;
    for (int i = 0; i < 3; i++) {
      const int j = (i + 1) % 3, k = (i + 2) % 3;
      N[i] = S[j] * fabs(e1[k]) + S[k] * fabs(e1[j]);
    }
    for (int i = 0; i < 3; i++) {
      Esh += S[i] * M[i];
      Edq += fabs(d[i]) * N[i];
      Eeq += fabs(e2[i]) * N[i];
    }
    Esh *= kCW * kEps * r1;
    Edq *= kCW * kEps * r1;
    Eeq *= kCW * kEps * r1;
    du = Esh / (alb * (1.0 - rho));
    dv = Edq / (alb * (1.0 - rho));
    dw = (4.0 * kEps + (Esh + Edq) / alb + rho) / (1.0 - rho);
    // T_D's corners (U, V) = (-du, -dv), (1 + dw + dv, -dv), (-du, 1 + dw + du)
    const double cU[3] = {-du, 1.0 + dw + dv, -du}, cV[3] = {-dv, -dv, 1.0 + dw + du};
    double rX = 0.0;
    for (int k = 0; k < 3; k++) {
      double w[3];
      for (int a = 0; a < 3; a++) {
        P[k][a] = v0[a] + cU[k] * e1[a] + cV[k] * e2[a];
        w[a] = P[k][a] - C[a];
      }
      rX = fmax(rX, norm3(w));
    }
    rX = rX * (1.0 + 1e-9) + 1e-9;
    if (pass == 2) break;
    // the origin lies on the line behind X: t <= the box exit along ud
    double tex = 1e300;
    for (int a = 0; a < 3; a++) {
      if (ud[a] > 0.0) tex = fmin(tex, (p.ohi[a] - (C[a] - rX)) / ud[a]);
      if (ud[a] < 0.0) tex = fmin(tex, ((C[a] + rX) - p.olo[a]) / -ud[a]);
    }
    tex = fmax(tex, 0.0) * (1.0 + 1e-9);
    for (int i = 0; i < 3; i++)
      S[i] = fmin(S[i], (fabs(C[i] - v0[i]) + rX + tex * fabs(ud[i])) * (1.0 + 1e-9));
  }
  const double Smax = sqrt(S[0] * S[0] + S[1] * S[1] + S[2] * S[2]);
  const double ext = (1.0 + du + dv + dw) * (norm3(e1) + norm3(e2));
  // the query's float projection (3 eps s1), and X - o along d seen through
  // the float axes (|X - o| <= |S| + T_D's extent)
  const double m = 3.0 * kEps * p.s1 * 1.01 + 1e-9 * p.s1 + p.skew * (Smax + ext) * 1.01;
  double hw;
  dir_rect(p, P, v0, e1, e2, m, f, hw);
  // an accept has t* >= -E_eq / |a|: X at most derr behind the origin
  const double derr = Eeq * p.dlen / A * 1.01;
  f.kpad = derr;
  f.key = -(hw + derr + 6.0 * kEps * p.s1 * 1.01 + 1e-9 * p.s1);
}

// reach of T_D beyond T for rays at cosine c (|d| cancels), Cauchy-Schwarz
// form as csrc/rt_shadow.hip; > 1e300: no bound
RTL_FN inline double reach_at(double c, double nl, double ea, double l1, double l2, double Smax) {
  const double den = nl * c - ea;
  if (!(den > 2.0001 * ea) || !(den > 0.0)) return 1e301;
  const double rho = ea / den, kap = kCDot * kEps / den;
  const double lmax = fmax(l1, l2), ls = l1 + l2;
  return (kap * ls * (lmax + ls) * Smax / (1.0 - rho) + (4.0 * kEps + rho) * lmax / (1.0 - rho)) * (1.0 + 1e-6);
}

// |o - v0| over the origins of accepting shadow rays of a point light that
// cross T's plane within rX of T's centroid C: o lies on a line through X
// (|X - C| <= rX) passing within dline of the light, either beyond X (o = X +
// lam u, u = (X - l.v) / |X - l.v|, the crossing between o and the light) or
// beyond the light (o = l.v - mu u, the crossing past the light); every such
// o is in the origin box, so lam, mu <= the box's exit along u's cone.
RTL_FN inline double point_smax(const LbGeom& p, const double* C, const double* v0, double rX, double dline, double sbox) {
  const double D[3] = {C[0] - p.lv[0], C[1] - p.lv[1], C[2] - p.lv[2]};
  const double dc = norm3(D);
  if (!(dc > 2.0 * (rX + dline) + 1e-9)) return sbox;
  // |u - c^| <= the cone's half-angle (plus the line's offset from the light)
  const double th = asin(fmin(1.0, (rX + dline) / dc)) + (rX + dline) / (dc - rX - dline) * 1e-6 + 1e-12;
  const double sp = fmin(2.0, th * 1.001);
  double lam = 1e300, mu = 1e300;
  for (int a = 0; a < 3; a++) {
    const double ulo = D[a] / dc - sp, uhi = D[a] / dc + sp;
    if (ulo > 0.0) lam = fmin(lam, (p.ohi[a] - (C[a] - rX)) / ulo);
    if (uhi < 0.0) lam = fmin(lam, ((C[a] + rX) - p.olo[a]) / -uhi);
    // beyond the light along -u
    // (from the line's point nearest the light, within dline of it)
    if (-uhi > 0.0) mu = fmin(mu, (p.ohi[a] - p.lv[a] + dline) / -uhi);
    if (-ulo < 0.0) mu = fmin(mu, (p.lv[a] + dline - p.olo[a]) / ulo);
  }
  lam = fmax(lam, 0.0);
  // mu < 0: the line beyond the light never reaches the box (no such origin)
  const double far = mu < 0.0 ? 0.0 : dc + rX + mu;
  const double ox = fmax(lam, far) + 2.0 * dline;
  double cv[3];
  for (int a = 0; a < 3; a++) cv[a] = C[a] - v0[a];
  return fmin(sbox, (norm3(cv) + rX + ox) * (1.0 + 1e-9) + 1e-9);
}

RTL_FN inline void footprint_point_proven(const LbGeom& p, const double V[3][3], const double* v0, const double* e1,
                                   const double* e2, Foot& f) {
  double n[3];
  cross3d(e1, e2, n);
  const double nl = norm3(n), l1 = norm3(e1), l2 = norm3(e2);
  const double lmax = fmax(l1, l2), ls = l1 + l2;
  const double ea = kCA * kEps * l1 * l2 * kDMax;  // E_a / |d|
  const double Dmax = p.dmax;
  // |a_f| <= |d| (|n| + e_a) < 1e-7 for every ray: never accepted
  if (Dmax * (nl + ea) * kDMax < kAMin * (1.0 - 1e-9)) {
    f.never = true;
    return;
  }
  if (!(nl > 0.0)) {  // degenerate: a is rounding noise, u, v unbounded
    f.global = true;
    return;
  }
  const double nh[3] = {n[0] / nl, n[1] / nl, n[2] / nl};
  const double LV[3] = {p.lv[0] - v0[0], p.lv[1] - v0[1], p.lv[2] - v0[2]};
  const double sL = fabs(dot3(nh, LV));
  double vmax = 0.0, S[3];
  for (int k = 0; k < 3; k++) {
    const double X[3] = {V[k][0] - p.lv[0], V[k][1] - p.lv[1], V[k][2] - p.lv[2]};
    vmax = fmax(vmax, norm3(X));
  }
  double C[3];
  for (int a = 0; a < 3; a++) C[a] = (V[0][a] + V[1][a] + V[2][a]) / 3.0;
  double rc = 0.0;
  for (int k = 0; k < 3; k++) {
    const double d[3] = {V[k][0] - C[0], V[k][1] - C[1], V[k][2] - C[2]};
    rc = fmax(rc, norm3(d));
  }
  rc *= 1.0 + 1e-12;
  for (int i = 0; i < 3; i++) S[i] = fmax(fabs(p.olo[i] - v0[i]), fabs(p.ohi[i] - v0[i]));
  const double Sbox = sqrt(S[0] * S[0] + S[1] * S[1] + S[2] * S[2]) * (1.0 + 1e-9);
  const double dline = 2.0 * kSqrt3 * kEps * Dmax;  // fl(l.v - o) from o passes this close to l.v
  const double a_ = sL - dline, b_ = vmax * (1.0 + 1e-12) + dline;
  // rays crossing within r of T: cosine >= c(r) = a_ / (b_ + r); R = a point
  // past the smallest fixed point of g(r) = reach_at(c(r)) (g(R) <= R)
  auto fixed_point = [&](double Sm) {
    double r = 0.0;
    if (!(a_ > 0.0)) return 1e301;
    for (int it = 0; it < 64; it++) {
      const double g = reach_at(a_ / (b_ + r), nl, ea, l1, l2, Sm);
      if (!(g < 1e300)) return 1e301;
      if (g <= r) return r;
      r = g * (1.0 + 1e-9) + 1e-300;
    }
    return 1e301;
  };
  double Smax = Sbox;
  double R = fixed_point(Smax);
  bool band = true;
  double clo = 0.0;
  if (R < 1e300) {
    // H_o(c) + Dmax c + dline: how close to the plane the light must be for a
    // ray at cosine < c to be accepted at all (module comment); any origin
    // in the box, so the box's |S|
    auto q = [&](double c) {
      return ls / (nl * (1.0 - c)) *
                 ((nl * c + ea) * (1.0 + 4.0 * kEps) + kCDot * kEps * Sbox * lmax + c * Sbox * lmax) *
                 (1.0 + 1e-6) +
             Dmax * c * (1.0 + 4.0 * kEps) + dline;
    };
    if (q(0.0) < sL) {
      double lo = 0.0, hi = 0.5;
      if (q(hi) <= sL) {
        lo = hi;
      } else {
        for (int it = 0; it < 64; it++) {
          const double mid = 0.5 * (lo + hi);
          if (q(mid) <= sL)
            lo = mid;
          else
            hi = mid;
        }
      }
      const double cst = lo;  // q(cst) <= sL: no accepted ray below cst
      if (cst > 0.0) {
        const double rhi = a_ / cst - b_;
        const double hc = reach_at(cst, nl, ea, l1, l2, Sbox);
        if (hc < rhi) {  // rays at c >= cst cross within R (convexity of g)
          band = false;
          // every accepting ray crosses within R: its origin's |S| is bounded
          // by point_smax, and the fixed point again with that bound (each
          // step valid for every accepting ray)
          for (int it = 0; it < 2; it++) {
            Smax = point_smax(p, C, v0, rc + R, dline, Sbox);
            const double R2 = fixed_point(Smax);
            if (!(R2 < 1e300)) break;
            R = fmin(R, R2);
          }
          clo = a_ / (b_ + R);
        }
      }
    }
  }
  // the band alternative (valid for every triangle): rays at c >= cst
  // cross within reach_at(cst) of T; rays below leave origins in the band of
  // directions within asin(cst + dline / rmin_o) of the plane through the
  // light parallel to T's.  Taken when the bound above fails, or when its
  // cone would cover more cells than the band and a small cone (a plane
  // passing close to the light: R grows like 1 / s_L).
  {
    const double Dc[3] = {C[0] - p.lv[0], C[1] - p.lv[1], C[2] - p.lv[2]};
    const double dc = norm3(Dc), hn = 0.5 * (double)p.n;
    auto cone_cells = [&](double Rr) {
      if (!(dc > (rc + Rr) * 1.001)) return 1e300;
      const double th = asin(fmin(1.0, (rc + Rr) / dc)) * hn;
      return 3.2 * th * th + 4.0 * th + 1.0;
    };
    const double rmin_o = p.rmin_o;
#ifndef RT_LB_BAND_C
#define RT_LB_BAND_C 0.5  // the band's cosine split c* = RT_LB_BAND_C / n (cells of the cube map's side n)
#endif
    const double cst = fmax(RT_LB_BAND_C / (double)p.n, 8.0 * ea / nl);
    double Sb = Sbox, Rb = reach_at(cst, nl, ea, l1, l2, Sb);
    if (Rb < 1e300) {
      Sb = point_smax(p, C, v0, rc + Rb, dline, Sbox);
      Rb = fmin(Rb, reach_at(cst, nl, ea, l1, l2, Sb));
    }
    const double bs = cst * (1.0 + 1e-6) + (rmin_o > 0.0 ? dline / rmin_o : 1e300) + 4.0 * kEps;
    const bool bok = cst < 0.25 && Rb < 1e300 && bs < 0.3;
    const double band_cells = bok ? 4.0 * (double)p.n * (bs * kSqrt3 * hn * 2.0 + 3.0) + cone_cells(Rb) : 1e300;
    if (!band && !(cone_cells(R) > band_cells)) {
      // keep the cone alone
    } else if (bok) {
      band = true;
      R = Rb;
      Smax = Sb;
      clo = cst;
      f.band = true;
      for (int a = 0; a < 3; a++) f.bn[a] = nh[a];
      // a face cell holds directions x = (s, t, +-1): |x| <= sqrt 3
      f.bB = bs * kSqrt3 * (1.0 + 1e-9) + 1e-12;
    } else if (band) {
      f.global = true;
      return;
    }
  }
  const double rb = rc + R + 1e-12;
  double rmin = 0.0;
  if (!point_cone(p, V, C, rb, rmin, R, f)) {
    f.n = 0;
    f.band = false;
    f.global = true;
    return;
  }
  // an accept has t* >= -E_eq / |a|, |a| >= |d| |n| clo: X at most derr
  // behind the origin (toward the light)
  const double derr = kCDot * kEps * Smax * l1 * l2 / (nl * clo) * 1.01;
  f.kpad = derr;
  f.key = rmin - derr - 2.0 * dline - 1e-9 * p.dmax;
}

RTL_FN inline void footprint(const LbGeom& p, uint32_t prim, Foot& f) {
  const float* r = (const float*)(p.tri + 3 * (size_t)prim);
  const double v0[3] = {r[0], r[1], r[2]}, e1[3] = {r[3], r[4], r[5]}, e2[3] = {r[6], r[7], r[8]};
  const double V[3][3] = {{v0[0], v0[1], v0[2]},
                          {v0[0] + e1[0], v0[1] + e1[1], v0[2] + e1[2]},
                          {v0[0] + e2[0], v0[1] + e2[1], v0[2] + e2[2]}};
  foot_init(f);
  if (!p.proven)
    footprint_slack(p, V, v0, e1, e2, f);
  else if (p.kind == RT_LB_DIR)
    footprint_dir_proven(p, v0, e1, e2, f);
  else
    footprint_point_proven(p, V, v0, e1, e2, f);
}

RTL_FN inline uint64_t foot_cells(const LbGeom&, const Foot& f) {
  uint64_t c = 0;
  for (int q = 0; q < f.n; q++)
    c += (uint64_t)(f.x1[q] - f.x0[q] + 1) * (uint64_t)(f.y1[q] - f.y0[q] + 1);
  return c;
}

// key of the triangle in cell (x, y) of rect q
RTL_FN inline float cell_key(const LbGeom& p, const Foot& f, int x, int y) {
  double key = f.key;
  if (p.kind == RT_LB_DIR && f.plane) {
    // the plane's depth over the cell's column grown by the margin: points of
    // the triangle in the column lie on the plane, h = (n.v0 - n_u pu - n_v pv) / n_w;
    // the float axes are orthonormal within a few ulps (1e-6 s1 covers it)
    const double ua = p.u0 + x * p.cs - f.m, ub = p.u0 + (x + 1) * p.cs + f.m;
    const double va = p.v0 + y * p.cs - f.m, vb = p.v0 + (y + 1) * p.cs + f.m;
    double h = -1e300;
    const double us[2] = {ua, ub}, vs[2] = {va, vb};
    for (int i = 0; i < 2; i++)
      for (int k = 0; k < 2; k++) h = fmax(h, (f.pn_d - f.pn_u * us[i] - f.pn_v * vs[k]) / f.pn_w);
    const double kc = -(h + f.kpad + 6.0 * kEps * p.s1 * 1.01 + 1e-6 * p.s1);
    key = fmax(key, kc);  // the tighter (larger) of the two lower bounds of -depth
  }
  return float_rd(key);
}

// Can the triangle's grown image in rect q reach cell (x, y)?  Separating
// axis test of the cell square (grown by the margin) against the image's edge
// lines; conservative (true when unsure: degenerate images, rect-only).
RTL_FN inline bool cell_overlaps(const LbGeom& p, const Foot& f, int q, int x, int y) {
  if (!f.tri_ok[q]) return true;
  double ox, oy, cs;
  if (p.kind == RT_LB_DIR) {
    ox = p.u0;
    oy = p.v0;
    cs = p.cs;
  } else {
    cs = 2.0 / (double)p.n;
    ox = oy = -1.0;
  }
  // the query's own cell index is within 0.01 cells of its exact position
  // (the bounding rects' margin): the square grows by as much
  const double M = f.tm[q] + 0.01 * cs;
  const double xa = ox + x * cs - M, xb = ox + (x + 1) * cs + M;
  const double ya = oy + y * cs - M, yb = oy + (y + 1) * cs + M;
  const double* X = f.tx[q];
  const double* Y = f.ty[q];
  const double area = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0]);
  const double scale = fabs(X[1] - X[0]) + fabs(X[2] - X[0]) + fabs(Y[1] - Y[0]) + fabs(Y[2] - Y[0]);
  if (!(fabs(area) > 1e-9 * scale * scale)) return true;  // (nearly) degenerate image: keep
  for (int e = 0; e < 3; e++) {
    const int a = e, b = (e + 1) % 3;
    // inward normal of edge a -> b (toward the third vertex)
    double nx = -(Y[b] - Y[a]), ny = X[b] - X[a];
    if (area < 0.0) {
      nx = -nx;
      ny = -ny;
    }
    // the square is outside when all its corners are beyond the edge line
    const double cx = nx > 0.0 ? xb : xa, cy = ny > 0.0 ? yb : ya;  // the corner farthest inward
    const double d = nx * (cx - X[a]) + ny * (cy - Y[a]);
    const double tol = 1e-9 * (fabs(nx) + fabs(ny)) * (fabs(cx) + fabs(cy) + fabs(X[a]) + fabs(Y[a]) + cs);
    if (d < -tol) return false;
  }
  return true;
}

RTL_FN inline uint32_t cell_index(const LbGeom& p, const Foot& f, int q, int x, int y) {
  if (p.kind == RT_LB_DIR) return (uint32_t)y * p.nx + (uint32_t)x;
  return f.face[q] * p.n * p.n + (uint32_t)y * p.n + (uint32_t)x;
}

// Band row (face, y) of a POINT footprint: the columns whose cells hold a
// direction x = (s, t, sigma) (face frame: s along axis a+1, t along a+2, as
// the query maps them) with |x.bn| <= bB; false: none.  Widened by 0.02 cells
// for the query's rounding.
RTL_FN inline bool band_row(const LbGeom& p, const Foot& f, uint32_t face, uint32_t y, int& xa, int& xb) {
  const int a = (int)(face >> 1), j = (a + 1) % 3, k = (a + 2) % 3;
  const double sigma = (face & 1) ? -1.0 : 1.0;
  const double cs = 2.0 / (double)p.n, pad = 0.02 * cs;
  const double t0 = -1.0 + y * cs - pad, t1 = -1.0 + (y + 1) * cs + pad;
  const double nj = f.bn[j], nk = f.bn[k], na = f.bn[a];
  const double g0 = nk * t0 + na * sigma, g1 = nk * t1 + na * sigma;
  const double glo = fmin(g0, g1), ghi = fmax(g0, g1);
  const double B = f.bB;
  double lo, hi;
  if (fabs(nj) < 1e-12) {
    if (glo > B + 1e-12 || ghi < -B - 1e-12) return false;
    lo = -1.0;
    hi = 1.0;
  } else {
    const double A0 = (-B - ghi) / nj, A1 = (B - glo) / nj;
    lo = fmin(A0, A1) - pad;
    hi = fmax(A0, A1) + pad;
  }
  if (lo > 1.0 || hi < -1.0) return false;
  const double hn = 0.5 * (double)p.n;
  xa = clampi(floor((fmax(lo, -1.0) + 1.0) * hn - 0.02), (int)p.n - 1);
  xb = clampi(floor((fmin(hi, 1.0) + 1.0) * hn + 0.02), (int)p.n - 1);
  return xa <= xb;
}

// A footprint as rows: each rect's rows, then (band) the 6 n rows of the cube map.
RTL_FN inline uint32_t foot_rows(const LbGeom& p, const Foot& f) {
  uint32_t r = 0;
  for (int q = 0; q < f.n; q++) r += (uint32_t)(f.y1[q] - f.y0[q] + 1);
  if (f.band) r += 6u * p.n;
  return r;
}

// entries of row `row`; with emit, written from `at` on, never at or past
// `lim` (the prim's own range: a count/emission mismatch is flagged in
// ctr[RT_LBC_OVERFLOW], not written out of bounds).  P: the geometry alone to
// count; to emit, the geometry with keys, vals and ctr (rtl::BP of
// rt_lightbuf.hip over device memory; tests/native/lightbuf_geom.cpp has one
// over host memory, so the host walks the emission's own loop).
template <bool EMIT, class P>
RTL_FN inline uint32_t row_entries(const P& p, const Foot& f, uint32_t prim, uint32_t row, uint64_t at,
                                       uint64_t lim) {
  for (int q = 0; q < f.n; q++) {
    const uint32_t nr = (uint32_t)(f.y1[q] - f.y0[q] + 1);
    if (row >= nr) {
      row -= nr;
      continue;
    }
    const int y = f.y0[q] + (int)row;
    uint32_t c = 0;
    for (int x = f.x0[q]; x <= f.x1[q]; x++)
      if (cell_overlaps(p, f, q, x, y)) {
        if constexpr (EMIT) {
          if (at + c >= lim) {
            p.ctr[RT_LBC_OVERFLOW] = 1u;
            return c;
          }
          p.keys[at + c] = ((unsigned long long)cell_index(p, f, q, x, y) << 32) | orderable(cell_key(p, f, x, y));
          p.vals[at + c] = prim;
        }
        c++;
      }
    return c;
  }
  // band rows: always tested (key -inf)
  const uint32_t face = row / p.n, y = row % p.n;
  int xa = 0, xb = -1;
  if (!band_row(p, f, face, y, xa, xb)) return 0;
  if constexpr (EMIT) {
    const uint32_t kb = orderable(-__builtin_inff());
    for (int x = xa; x <= xb; x++) {
      const uint64_t i = at + (uint64_t)(x - xa);
      if (i >= lim) {
        p.ctr[RT_LBC_OVERFLOW] = 1u;
        break;
      }
      p.keys[i] = ((unsigned long long)(face * p.n * p.n + y * p.n + (uint32_t)x) << 32) | kb;
      p.vals[i] = prim;
    }
  }
  return (uint32_t)(xb - xa + 1);
}

RTL_FN inline bool foot_is_big(const LbGeom& p, const Foot& f) { return f.band || foot_cells(p, f) > kSmallCells; }

// distance from x to the triangle (a, b, c), double: the closest point by the
// interior / edge cases
RTL_FN inline double pt_tri_dist(const double* x, const double* a, const double* b, const double* c) {
  double ab[3], ac[3], ax[3];
  for (int i = 0; i < 3; i++) {
    ab[i] = b[i] - a[i];
    ac[i] = c[i] - a[i];
    ax[i] = x[i] - a[i];
  }
  double n[3];
  cross3d(ab, ac, n);
  const double nn = dot3(n, n);
  if (nn > 0.0) {
    double t[3], s[3];
    cross3d(ab, ax, t);
    cross3d(ax, ac, s);
    const double v = dot3(t, n) / nn, u = dot3(s, n) / nn;
    if (u >= 0.0 && v >= 0.0 && u + v <= 1.0) return fabs(dot3(ax, n)) / sqrt(nn);
  }
  double best = 1e300;
  const double* P[3] = {a, b, c};
  for (int e = 0; e < 3; e++) {
    const double* p0 = P[e];
    const double* p1 = P[(e + 1) % 3];
    double d[3], w[3];
    for (int i = 0; i < 3; i++) {
      d[i] = p1[i] - p0[i];
      w[i] = x[i] - p0[i];
    }
    const double dd = dot3(d, d);
    double t = dd > 0.0 ? dot3(w, d) / dd : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double z[3] = {w[0] - t * d[0], w[1] - t * d[1], w[2] - t * d[2]};
    best = fmin(best, norm3(z));
  }
  return best;
}

// a lower bound of the distance from the light to the shadow-ray origins on
// this triangle (hit points: on it up to their float rounding, 1e-6 s1)
RTL_FN inline double prim_rmin(const LbGeom& p, uint32_t prim) {
  const float* r = (const float*)(p.tri + 3 * (size_t)prim);
  const double v0[3] = {r[0], r[1], r[2]};
  const double v1[3] = {v0[0] + r[3], v0[1] + r[4], v0[2] + r[5]};
  const double v2[3] = {v0[0] + r[6], v0[1] + r[7], v0[2] + r[8]};
  const double d = pt_tri_dist(p.lv, v0, v1, v2) * (1.0 - 1e-9) - 1e-6 * p.s1;
  return d > 0.0 ? d : 0.0;
}

}  // namespace rtl

// rt_lightbuf_host.cpp: the geometry of a build from its parameters -- the
// grid alone (the device build finds rmin_o itself), or all of it on the host
int lb_derive_grid(const LBParams* in, rtl::LbGeom& p, RtLightBuf* out, uint64_t& ncell, char* err, size_t errlen);
int lb_geom_host(const LBParams* in, rtl::LbGeom& p, RtLightBuf* lb, uint64_t& ncell, char* err, size_t errlen);
