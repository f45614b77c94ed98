// rt_cand_geom.h -- the proof geometry of the camera rays' candidate lists
// (DESIGN.md §2 "Exact camera rays"): the error-bound constants, Footprint
// and its classification (classify), the float fast path (quick_class,
// rank_may_touch), the raster family that turns a footprint into this rank's
// tiles (raster_rows, row_tiles, raster_row / count_row / row_ivs, raster /
// raster_count), the per-tile refinement (TileTri, TileFrame, tile_keep) and
// the footprint size classes (kSmallRows, kSmallEntries, refined_footprint).
// Double and float arithmetic only, all of it __host__ __device__: no kernel,
// no thread index, no memory but its arguments.  The device passes
// (rt_cand_passes.h, in rt_cand.hip's one translation unit) and the host
// mirrors (rt_cand_host.cpp) run this same code, so a host re-derivation
// gives the device's bits; a plain C++ compiler builds it too
// (tests/native/cand_geom.cpp, -D__HIP_PLATFORM_AMD__ for the HIP headers'
// types).  Needs CandParams (rt_cand.h) and the tile map (rt_tiles.h),
// included here.
#pragma once

#include <cmath>
#include <cstdint>

#include "rt_cand.h"
#include "rt_tiles.h"

namespace rtc {

constexpr double kEps = 0x1p-24;             // float unit roundoff
constexpr double kAMin = 9.99999997e-08;     // (double)(float)1e-7, cpu/hit.c:7
constexpr double kDMin = 1.0 - 4.0 * kEps;   // |normalize(.)| of a float vector
constexpr double kDMax = 1.0 + 4.0 * kEps;

#define RTC_FN __host__ __device__ __forceinline__

RTC_FN double dot3(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
RTC_FN double norm3(const double* a) { return sqrt(dot3(a, a)); }
RTC_FN double dist3(const double* a, const double* b) {
  double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
  return sqrt(x * x + y * y + z * z);
}

enum { SAFE = 0, FOOTPRINT = 1, GLOBAL = 2 };

// The camera samples a triangle can be a float-MT candidate for, as a
// superset: (projected T_D widened by dimg, if tri_ok) intersected with the
// band of lines nearly parallel to the triangle's plane, |b0 + b1 k + b2 l|
// <= hw (b = n . (pos - o(k, l)), world units); plus, for very large
// triangles whose |a| error can reach the 1e-7 threshold, the thinner band
// hw0 of the lines too parallel to bound (c_ok > 0).
struct Footprint {
  int tri_ok;
  double k[3], l[3], dimg;
  double b0, b1, b2, hw, hw0;
  float skip;  // lower bound of (float new_dist) - |pos - o| over the candidate crossings
};

// point-triangle distance (double): closest point by the edge/interior cases
RTC_FN double pt_tri_dist(const double* x, const double* a, const double* b, const double* c) {
  double ab[3], ac[3], ax[3];
  for (int i = 0; i < 3; i++) {
    ab[i] = b[i] - a[i];
    ac[i] = c[i] - a[i];
    ax[i] = x[i] - a[i];
  }
  const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2],
                       ab[0] * ac[1] - ab[1] * ac[0]};
  const double nn = dot3(n, n);
  if (nn > 0.0) {  // interior: barycentrics of the projection
    double t[3] = {ab[1] * ax[2] - ab[2] * ax[1], ab[2] * ax[0] - ab[0] * ax[2],
                   ab[0] * ax[1] - ab[1] * ax[0]};
    double s[3] = {ax[1] * ac[2] - ax[2] * ac[1], ax[2] * ac[0] - ax[0] * ac[2],
                   ax[0] * ac[1] - ax[1] * ac[0]};
    const double inn = 1.0 / nn;  // (an ulp of the barycentrics: the edge cases take over)
    const double v = dot3(t, n) * inn, u = dot3(s, n) * inn;
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
    double z[3] = {w[0] - t * d[0], w[1] - t * d[1], w[2] - t * d[2]};
    best = fmin(best, norm3(z));
  }
  return best;
}

// Classify one triangle (record r: v0, e1, e2 as floats) and build its footprint.
// td (optional, FOOTPRINT only): the bounding box of T_D(cl) (lo xyz, hi xyz)
// and the distance error derr; td[6] = -1 when T_D has no bound for every
// candidate line (c_ok > 0).
RTC_FN int classify(const CandParams& p, const float* r, const float* leafbox, Footprint& fp,
                    double* td = nullptr, int* why = nullptr) {
  const double v0[3] = {r[0], r[1], r[2]}, e1[3] = {r[3], r[4], r[5]}, e2[3] = {r[6], r[7], r[8]};
  const double v1[3] = {v0[0] + e1[0], v0[1] + e1[1], v0[2] + e1[2]};
  const double v2[3] = {v0[0] + e2[0], v0[1] + e2[1], v0[2] + e2[2]};
  const double l1 = norm3(e1), l2 = norm3(e2);
  const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                       e1[0] * e2[1] - e1[1] * e2[0]};
  const double nl = norm3(n);
  double e_a = p.c_a * kEps * l1 * l2 * kDMax;
  if (nl * kDMax + e_a < kAMin) {  // |a| < 1e-7 for every ray: never accepted
    if (why) *why = 0;
    return SAFE;
  }
  // degenerate (collinear or repeated vertices) with edges long enough for
  // rounding alone to lift |a| past 1e-7: a is noise, u and v are unbounded,
  // no line has a bound (c_ok = inf) and n / |n| would put NaN into every band
  // coefficient below -- every camera ray tests it (as rt_lightbuf_geom.h's
  // footprint_point_proven does for the shadow rays)
  if (!(nl > 0.0)) return GLOBAL;
  const double inl = 1.0 / nl;  // (the unit normal to an ulp or two: inside every margin below)
  const double nh[3] = {n[0] * inl, n[1] * inl, n[2] * inl};
  const double pv[3] = {p.pos[0] - v0[0], p.pos[1] - v0[1], p.pos[2] - v0[2]};
  const double deye = fabs(dot3(nh, pv));
  const double smax = p.lmax + norm3(pv);  // |o - v0| <= |o - pos| + |pos - v0|
  double e_sh = p.c_dot * kEps * smax * kDMax * l2;
  double e_dq = p.c_dot * kEps * smax * kDMax * l1;
  double e_eq = p.c_dot * kEps * smax * l1 * l2;
  // lines with grazing cosine c: |a| >= a_lb(c); the bound of
  // tools/mt_bound.py needs rho = e_a / a_lb < 1/2, i.e. c >= c_ok
  const double c_ok = kAMin >= 2.0 * e_a ? 0.0 : 3.0 * e_a / (kDMin * nl);
  auto alb = [&](double c) { return fmax(kAMin, kDMin * nl * c - e_a); };
  double P[3][3];
  // T_D(c) corners; returns how far they reach beyond the triangle
  // (two divisions instead of five: the products differ from the quotients
  // by an ulp or two, far inside the bound's own slack -- its constants are
  // rounded up by 1.3 %, tools/mt_bound.py)
  auto expand = [&](double c, double& rho_o, double& a_o) {
    const double a = alb(c), ia = 1.0 / a, rho = e_a * ia, i1r = 1.0 / (1.0 - rho);
    const double du = e_sh * ia * i1r, dv = e_dq * ia * i1r;
    const double dw = (4.0 * kEps + (e_sh + e_dq) * ia + rho) * i1r;
    for (int k = 0; k < 3; k++) {
      P[0][k] = v0[k] - du * e1[k] - dv * e2[k];
      P[1][k] = v0[k] + (1.0 + dw + dv) * e1[k] - dv * e2[k];
      P[2][k] = v0[k] - du * e1[k] + (1.0 + dw + du) * e2[k];
    }
    rho_o = rho;
    a_o = a;
    return fmax(dist3(P[0], v0), fmax(dist3(P[1], v1), dist3(P[2], v2)));
  };
  // K' >= c H(c) over every c >= c_ok: with a_lb = dmin nl c - e_a, c H(c)
  // is a convex rational function of c, so its maximum is at an end point
  double rho = 0.0, a_lb = 0.0, kmax_ch;
  const double ck = fmax(c_ok, (kAMin + e_a) / (kDMin * nl));  // kink of a_lb(c)
  {
    double rr, aa;
    kmax_ch = fmax(fmin(ck, 1.0) * expand(fmin(ck, 1.0), rr, aa), expand(1.0, rr, aa));
  }
  // smallest grazing cosine of a camera line through T_D: such a line
  // passes within dline of the eye, so c >= (deye - dline) / (|X - pos| +
  // dline) with |X - pos| <= max |v - pos| + H(c), and c H(c) <= K'
  double vmax = 0.0;
  {
    const double* V[3] = {v0, v1, v2};
    for (int k = 0; k < 3; k++) vmax = fmax(vmax, dist3(V[k], p.pos));
  }
  double cl = fmax(c_ok, (deye - p.dline - kmax_ch) / (vmax + p.dline));
  double hreach = expand(cl, rho, a_lb);
  // Second round, componentwise (tools/mt_bound.py stress_cw): every
  // candidate line crosses T_D, so its direction lies in the cone from the
  // eye to T_D's bounding sphere, which bounds each |d_i| and |S_i| =
  // |o_i - v0_i| <= lmax |d_i| + |pos_i - v0_i|; the sums
  //   E_sh <= 6.01 eps sum |S_i| M_i,  M_i = |d_j| |e2_k| + |d_k| |e2_j|
  //   E_dq <= 6.01 eps sum |d_i| N_i,  N_i = |S_j| |e1_k| + |S_k| |e1_j|
  //   E_eq <= 6.01 eps sum |e2_i| N_i, E_a <= 5.01 eps sum |e1_i| M_i
  // are much smaller than their Cauchy-Schwarz versions for camera rays.
  if (c_ok == 0.0) {
    double q[3], qr = 0.0;
    for (int a = 0; a < 3; a++) q[a] = (P[0][a] + P[1][a] + P[2][a]) / 3.0;
    for (int k = 0; k < 3; k++) qr = fmax(qr, dist3(P[k], q));
    const double R = dist3(q, p.pos);
    if (R > 2.0 * (qr + p.dline)) {
      const double iR = 1.0 / R;
      const double st = (qr + p.dline) * iR * 1.42 + 8.0 * kEps;  // |d - q^| <= 2 sin(theta / 2)
      double dm[3], sm[3], ae1[3], ae2[3];
      for (int a = 0; a < 3; a++) {
        dm[a] = fmin(1.0, fabs(q[a] - p.pos[a]) * iR + st) * kDMax;
        sm[a] = ((p.lmax + p.dline) * dm[a] + fabs(pv[a]) + p.dline) * (1.0 + 1e-9);
        ae1[a] = fabs(e1[a]);
        ae2[a] = fabs(e2[a]);
      }
      double M[3], N[3];
      for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        M[i] = dm[j] * ae2[k] + dm[k] * ae2[j];
        N[i] = sm[j] * ae1[k] + sm[k] * ae1[j];
      }
      const double cw = p.c_dot / 8.6 * 6.01 * kEps, ca = p.c_a / 7.2 * 5.01 * kEps;
      const double w_sh = cw * (sm[0] * M[0] + sm[1] * M[1] + sm[2] * M[2]);
      const double w_dq = cw * (dm[0] * N[0] + dm[1] * N[1] + dm[2] * N[2]);
      const double w_eq = cw * (ae2[0] * N[0] + ae2[1] * N[1] + ae2[2] * N[2]);
      const double w_a = ca * (ae1[0] * M[0] + ae1[1] * M[1] + ae1[2] * M[2]);
      if (w_sh < e_sh) e_sh = w_sh;
      if (w_dq < e_dq) e_dq = w_dq;
      if (w_eq < e_eq) e_eq = w_eq;
      if (w_a < e_a) e_a = w_a;
      double rr, aa;
      const double ck2 = fmax(c_ok, (kAMin + e_a) / (kDMin * nl));
      kmax_ch = fmax(fmin(ck2, 1.0) * expand(fmin(ck2, 1.0), rr, aa), expand(1.0, rr, aa));
      cl = fmax(cl, (deye - p.dline - kmax_ch) / (vmax + p.dline));
      hreach = expand(cl, rho, a_lb);
    }
  }
  const double rmax = fmax(dist3(P[0], p.pos), fmax(dist3(P[1], p.pos), dist3(P[2], p.pos)));
  const double derr = kDMax * e_eq / (a_lb * (1.0 - rho)) +
                      (rmax + p.lmax) * (rho + 4.0 * kEps) / (1.0 - rho) +
                      4.0 * kEps * (p.omax + rmax + p.lmax);
  // safe: every crossing point lies within the slack of the box of a leaf
  // holding the triangle (so the walk visits that leaf and tests it), and
  // the float distance error cannot push it past the walk's pruning
  if (c_ok == 0.0 && derr <= 2.0 * p.eps_avail) {
    if (hreach <= p.eps_avail) {
      if (why) *why = 1;
      return SAFE;
    }
    if (leafbox) {
      const double e = p.eps_avail;
      bool in = true;
      for (int k = 0; k < 3 && in; k++)
        for (int a = 0; a < 3 && in; a++)
          in = P[k][a] >= (double)leafbox[a] - e && P[k][a] <= (double)leafbox[4 + a] + e;
      if (in) {
        if (why) *why = 2;
        return SAFE;
      }
    }
  }
  // band: a candidate line at cosine c crosses the plane |h'| / c from a
  // point within dline of the eye, within H(c) of the triangle, so
  // c (r_T - dline) - (deye + dline) <= c H(c) <= K' (max over c >= c_ok)
  const double rT = pt_tri_dist(p.pos, v0, v1, v2);
  if (!(rT > 2.0 * p.dline + 1e-9)) return GLOBAL;
  const double c_band = fmin(1.0, (deye + p.dline + kmax_ch) / (rT - p.dline));
  // cpu/hit.c:19-20 rejects |a| < 1e-7, and |a| <= kDMax nl c + e_a: no
  // line with c < c_min is accepted.  Every candidate line has c <= c_band,
  // so c_min > c_band leaves none (with c_ok > 0 the lines below c_ok are
  // unbounded and c_min < c_ok: no exit there)
  if (c_ok == 0.0 && (kAMin - e_a) > c_band * (kDMax * nl) * (1.0 + 1e-6)) {
    if (why) *why = 3;
    return SAFE;
  }
  const double wide = p.lmax + p.dline + p.dorig;
  fp.b0 = dot3(nh, p.pos) - dot3(nh, p.C);
  fp.b1 = -dot3(nh, p.u);
  fp.b2 = -dot3(nh, p.v);
  fp.hw = c_band * wide + p.dline + p.dorig + 1e-9 * wide;
  fp.hw0 = c_ok > 0.0 ? c_ok * wide + p.dline + p.dorig + 1e-9 * wide : -1.0;
  // the projected T_D, valid when it stays on one side of the eye plane
  fp.tri_ok = 0;
  double yn[3];
  for (int k = 0; k < 3; k++) {
    const double Y[3] = {P[k][0] - p.pos[0], P[k][1] - p.pos[1], P[k][2] - p.pos[2]};
    yn[k] = dot3(Y, p.n);
  }
  const double rmin = pt_tri_dist(p.pos, P[0], P[1], P[2]);
  const double ymag = rmax + 1.0;
  if (rmin > 1e-6 && (fmin(yn[0], fmin(yn[1], yn[2])) > 1e-9 * ymag ||
                      fmax(yn[0], fmax(yn[1], yn[2])) < -1e-9 * ymag)) {
    fp.tri_ok = 1;
    for (int k = 0; k < 3; k++) {
      const double lam = p.plane / yn[k];
      double w[3];
      for (int c = 0; c < 3; c++) w[c] = p.pos[c] + lam * (P[k][c] - p.pos[c]) - p.C[c];
      const double b1 = dot3(w, p.u), b2 = dot3(w, p.v);
      fp.k[k] = p.ginv[0] * b1 + p.ginv[1] * b2;
      fp.l[k] = p.ginv[1] * b1 + p.ginv[2] * b2;
    }
    // a float camera line through X passes within dline of the eye: at the
    // image plane it lands within dline (1 + lmax / |X - pos|) of X's projection
    fp.dimg = 1.5 * p.gscale * (p.dline * (1.0 + p.lmax / rmin) + p.dorig) + 1e-3;
  }
  // depth skip: new_dist >= |pos - o| + |X - pos| - 2 dline - derr
  const double sk = c_ok > 0.0 ? -1e30 : rmin - 2.0 * p.dline - derr - 1e-6 * (p.lmax + rmax) - 1e-3;
  fp.skip = sk > 0.0 ? (float)(sk * (1.0 - 1e-6)) : -1e30f;
  if (td) {
    for (int a = 0; a < 3; a++) {
      td[a] = fmin(P[0][a], fmin(P[1][a], P[2][a]));
      td[3 + a] = fmax(P[0][a], fmax(P[1][a], P[2][a]));
    }
    td[6] = c_ok > 0.0 ? -1.0 : derr;
  }
  return FOOTPRINT;
}

// This rank's tiles in tile row ty, columns [x0, x1] (csrc/rt_tiles.h).
__host__ __device__ inline uint32_t rank_tiles(const CandParams& p, int ty, int x0, int x1) {
  if (x0 > x1) return 0u;
  return rt_rank_row_tiles(ty, x0, x1, (uint32_t)p.nranks, (uint32_t)p.rank, (uint32_t)p.blocks_x,
                           (uint32_t)p.tb, nullptr);
}

// The pixel columns (rows: row = true) whose samples' k (l) can lie in
// [a, b], clamped to the frame (empty: c0 > c1).  cpu/rt: pixel c samples
// k in [W/2 - c, W/2 - c + 1/2] (cpu/raytracer.c:55-58);
// compatibility mode: pixel c is the one sample k = c - W/2.  Clamped in
// double before the conversion (a far-off footprint gives values beyond
// int range, whose conversion the host does not saturate).
__host__ __device__ inline void pixel_range(const CandParams& p, double a, double b, int& c0, int& c1, bool row) {
  const int n = row ? p.H : p.W;
  const double h = (double)(n / 2);
  if (p.compat) {
    c0 = (int)fmin(fmax(0.0, ceil(a + h)), (double)n);
    c1 = (int)fmax(fmin((double)(n - 1), floor(b + h)), -1.0);
  } else {
    c0 = (int)fmin(fmax(0.0, ceil(h - b)), (double)n);
    c1 = (int)fmax(fmin((double)(n - 1), floor(h - a + 0.5)), -1.0);
  }
}

// Can a footprint inside the ball (q, rb) -- every candidate crossing point
// of the triangle lies in it -- reach a tile of this rank?  The ball's
// bounding box projects (through the eye, on one side of the eye plane) into
// the image rectangle spanned by its corners' projections; widened by the
// float deviation of camera lines (classify's dimg) plus 2 pixels, it gives
// the pixel rows and columns the footprint can touch, clipped to the frame.
// false = none of this rank's tiles (off-frame, or between the rank's tiles
// of an interleaved split); true whenever unsure.
RTC_FN bool rank_may_touch(const CandParams& p, const double q[3], double rb) {
  // in float (the triangles that reach here are a third of the scene): the
  // corners must lie well in front of the eye (|Y . n| >= |Y| / 20, i.e.
  // within ~87 degrees of the view axis; anything else is kept), so the
  // projection's relative rounding stays below 1e-5 and its absolute error
  // below a pixel -- covered by the 3-pixel margin
  const float dq0 = (float)(q[0] - p.pos[0]), dq1 = (float)(q[1] - p.pos[1]),
              dq2 = (float)(q[2] - p.pos[2]);
  const float rbf = (float)rb;
  const float R = sqrtf(dq0 * dq0 + dq1 * dq1 + dq2 * dq2);
  if (!(R > 2.0f * rbf + 1e-6f)) return true;
  const float n0 = (float)p.n[0], n1 = (float)p.n[1], n2 = (float)p.n[2];
  const float u0 = (float)p.u[0], u1 = (float)p.u[1], u2 = (float)p.u[2];
  const float v0 = (float)p.v[0], v1 = (float)p.v[1], v2 = (float)p.v[2];
  const float pc0 = (float)(p.pos[0] - p.C[0]), pc1 = (float)(p.pos[1] - p.C[1]),
              pc2 = (float)(p.pos[2] - p.C[2]);
  const float plane = (float)p.plane, g0 = (float)p.ginv[0], g1 = (float)p.ginv[1],
              g2 = (float)p.ginv[2];
  const float ymin = 0.05f * (R + 1.8f * rbf);
  float kmn = 1e30f, kmx = -1e30f, lmn = 1e30f, lmx = -1e30f;
  int side = 0;
  for (int c = 0; c < 8; c++) {
    const float Y0 = dq0 + ((c & 1) ? rbf : -rbf), Y1 = dq1 + ((c & 2) ? rbf : -rbf),
                Y2 = dq2 + ((c & 4) ? rbf : -rbf);
    const float yn = Y0 * n0 + Y1 * n1 + Y2 * n2;
    const int sd = yn > ymin ? 1 : (yn < -ymin ? -1 : 0);
    if (sd == 0 || (side != 0 && sd != side)) return true;
    side = sd;
    const float lam = plane / yn;
    const float w0 = pc0 + lam * Y0, w1 = pc1 + lam * Y1, w2 = pc2 + lam * Y2;
    const float b1 = w0 * u0 + w1 * u1 + w2 * u2, b2 = w0 * v0 + w1 * v1 + w2 * v2;
    const float k = g0 * b1 + g1 * b2, l = g1 * b1 + g2 * b2;
    kmn = fminf(kmn, k);
    kmx = fmaxf(kmx, k);
    lmn = fminf(lmn, l);
    lmx = fmaxf(lmx, l);
  }
  const double m = 3.0 + 1.5 * p.gscale * (p.dline * (1.0 + p.lmax / ((double)R - 2.0 * rb)) + p.dorig) +
                   1e-5 * (fabs((double)kmn) + fabs((double)kmx) + fabs((double)lmn) + fabs((double)lmx));
  kmn -= m;
  kmx += m;
  lmn -= m;
  lmx += m;
  // samples of pixel (r, c): k in [W/2 - c, W/2 - c + 1/2], l likewise (raster_rows)
  int r0, r1, c0, c1;
  pixel_range(p, (double)kmn, (double)kmx, c0, c1, false);
  pixel_range(p, (double)lmn, (double)lmx, r0, r1, true);
  if (r0 > r1 || c0 > c1) return false;  // off the frame
  const uint32_t n = (uint32_t)p.nranks, rk = (uint32_t)p.rank;
  if (n == 1) return true;
  // whole tb x tb-tile blocks per rank, block (bx, by) -> rank (bx + by) mod
  // n (csrc/rt_tiles.h): a block column range of >= n blocks meets every
  // rank in every block row; otherwise one check per block row (the residues
  // of the rows repeat with period n)
  const int bx0 = (c0 >> 3) / p.tb, bx1 = (c1 >> 3) / p.tb;
  const int by0 = (r0 >> 3) / p.tb, by1 = (r1 >> 3) / p.tb;
  if ((uint32_t)(bx1 - bx0 + 1) >= n) return true;
  const int rows = by1 - by0 + 1 < (int)n ? by1 - by0 + 1 : (int)n;
  for (int k = 0; k < rows; k++) {
    const uint32_t res = rt_row_res((uint32_t)(by0 + k), n, rk);
    const uint32_t f = (uint32_t)bx0 <= res ? res : (uint32_t)bx0 + (res + n - (uint32_t)bx0 % n) % n;
    if (f <= (uint32_t)bx1) return true;
  }
  return false;
}

enum { Q_SAFE = 0, Q_LIST = 1, Q_AWAY = 2 };

// Fast, conservative float version of classify()'s SAFE test (no leaf box):
// every quantity is a positive magnitude computed in a few float operations,
// bounded with explicit margins, so a true result is a proof on its own.
// Most triangles of a frame take this exit.  A triangle it cannot prove safe
// whose error region provably stays off this rank's tiles (rank_may_touch)
// is Q_AWAY: its footprint would be empty here, so it is not classified.
RTC_FN int quick_class(const CandParams& p, const float* r) {
  const float fe = 5.9604645e-8f;
  const float e1x = r[3], e1y = r[4], e1z = r[5], e2x = r[6], e2y = r[7], e2z = r[8];
  const float l1 = sqrtf(e1x * e1x + e1y * e1y + e1z * e1z) * 1.00001f;
  const float l2 = sqrtf(e2x * e2x + e2y * e2y + e2z * e2z) * 1.00001f;
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float nl = sqrtf(nx * nx + ny * ny + nz * nz);
  // |n| and its direction carry an absolute error <= 4 eps |e1| |e2|
  const float nerr = 4.0f * fe * l1 * l2;
  if (!(nl > 64.0f * nerr)) return Q_LIST;
  const float nlo = nl - nerr;
  float e_a = (float)p.c_a * fe * l1 * l2 * 1.0001f;
  const float amin = 9.99999975e-08f;
  if (amin < 2.0f * e_a) return Q_LIST;
  const float px = (float)p.pos[0] - r[0], py = (float)p.pos[1] - r[1], pz = (float)p.pos[2] - r[2];
  const float pvl = sqrtf(px * px + py * py + pz * pz) * 1.00001f + 1e-6f;
  const float deye = fabsf(nx * px + ny * py + nz * pz) / nl;
  const float deye_lb = deye - pvl * (2.0f * nerr / nlo + 8.0f * fe) - 1e-6f;
  const float smax = ((float)p.lmax + pvl) * 1.00001f;
  float e_sh = (float)p.c_dot * fe * smax * l2 * 1.0001f;
  float e_dq = (float)p.c_dot * fe * smax * l1 * 1.0001f;
  float e_eq = (float)p.c_dot * fe * smax * l1 * l2 * 1.0001f;
  const float dmin = 1.0f - 4.0f * fe;
  // H(c) <= (du + dv + dw) (l1 + l2) with a = a_lb(c).  The quotients share
  // two IEEE reciprocals (this kernel is VALU-bound, a division is ~10
  // instructions): each product adds one rounding of a positive term (rho <=
  // 1/2 above), far inside the 1.0001 margin
  auto H = [&](float c, float& a_o, float& rho_o) {
    const float a = fmaxf(amin, (dmin * nlo * c - e_a) * 0.99999f);
    const float ra = 1.0f / a;
    const float rho = e_a * ra;
    const float rom = 1.0f / (1.0f - rho);
    const float du = e_sh * ra * rom, dv = e_dq * ra * rom;
    const float dw = (4.0f * fe + (e_sh + e_dq) * ra + rho) * rom;
    a_o = a;
    rho_o = rho;
    return (du + dv + dw) * (l1 + l2) * 1.0001f;
  };
  // H with the corners' own displacements (classify's expand: |du e1 + dv
  // e2|, |(dw + dv) e1 - dv e2|, |-du e1 + (dw + du) e2|) instead of their
  // common bound (du + dv + dw)(l1 + l2), which is up to ~2x larger: the
  // crossing region's reach, whose test below decides most triangles.  The
  // vectors' rounding is absolute (cancellation), so it is bounded by 8 eps
  // of the terms' magnitudes on top of the relative margin.
  auto Ht = [&](float c, float& a_o, float& rho_o) {
    const float a = fmaxf(amin, (dmin * nlo * c - e_a) * 0.99999f);
    const float ra = 1.0f / a;
    const float rho = e_a * ra;
    const float rom = 1.0f / (1.0f - rho);
    const float du = e_sh * ra * rom, dv = e_dq * ra * rom;
    const float dw = (4.0f * fe + (e_sh + e_dq) * ra + rho) * rom;
    a_o = a;
    rho_o = rho;
    const float p1 = dw + dv, p2 = dw + du;
    const float x0 = du * e1x + dv * e2x, y0 = du * e1y + dv * e2y, z0 = du * e1z + dv * e2z;
    const float x1 = p1 * e1x - dv * e2x, y1 = p1 * e1y - dv * e2y, z1 = p1 * e1z - dv * e2z;
    const float x2 = p2 * e2x - du * e1x, y2 = p2 * e2y - du * e1y, z2 = p2 * e2z - du * e1z;
    const float m = fmaxf(x0 * x0 + y0 * y0 + z0 * z0, fmaxf(x1 * x1 + y1 * y1 + z1 * z1, x2 * x2 + y2 * y2 + z2 * z2));
    return sqrtf(m) * 1.0002f + 8.0f * fe * (p1 + p2) * (l1 + l2);
  };
  float a, rho;
  const float ck = fminf(1.0f, (amin + e_a) / (dmin * nlo) * 1.0001f);
  const float kmax_ch = fmaxf(ck * H(ck, a, rho), H(1.0f, a, rho)) * 1.0001f;
  float vmax = 0.0f;
  for (int k = 0; k < 3; k++) {
    const float ox = k == 0 ? 0.0f : (k == 1 ? e1x : e2x), oy = k == 0 ? 0.0f : (k == 1 ? e1y : e2y),
                oz = k == 0 ? 0.0f : (k == 1 ? e1z : e2z);
    const float qx = px - ox, qy = py - oy, qz = pz - oz;
    vmax = fmaxf(vmax, sqrtf(qx * qx + qy * qy + qz * qz));
  }
  vmax = vmax * 1.00002f + 1e-6f;
  float num = deye_lb - (float)p.dline - kmax_ch - 1e-5f * (deye + kmax_ch);
  if (!(num > 0.0f)) return Q_LIST;
  float cl = num / (vmax + (float)p.dline) * 0.9999f;
  float h = H(cl, a, rho);
  // componentwise second round (see classify): the candidate lines cross
  // T_D, inside the ball (centroid, max vertex distance + h) -- with the
  // common bound h, so that the cone, and the componentwise error terms from
  // it, stay above classify()'s own (its ball is around T_D's corners):
  // every verdict here is one classify() also reaches (rt_cand_survey [80])
  const float cx = (e1x + e2x) / 3.0f, cy = (e1y + e2y) / 3.0f, cz = (e1z + e2z) / 3.0f;  // - v0
  float rv = sqrtf(cx * cx + cy * cy + cz * cz);  // max vertex distance from the centroid
  rv = fmaxf(rv, sqrtf((e1x - cx) * (e1x - cx) + (e1y - cy) * (e1y - cy) + (e1z - cz) * (e1z - cz)));
  rv = fmaxf(rv, sqrtf((e2x - cx) * (e2x - cx) + (e2y - cy) * (e2y - cy) + (e2z - cz) * (e2z - cz)));
  {
    float rq = (rv + h) * 1.0001f + 1e-6f + (float)p.dline;
    const float qx = cx - px, qy = cy - py, qz = cz - pz;  // centroid - pos
    const float R = sqrtf(qx * qx + qy * qy + qz * qz) * 0.99999f;
    if (R > 2.0f * rq) {
      const float rR = 1.0f / R;  // (one more rounding per quotient, inside the 1.00001 margins)
      const float st = rq * rR * 1.42f + 8.0f * fe + 1e-6f;
      const float d0 = fminf(1.0f, fabsf(qx) * rR + st) * 1.00001f;
      const float d1 = fminf(1.0f, fabsf(qy) * rR + st) * 1.00001f;
      const float d2 = fminf(1.0f, fabsf(qz) * rR + st) * 1.00001f;
      const float L = ((float)p.lmax + (float)p.dline) * 1.00001f, dl = (float)p.dline + 1e-6f;
      const float s0 = (L * d0 + fabsf(px) + dl) * 1.00001f;
      const float s1 = (L * d1 + fabsf(py) + dl) * 1.00001f;
      const float s2 = (L * d2 + fabsf(pz) + dl) * 1.00001f;
      const float a1x = fabsf(e1x), a1y = fabsf(e1y), a1z = fabsf(e1z);
      const float a2x = fabsf(e2x), a2y = fabsf(e2y), a2z = fabsf(e2z);
      const float M0 = d1 * a2z + d2 * a2y, M1 = d2 * a2x + d0 * a2z, M2 = d0 * a2y + d1 * a2x;
      const float N0 = s1 * a1z + s2 * a1y, N1 = s2 * a1x + s0 * a1z, N2 = s0 * a1y + s1 * a1x;
      const float cw = (float)(p.c_dot / 8.6 * 6.01) * fe * 1.0001f;
      const float ca = (float)(p.c_a / 7.2 * 5.01) * fe * 1.0001f;
      e_sh = fminf(e_sh, cw * (s0 * M0 + s1 * M1 + s2 * M2));
      e_dq = fminf(e_dq, cw * (d0 * N0 + d1 * N1 + d2 * N2));
      e_eq = fminf(e_eq, cw * (a2x * N0 + a2y * N1 + a2z * N2));
      e_a = fminf(e_a, ca * (a1x * M0 + a1y * M1 + a1z * M2));
      const float ck2 = fminf(1.0f, (amin + e_a) / (dmin * nlo) * 1.0001f);
      const float k2 = fmaxf(ck2 * H(ck2, a, rho), H(1.0f, a, rho)) * 1.0001f;
      const float num2 = deye_lb - (float)p.dline - k2 - 1e-5f * (deye + k2);
      if (num2 > 0.0f) cl = fmaxf(cl, num2 / (vmax + (float)p.dline) * 0.9999f);
      h = H(cl, a, rho);
    }
  }
  // the final reach from the corners' own displacements (the common bound
  // H alone measured lists 2.18 / 2.20 vs 1.97 / 1.96 ms on C5,
  // profiles/r08_quick_tight/, removed)
  h = Ht(cl, a, rho);
  const float rmax = vmax + h;
  const float derr = (e_eq / (a * (1.0f - rho)) + (rmax + (float)p.lmax) * (rho + 4.0f * fe) / (1.0f - rho) +
                      4.0f * fe * ((float)p.omax + rmax + (float)p.lmax)) * 1.0001f;
  if (h <= (float)p.eps_avail * 0.9999f && derr <= 2.0f * (float)p.eps_avail * 0.9999f) return Q_SAFE;
  // T_D lies in the ball (centroid, rv + h): every corner of T_D is within
  // H(cl) of its vertex.  The centroid in double from the record's floats.
  const double q[3] = {(double)r[0] + (double)cx, (double)r[1] + (double)cy, (double)r[2] + (double)cz};
  const double rb = ((double)rv + (double)h) * 1.001 + 1e-5 + 1e-6 * (fabs(q[0]) + fabs(q[1]) + fabs(q[2]));
  return rank_may_touch(p, q, rb) ? Q_LIST : Q_AWAY;
}

// Tiles of this rank whose camera samples can be candidates for the
// triangle.  Pixel (r, c) samples k in [W/2 - c, W/2 - c + 1/2], l in
// [H/2 - r, H/2 - r + 1/2] (cpu/raytracer.c:55-58 with i = W/2 - c, j = H/2 -
// r).
// Pixel rows [r0, r1] the footprint can reach; false: none.
__host__ __device__ inline bool raster_rows(const CandParams& p, const Footprint& fp, int& r0, int& r1) {
  r0 = 0;
  r1 = p.H - 1;
  if (fp.tri_ok && fp.hw0 < 0.0) {
    const double lmn = fmin(fp.l[0], fmin(fp.l[1], fp.l[2])) - fp.dimg;
    const double lmx = fmax(fp.l[0], fmax(fp.l[1], fp.l[2])) + fp.dimg;
    if (!(lmx >= p.lmin && lmn <= p.lmax_)) return false;
    pixel_range(p, lmn, lmx, r0, r1, true);
  }
  return r0 <= r1;
}

// The footprint's tiles in tile row ty (rows clipped to [r0, r1]): tile
// columns [a0, a1] and [b0, b1] (empty when a0 > a1; the second range only
// counts where it leaves the first).
__host__ __device__ inline void row_tiles(const CandParams& p, const Footprint& fp, int ty, int r0,
                                          int r1, int& a0, int& a1, int& b0, int& b1) {
  const double hh = (double)(p.H / 2);
  auto cols = [&](double a, double b, int& c0, int& c1) {  // k in [a, b] -> columns
    pixel_range(p, a, b, c0, c1, false);
  };
  // k-range of a band |b0 + b1 k + b2 l| <= hw for some l in [la, lb]
  auto band = [&](double hw, double la, double lb, double& a, double& b) {
    const double m = fmin(fp.b2 * la, fp.b2 * lb), M = fmax(fp.b2 * la, fp.b2 * lb);
    const double lo = -hw - fp.b0 - M, hi = hw - fp.b0 - m;  // b1 k in [lo, hi]
    if (fabs(fp.b1) < 1e-12) {
      if (lo <= 0.0 && hi >= 0.0) {
        a = -1e300;
        b = 1e300;
      } else {
        a = 1e300;
        b = -1e300;
      }
    } else if (fp.b1 > 0.0) {
      a = lo / fp.b1;
      b = hi / fp.b1;
    } else {
      a = hi / fp.b1;
      b = lo / fp.b1;
    }
  };
  const int ra = ty * 8 > r0 ? ty * 8 : r0, rb = ty * 8 + 7 < r1 ? ty * 8 + 7 : r1;
  // l-range of the strip's samples
  const double la = p.compat ? ra - hh : hh - rb, lb = p.compat ? rb - hh : hh - ra + 0.5;
  double a = -1e300, b = 1e300;
  if (fp.tri_ok) {  // the projected T_D cut to the (widened) strip
    const double la2 = la - fp.dimg, lb2 = lb + fp.dimg;
    double ta = 1e300, tb = -1e300;
    for (int i = 0; i < 3; i++) {
      if (fp.l[i] >= la2 && fp.l[i] <= lb2) {
        ta = fmin(ta, fp.k[i]);
        tb = fmax(tb, fp.k[i]);
      }
      const int j = (i + 1) % 3;
      const double ys[2] = {la2, lb2};
      for (int s = 0; s < 2; s++) {
        const double y = ys[s];
        if ((fp.l[i] - y) * (fp.l[j] - y) < 0.0) {
          const double t = (y - fp.l[i]) / (fp.l[j] - fp.l[i]);
          const double x = fp.k[i] + t * (fp.k[j] - fp.k[i]);
          ta = fmin(ta, x);
          tb = fmax(tb, x);
        }
      }
    }
    a = ta - fp.dimg;
    b = tb + fp.dimg;
  }
  double ba, bb;
  band(fp.hw, la, lb, ba, bb);
  a = fmax(a, ba);
  b = fmin(b, bb);
  int c0 = 1, c1 = 0, d0 = 1, d1 = 0;
  if (a <= b) cols(fmax(a, p.kmin - 1.0), fmin(b, p.kmax + 1.0), c0, c1);
  if (fp.hw0 >= 0.0) {
    band(fp.hw0, la, lb, ba, bb);
    if (ba <= bb) cols(fmax(ba, p.kmin - 1.0), fmin(bb, p.kmax + 1.0), d0, d1);
  }
  a0 = c0 <= c1 ? c0 >> 3 : 1;
  a1 = c0 <= c1 ? c1 >> 3 : 0;
  b0 = d0 <= d1 ? d0 >> 3 : 1;
  b1 = d0 <= d1 ? d1 >> 3 : 0;
}

// The footprint's tiles of this rank in tile row ty, in column order.
template <class F>
__host__ __device__ void raster_row(const CandParams& p, const Footprint& fp, int ty, int r0, int r1,
                                    F emit) {
  int a0, a1, b0, b1;
  row_tiles(p, fp, ty, r0, r1, a0, a1, b0, b1);
  auto put = [&](int tx) {
    uint32_t rk;
    const uint32_t t = rt_tile_local(tx, ty, (uint32_t)p.nranks, (uint32_t)p.blocks_x, (uint32_t)p.tb, &rk);
    if ((int)rk == p.rank) emit(t);
  };
  for (int tx = a0; tx <= a1; tx++) put(tx);
  for (int tx = b0; tx <= b1; tx++)
    if (!(tx >= a0 && tx <= a1)) put(tx);
}

// Number of tiles raster_row emits for row ty, without visiting them.
__host__ __device__ inline uint32_t count_row(const CandParams& p, const Footprint& fp, int ty, int r0,
                                              int r1) {
  int a0, a1, b0, b1;
  row_tiles(p, fp, ty, r0, r1, a0, a1, b0, b1);
  auto cnt = [&](int x0, int x1) { return rank_tiles(p, ty, x0, x1); };
  uint32_t c = cnt(a0, a1) + cnt(b0, b1);
  if (a0 <= a1 && b0 <= b1) c -= cnt(a0 > b0 ? a0 : b0, a1 < b1 ? a1 : b1);  // overlap counted once
  return c;
}

// raster_row's tiles of row ty as three disjoint column intervals, in
// emission order: x[0..1] = [a0, a1], then the parts of [b0, b1] left and
// right of it (x[2..3], x[4..5]; empty: x0 > x1); c[i] = this rank's tiles in
// interval i, f[i] = its first block column (rt_rank_row_tiles).  c[0] + c[1]
// + c[2] == count_row (the rank's tiles of a column set add up over disjoint
// parts).
__host__ __device__ inline void row_ivs(const CandParams& p, const Footprint& fp, int ty, int r0, int r1,
                                        int* x, int* f, uint32_t* c) {
  int a0, a1, b0, b1;
  row_tiles(p, fp, ty, r0, r1, a0, a1, b0, b1);
  x[0] = a0;
  x[1] = a1;
  if (a0 > a1) {
    x[2] = b0;
    x[3] = b1;
    x[4] = 1;
    x[5] = 0;
  } else {
    x[2] = b0;
    x[3] = b1 < a0 - 1 ? b1 : a0 - 1;
    x[4] = b0 > a1 + 1 ? b0 : a1 + 1;
    x[5] = b1;
  }
  for (int i = 0; i < 3; i++) {
    f[i] = 0;
    c[i] = x[2 * i] > x[2 * i + 1]
               ? 0u
               : rt_rank_row_tiles(ty, x[2 * i], x[2 * i + 1], (uint32_t)p.nranks, (uint32_t)p.rank,
                                   (uint32_t)p.blocks_x, (uint32_t)p.tb, &f[i]);
  }
}

// Tiles of this rank whose camera samples can be candidates for the
// triangle.  Pixel (r, c) samples k in [W/2 - c, W/2 - c + 1/2], l in
// [H/2 - r, H/2 - r + 1/2] (cpu/raytracer.c:55-58 with i = W/2 - c, j = H/2 -
// r).
template <class F>
__host__ __device__ void raster(const CandParams& p, const Footprint& fp, F emit) {
  int r0, r1;
  if (!raster_rows(p, fp, r0, r1)) return;
  for (int ty = r0 >> 3; ty <= (r1 >> 3); ty++) raster_row(p, fp, ty, r0, r1, emit);
}

// The number of tiles raster() emits, one step per tile row.
__host__ __device__ inline uint32_t raster_count(const CandParams& p, const Footprint& fp) {
  int r0, r1;
  if (!raster_rows(p, fp, r0, r1)) return 0;
  uint32_t n = 0;
  for (int ty = r0 >> 3; ty <= (r1 >> 3); ty++) n += count_row(p, fp, ty, r0, r1);
  return n;
}

// Per-tile refinement of a listed (prim, tile) entry.  classify() bounds the
// error region T_D once per triangle, over every camera line that can reach
// it: the smallest grazing cosine of any such line and the widest cone of
// directions.  The rays of one 8x8 tile have nearly one direction, so the
// same bound (tools/mt_bound.py, componentwise) evaluated with that tile's
// own |d_i|, |o_i - v0_i| and |a| gives a T_D of the tile's rays alone;
// false when the tile's samples, projected through the eye and widened by
// the camera lines' float deviation (classify's dimg), provably miss it (or
// no ray of the tile reaches |a| >= 1e-7).  true whenever unsure.
// The triangle's part (once per footprint; the big emission keeps it in LDS).
// With Y = P - pos for a point P = v0 + cu e1 + cv e2 of the triangle's
// plane, the homogeneous image point of P (classify's projection through the
// eye, H = (k0 yn + plane (g0 yu + g1 yv), l0 yn + plane (g1 yu + g2 yv), yn),
// yn / yu / yv = Y . n / u / v) is linear in (cu, cv): H = B0 + cu B1 + cv B2.
struct TileTri {
  double pv0[3];           // pos - v0
  double ae1[3], ae2[3];   // |e1_i|, |e2_i|
  double nl;               // |e1 x e2|
  double bcp, bcx, bcy;    // grazing offset (pos - o) . nh at tile (tx, ty): bcp - tx bcx - ty bcy
  double bw;               // its spread over a tile's rectangle
  double B[3][3];          // H of v0 - pos, e1, e2 (as points / directions)
  double ym[3];            // L1 norms of v0 - pos, e1, e2 (bounds of |Y|)
};
// The frame's part (CandParams' tile_* constants and the bound's terms).
struct TileFrame {
  double k00, l00, dk, dl, hk, hl, hd;
  double p00[3], du[3], dv[3], w[3];
  double dorig, cw, ca, gscale, dline, lmax;
};
RTC_FN void tile_frame(const CandParams& p, TileFrame& f) {
  f.k00 = p.tile_k00;
  f.l00 = p.tile_l00;
  f.dk = p.tile_dk;
  f.dl = p.tile_dl;
  f.hk = p.tile_hk;
  f.hl = p.tile_hl;
  f.hd = p.tile_hd;
  for (int a = 0; a < 3; a++) {
    f.p00[a] = p.tile_p00[a];
    f.du[a] = p.tile_du[a];
    f.dv[a] = p.tile_dv[a];
    f.w[a] = p.tile_w[a];
  }
  f.dorig = p.dorig;
  f.cw = p.c_dot / 8.6 * 6.01 * kEps;
  f.ca = p.c_a / 7.2 * 5.01 * kEps;
  f.gscale = p.gscale;
  f.dline = p.dline;
  f.lmax = p.lmax;
}
RTC_FN bool tile_tri(const CandParams& p, const float* r, TileTri& t) {
  double v0[3], e1[3], e2[3];
  for (int a = 0; a < 3; a++) {
    v0[a] = r[a];
    e1[a] = r[3 + a];
    e2[a] = r[6 + a];
    t.pv0[a] = p.pos[a] - v0[a];
    t.ae1[a] = fabs(e1[a]);
    t.ae2[a] = fabs(e2[a]);
  }
  const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  t.nl = norm3(n);
  if (!(t.nl > 0.0)) return false;
  const double inl = 1.0 / t.nl;
  const double nh[3] = {n[0] * inl, n[1] * inl, n[2] * inl};
  t.bcp = dot3(p.tile_p00, nh);
  t.bcx = dot3(p.tile_du, nh);
  t.bcy = dot3(p.tile_dv, nh);
  t.bw = fabs(dot3(p.u, nh)) * p.tile_hk + fabs(dot3(p.v, nh)) * p.tile_hl;
  const double* V[3] = {t.pv0, e1, e2};
  for (int k = 0; k < 3; k++) {
    const double sgn = k == 0 ? -1.0 : 1.0;  // v0 - pos = -(pos - v0)
    const double yn = sgn * dot3(V[k], p.n), yu = sgn * dot3(V[k], p.u), yv = sgn * dot3(V[k], p.v);
    t.B[k][0] = p.k0 * yn + p.plane * (p.ginv[0] * yu + p.ginv[1] * yv);
    t.B[k][1] = p.l0 * yn + p.plane * (p.ginv[1] * yu + p.ginv[2] * yv);
    t.B[k][2] = yn;
    t.ym[k] = fabs(V[k][0]) + fabs(V[k][1]) + fabs(V[k][2]);
  }
  return true;
}

// The tile's part.  Division-light (the big emission runs it per entry, in
// f64): the affine quantities' extremes over the tile's sample rectangle in
// closed form (|f_c| + |f_k| hk + |f_l| hl), and T_D's projection tested in
// homogeneous image coordinates (no per-corner division).
RTC_FN bool tile_keep(const TileFrame& p, const TileTri& t, int tx, int ty) {
  // the tile's sample rectangle [kc -+ hk] x [lc -+ hl] (pixel_range's
  // inverse, CandParams::tile_*), its centre o_c = C + kc u + lc v, and per
  // axis max |pos_i - o_i| and max |o_i - v0_i| over it
  // (fused multiply-adds throughout: these are bounds of our own, each
  // rounding far inside their margins, and fma is exact IEEE on host and device)
  const double dtx = (double)tx, dty = (double)ty;
  const double kc = fma(dtx, p.dk, p.k00), lc = fma(dty, p.dl, p.l00);
  double pm[3], sm[3], po[3];
  for (int a = 0; a < 3; a++) {
    po[a] = fma(-dtx, p.du[a], fma(-dty, p.dv[a], p.p00[a]));  // pos - o_c
    pm[a] = fabs(po[a]) + p.w[a];
    sm[a] = (fabs(t.pv0[a] - po[a]) + p.w[a] + p.dorig) * (1.0 + 1e-9);
  }
  // |pos - o| within the centre's +- the tile's half diagonal (hk |u| + hl |v|)
  const double rc = sqrt(fma(po[0], po[0], fma(po[1], po[1], po[2] * po[2])));
  const double rmn = rc - p.hd - p.dorig, rmx = (rc + p.hd + p.dorig) * (1.0 + 1e-9);
  if (!(rmn > 1e-6)) return true;
  const double irn = 1.0 / rmn;
  // float origins within dorig, float directions within a few eps of pos - o
  double dm[3];
  for (int a = 0; a < 3; a++) dm[a] = fmin(1.0, fma(pm[a] + p.dorig, irn, 8.0 * kEps)) * kDMax;
  double M[3], N[3];
  for (int i = 0; i < 3; i++) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    M[i] = fma(dm[j], t.ae2[k], dm[k] * t.ae2[j]);
    N[i] = fma(sm[j], t.ae1[k], sm[k] * t.ae1[j]);
  }
  // the componentwise bounds alone (each of them and classify's Cauchy-Schwarz
  // ones is a bound on its own; for a tile's narrow cone these are the
  // smaller)
  const double cw = p.cw, ca = p.ca;
  auto dotf = [](const double* a, const double* b) { return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2])); };
  const double e_sh = cw * dotf(sm, M);
  const double e_dq = cw * dotf(dm, N);
  const double e_a = ca * dotf(t.ae1, M);
  // grazing cosine of the tile's rays: |b| over the rectangle is in [bl, bh]
  const double bc = fma(-dtx, t.bcx, fma(-dty, t.bcy, t.bcp));
  const double bl = fmax(0.0, fabs(bc) - t.bw), bh = fabs(bc) + t.bw;
  const double cmax = fmin(1.0, fma(bh + p.dorig, irn, 8.0 * kEps));
  if (kDMax * t.nl * cmax + e_a < kAMin) return false;  // |a| < 1e-7 for every ray of the tile
  // a_lb = max(kAMin, dmin nl cmin - e_a), cmin = (bl - dorig) / rmx - 8 eps,
  // kept as the fraction num / rmx; rho = e_a / a_lb < 1/2 <=> 2 e_a < a_lb
  const double num = fma(kDMin * t.nl, bl - p.dorig - 8.0 * kEps * rmx, -e_a * rmx);
  const bool clamp = !(num > kAMin * rmx);
  if (clamp ? !(2.0 * e_a < kAMin) : !(2.0 * e_a * rmx < num)) return true;
  // 1 / (a_lb (1 - rho)) = 1 / (a_lb - e_a): du = e_sh / (a_lb - e_a), and
  // dw = (4 eps + (e_sh + e_dq) / a_lb + rho) / (1 - rho)
  //    = 4 eps / (1 - rho) + (e_sh + e_dq + e_a) / (a_lb - e_a)
  //   <= 8 eps + (e_sh + e_dq + e_a) / (a_lb - e_a)
  const double iq = clamp ? 1.0 / (kAMin - e_a) : rmx / fma(-e_a, rmx, num);
  const double du = e_sh * iq, dv = e_dq * iq;
  const double dw = fma(e_sh + e_dq + e_a, iq, 8.0 * kEps);
  // T_D's corners (cu, cv) and their homogeneous image points H_k = B0 + cu
  // B1 + cv B2 ~ (K_k, L_k, 1): classify's lam = plane / yn, without dividing
  const double cu[3] = {-du, 1.0 + dw + dv, -du}, cv[3] = {-dv, -dv, 1.0 + dw + du};
  double H[3][3], ymag = 1.0, ylo = 1e300, yhi = -1e300;
  for (int k = 0; k < 3; k++) {
    for (int c = 0; c < 3; c++) H[k][c] = fma(cu[k], t.B[1][c], fma(cv[k], t.B[2][c], t.B[0][c]));
    ymag = fmax(ymag, fma(fabs(cu[k]), t.ym[1], fma(fabs(cv[k]), t.ym[2], t.ym[0])));
    ylo = fmin(ylo, H[k][2]);
    yhi = fmax(yhi, H[k][2]);
  }
  // every corner strictly on one side of the eye plane; the nearest point of
  // T_D is then at least min |yn| from the eye
  if (!(ylo > 1e-6 * ymag || yhi < -1e-6 * ymag)) return true;
  const double sg = ylo > 0.0 ? 1.0 : -1.0, rlo = fmin(fabs(ylo), fabs(yhi));
  const double dimg = 1.5 * p.gscale * (p.dline * (1.0 + p.lmax / rlo) + p.dorig) + 1e-3;
  const double x0 = kc - p.hk - dimg, x1 = kc + p.hk + dimg;
  const double y0 = lc - p.hl - dimg, y1 = lc + p.hl + dimg;
  // separating axes: the rectangle's (K_k < x0 <=> sg H_k0 < sg x0 yn_k, ...)
  {
    bool lx = true, gx = true, ly = true, gy = true;
    for (int k = 0; k < 3; k++) {
      const double hx = sg * H[k][0], hy = sg * H[k][1], w = sg * H[k][2];  // w > 0
      const double tx0 = 1e-9 * (fabs(hx) + fabs(x0) * w), tx1 = 1e-9 * (fabs(hx) + fabs(x1) * w);
      const double ty0 = 1e-9 * (fabs(hy) + fabs(y0) * w), ty1 = 1e-9 * (fabs(hy) + fabs(y1) * w);
      lx = lx && hx < x0 * w - tx0;
      gx = gx && hx > x1 * w + tx1;
      ly = ly && hy < y0 * w - ty0;
      gy = gy && hy > y1 * w + ty1;
    }
    if (lx || gx || ly || gy) return false;
  }
  // and the triangle's edges: q = (x, y, 1) lies outside edge e -> f when
  // det[H_e; H_f; q] has the sign opposite to det[H_0; H_1; H_2] sg
  double c01[3], c12[3], c20[3];
  auto cross3 = [](const double* a, const double* b, double* c) {
    c[0] = fma(a[1], b[2], -a[2] * b[1]);
    c[1] = fma(a[2], b[0], -a[0] * b[2]);
    c[2] = fma(a[0], b[1], -a[1] * b[0]);
  };
  cross3(H[0], H[1], c01);
  cross3(H[1], H[2], c12);
  cross3(H[2], H[0], c20);
  const double orient = dotf(H[2], c01) * sg;
  if (orient == 0.0) return true;
  const double so = orient > 0.0 ? 1.0 : -1.0;
  const double* C3[3] = {c01, c12, c20};
  for (int e = 0; e < 3; e++) {
    const double cx = so * C3[e][0], cy = so * C3[e][1], cz = so * C3[e][2];
    const double mx = fmax(cx * x0, cx * x1) + fmax(cy * y0, cy * y1) + cz;  // largest over the rectangle
    const double tol = 1e-9 * (fabs(cx) * fmax(fabs(x0), fabs(x1)) + fabs(cy) * fmax(fabs(y0), fabs(y1)) + fabs(cz));
    if (mx < -tol) return false;
  }
  return true;
}

RTC_FN bool tile_keep(const CandParams& p, const float* r, int tx, int ty) {
  TileTri t;
  TileFrame f;
  tile_frame(p, f);
  return !tile_tri(p, r, t) || tile_keep(f, t, tx, ty);
}

// A footprint is "big" -- counted and emitted by one wave, its tile rows
// spread over the lanes -- when it spans more than kSmallRows tile rows or
// has more than kSmallEntries entries; the others are counted and emitted by
// one thread each.  (A thread per footprint of hundreds of entries stalled
// its whole wave: count 2.6 ms, emit 1.4 ms on C5 before the split.)
constexpr int kSmallRows = 2;
constexpr uint32_t kSmallEntries = 32;

// The footprints whose entries are refined per tile (CandParams::refine):
// those spanning more than kSmallRows tile rows of the frame.  A property of
// the footprint alone, not of a rank's share of its tiles, so a rank's own
// lists and the triangle-parallel build (one whole-frame rank) refine the same
// entries; all of them are big footprints (the big passes emit them).
__host__ __device__ inline bool refined_rows(int r0, int r1) { return (r1 >> 3) - (r0 >> 3) + 1 > kSmallRows; }
__host__ __device__ inline bool refined_footprint(const CandParams& p, const Footprint& fp) {
  int r0, r1;
  return raster_rows(p, fp, r0, r1) && refined_rows(r0, r1);
}

}  // namespace rtc
