// rt_lightbuf_host.cpp -- the light buffers' host side that needs no device:
// a light's build parameters from the scene's extent (lb_fill), the grid and
// the geometry parameters every build and every survey starts from
// (lb_derive_grid, lb_geom_host) and the host survey of a build
// (rt_lightbuf_survey_host).  Plain C++: it runs the same footprint code as
// the device build (rt_lightbuf_geom.h) and makes no HIP call, so a
// stand-alone program can link it with host/rt_error.c alone
// (tests/native/lightbuf_geom.cpp).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rt_lightbuf_geom.h"

extern "C" {
#include "../host/rt_cull.h"
}

// The build's geometry (shared by the device build and the host survey): the
// DIR grid's float axes and extent, the POINT cube map's side.  1 with err
// filled: no grid (a zero directional vector, a non-finite vector, too many
// cells).
int lb_derive_grid(const LBParams* in, rtl::LbGeom& p, RtLightBuf* out, uint64_t& ncell, char* err, size_t errlen) {
  using namespace rtl;
  std::memset(&p, 0, sizeof p);
  std::memset(out, 0, sizeof *out);
  p.tri = in->tri;
  p.nprim = in->nprim;
  p.kind = in->kind;
  p.proven = in->proven ? 1u : 0u;
  for (int a = 0; a < 3; a++) {
    p.lv[a] = in->lv[a];
    p.olo[a] = in->box_lo[a];
    p.ohi[a] = in->box_hi[a];
  }
  p.slack = in->slack;
  p.s1 = in->s1;
  p.dmax = in->dmax;
  if (!(std::isfinite(in->lv[0]) && std::isfinite(in->lv[1]) && std::isfinite(in->lv[2]))) {
    // an infinite direction would give a one-cell grid with NaN axes, a NaN
    // position a NaN cell coordinate in the query (rt_lightbuf_cell.h)
    snprintf(err, errlen, "light with a non-finite vector");
    return 1;  // no buffer, like the zero vector
  }
  if (in->kind == RT_LB_DIR) {
    // axes: w = normalize(-l.v) (the rays' direction), u, v completing it;
    // rounded to float once -- the build and the query use the same floats
    double w[3] = {-in->lv[0], -in->lv[1], -in->lv[2]};
    const double wl = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (!(wl > 0.0)) {
      snprintf(err, errlen, "directional light with a zero vector");
      return 1;  // no grid: its queries walk (the walk takes any direction)
    }
    for (int a = 0; a < 3; a++) {
      p.d[a] = (double)(float)(-in->lv[a]);  // the rays' direction, exactly (cpu/light.c:53)
      w[a] /= wl;
    }
    p.dlen = sqrt(p.d[0] * p.d[0] + p.d[1] * p.d[1] + p.d[2] * p.d[2]);
    int m = 0;
    for (int a = 1; a < 3; a++)
      if (fabs(w[a]) < fabs(w[m])) m = a;
    double e[3] = {0, 0, 0}, u[3], v[3];
    e[m] = 1.0;
    cross3d(w, e, u);
    const double ul = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    for (int a = 0; a < 3; a++) u[a] /= ul;
    cross3d(w, u, v);
    for (int a = 0; a < 3; a++) {
      out->u[a] = (float)u[a];
      out->v[a] = (float)v[a];
      out->w[a] = (float)w[a];
      p.u[a] = out->u[a];
      p.v[a] = out->v[a];
      p.w[a] = out->w[a];
    }
    {
      double su = 0.0, sv = 0.0;
      for (int a = 0; a < 3; a++) {
        su += p.u[a] * p.d[a] / p.dlen;
        sv += p.v[a] * p.d[a] / p.dlen;
      }
      p.skew = (fmax(fabs(su), fabs(sv)) + 1e-15) * 1.01;
    }
    // grid over the projected scene box (in->lv unused beyond the axes)
    const double m0 = in->slack + 3.0 * kEps * in->s1 * 1.01 + 1e-9 * in->s1;
    double lu = 1e300, hu = -1e300, lv2 = 1e300, hv2 = -1e300;
    for (int c = 0; c < 8; c++) {
      const double X[3] = {(c & 1) ? in->box_hi[0] : in->box_lo[0], (c & 2) ? in->box_hi[1] : in->box_lo[1],
                           (c & 4) ? in->box_hi[2] : in->box_lo[2]};
      const double a = X[0] * p.u[0] + X[1] * p.u[1] + X[2] * p.u[2];
      const double b = X[0] * p.v[0] + X[1] * p.v[1] + X[2] * p.v[2];
      lu = fmin(lu, a);
      hu = fmax(hu, a);
      lv2 = fmin(lv2, b);
      hv2 = fmax(hv2, b);
    }
    lu -= 2.0 * m0;
    lv2 -= 2.0 * m0;
    hu += 2.0 * m0;
    hv2 += 2.0 * m0;
    const double A = (hu - lu) * (hv2 - lv2);
    double cs = sqrt(A / (double)(in->target_cells ? in->target_cells : 1u));
    if (!(cs > 0.0)) cs = 1.0;
    p.nx = (uint32_t)fmin(16384.0, ceil((hu - lu) / cs) + 1.0);
    p.ny = (uint32_t)fmin(16384.0, ceil((hv2 - lv2) / cs) + 1.0);
    cs = fmax(cs, fmax((hu - lu) / (p.nx - 1), (hv2 - lv2) / (p.ny - 1)));
    out->u0 = (float)lu;
    out->v0 = (float)lv2;
    out->inv_cs = (float)(1.0 / cs);
    p.u0 = out->u0;
    p.v0 = out->v0;
    p.inv_cs = out->inv_cs;  // the float the query multiplies by
    p.cs = 1.0 / p.inv_cs;
    out->nx = p.nx;
    out->ny = p.ny;
    ncell = (uint64_t)p.nx * p.ny;
  } else {
    uint32_t n = (uint32_t)ceil(sqrt((double)(in->target_cells ? in->target_cells : 6u) / 6.0));
    if (n < 1) n = 1;
    if (n > 8192) n = 8192;
    p.n = n;
    out->nx = out->ny = n;
    out->half_n = 0.5f * (float)n;
    ncell = 6ull * n * n;
  }
  out->kind = in->kind;
  out->proven = p.proven;
  for (int a = 0; a < 3; a++) {  // rounded inward: a float inside is inside the build's box
    float lo = (float)in->box_lo[a], hi = (float)in->box_hi[a];
    if ((double)lo < in->box_lo[a]) lo = std::nextafter(lo, 3.0e38f);
    if ((double)hi > in->box_hi[a]) hi = std::nextafter(hi, -3.0e38f);
    out->olo[a] = lo;
    out->ohi[a] = hi;
  }
  if (ncell >= (1ull << 31)) {
    snprintf(err, errlen, "light buffer of %llu cells", (unsigned long long)ncell);
    return 1;
  }
  return 0;
}

// The whole geometry of a build on the host (in->tri = host records): the
// grid, and for a proven point light the nearest shadow-ray origin.
int lb_geom_host(const LBParams* in, rtl::LbGeom& p, RtLightBuf* lb, uint64_t& ncell, char* err, size_t errlen) {
  using namespace rtl;
  if (const int r = lb_derive_grid(in, p, lb, ncell, err, errlen)) return r;
  if (p.proven && p.kind == RT_LB_POINT) {
    double m = 1e300;
    for (uint32_t i = 0; i < p.nprim; i++) m = fmin(m, prim_rmin(p, i));
    p.rmin_o = p.nprim ? (double)(float)m : 0.0;
    if (p.rmin_o > m) p.rmin_o = std::nextafter((float)m, 0.0f);  // rounded down, as the device does
  }
  return 0;
}

// Host survey of a build (tests, tools; no device): the same footprints,
// counted on the CPU for every stride-th prim of in->tri (HOST prim-order
// records) into the slots of RtLbSurvey (rt_lightbuf.h).
extern "C" int rt_lightbuf_survey_host(const LBParams* in, uint32_t stride, unsigned long long out[RT_LBS_WORDS],
                                       char* err, size_t errlen) {
  using namespace rtl;
  LbGeom p;
  RtLightBuf lb;
  uint64_t ncell = 0;
  if (lb_geom_host(in, p, &lb, ncell, err, errlen)) return -1;
  for (uint32_t k = 0; k < RT_LBS_WORDS; k++) out[k] = 0;
  if (!stride) stride = 1;
  for (uint32_t prim = 0; prim < p.nprim; prim += stride) {
    Foot f;
    footprint(p, prim, f);
    out[RT_LBS_PRIMS]++;
    if (f.never) {
      out[RT_LBS_NEVER]++;
      continue;
    }
    if (f.global) {
      out[RT_LBS_GLOBAL]++;
      continue;
    }
    if (f.band) out[RT_LBS_BAND]++;
    if (foot_is_big(p, f)) out[RT_LBS_BIG]++;
    const uint32_t rows = foot_rows(p, f);
    uint64_t c = 0;
    for (uint32_t r = 0; r < rows; r++) {
      const uint32_t e = row_entries<false>(p, f, prim, r, 0, 0);
      c += e;
      if (f.band && r >= rows - 6u * p.n) out[RT_LBS_BAND_ENTRIES] += e;
    }
    out[RT_LBS_ENTRIES] += c;
    if (c > 1024) out[RT_LBS_ENTRIES_OVER_1024] += c;
    if (c > 64 && c <= 1024) out[RT_LBS_ENTRIES_65_1024] += c;
    if (c > 64) out[RT_LBS_PRIMS_OVER_64]++;
    if (c > out[RT_LBS_MAX_COUNT]) {
      out[RT_LBS_MAX_COUNT] = c;
      out[RT_LBS_MAX_PRIM] = prim;
    }
  }
  return 0;
}

// The build parameters of one light's buffer for a scene of nprim triangles
// in the box (scene_c, scene_r) and the culling slack eps_ulps.
void lb_fill(LBParams& lp, const float scene_c[3], float scene_r, const float aabb_lo[3],
                    const float aabb_hi[3], float eps_ulps, uint32_t type, const float lv[3], uint32_t nprim,
                    int proven) {
  std::memset(&lp, 0, sizeof lp);
  // a shadow ray leaves a hit point: inside the scene cube up to the float
  // error of the hit, so its slack eps(o) (host/rt_cull.h, float) is at most
  const double R = scene_r, eps_rel = (double)(eps_ulps * kSlackUnit);
  const double cmag = std::fmax(std::fabs(scene_c[0]), std::fmax(std::fabs(scene_c[1]), std::fabs(scene_c[2])));
  const double slack = (eps_rel * (2.0 * R * 1.001 + 1e-3) + (double)RT_CULL_PLANE * (cmag + R) + 1e-6) * 1.01;
  double lo[3], hi[3], s1 = 0.0;
  for (int a = 0; a < 3; a++) {
    if (proven) {
      // the proof's origin box: the triangles' box grown by 1 + 1 % of the
      // scene (hit points off it -- float garbage hits beyond that -- are
      // counted by the shade pass, never assumed)
#ifndef RT_LB_PROOF_BOX
#define RT_LB_PROOF_BOX 1.0  // the proof box: the triangles' box grown by g = RT_LB_PROOF_BOX (1 + 0.02 R)
#endif
      const double g = RT_LB_PROOF_BOX * (1.0 + 0.02 * R);
      lo[a] = (double)aabb_lo[a] - g;
      hi[a] = (double)aabb_hi[a] + g;
    } else {
      lo[a] = scene_c[a] - R * 1.001 - 1e-3;
      hi[a] = scene_c[a] + R * 1.001 + 1e-3;
    }
    s1 += std::fmax(std::fabs(lo[a]), std::fabs(hi[a]));
  }
  lp.nprim = nprim;
  lp.kind = type == 1 ? RT_LB_DIR : RT_LB_POINT;
  double dmax = 0.0;
  for (int a = 0; a < 3; a++) {
    lp.lv[a] = lv[a];
    lp.box_lo[a] = lo[a];
    lp.box_hi[a] = hi[a];
  }
  for (int k = 0; k < 8; k++) {
    double d2 = 0.0;
    for (int a = 0; a < 3; a++) {
      const double x = ((k >> a) & 1 ? hi[a] : lo[a]) - lp.lv[a];
      d2 += x * x;
    }
    dmax = std::fmax(dmax, std::sqrt(d2));
  }
  lp.slack = slack;
  lp.s1 = s1;
  lp.dmax = dmax * 1.01 + 1.0;
  // two cells per triangle: C5 shade 1.97 -> 1.93 ms against one (half: 2.12,
  // four: 2.09; 117 M -> 172 M proven entries, 8 GB; profiles/r05x_tuning/)
  const uint64_t cells = 2ull * nprim;
  lp.target_cells = cells < 4096u ? 4096u : (cells > (1u << 25) ? (1u << 25) : (uint32_t)cells);
  lp.proven = proven ? 1u : 0u;
}
