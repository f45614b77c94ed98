// rt_cand_host.cpp -- the candidate lists' host side that needs no device:
// the frame constants every build and every mirror starts from (cand_params)
// and the host mirrors of the proof geometry (rt_cand_survey_host,
// rt_cand_refine_sample_host, rt_cand_verify_host).  Plain C++: it runs the
// same classify / raster / tile_keep code as the device passes
// (rt_cand_geom.h) and launches nothing, so a stand-alone program can link
// it with host/rt_error.c alone (tests/native/cand_geom.cpp).  Knows nothing
// of the device context (rt_ctx.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "rt_cand_geom.h"

extern "C" {
#include "../host/rt_cull.h"
#include "../host/rt_internal.h"
}

static double d3dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// Frame constants of the candidate lists for rank/nranks (no device work).
int cand_params(const rt_frame* f, const float scene_c[3], float scene_r, float eps_ulps,
                       double bound_scale, int rank, int nranks, CandParams* out, int compat) {
  const double eps = 0x1p-24;
  CandParams& cp = *out;
  std::memset(&cp, 0, sizeof cp);
  const double pos[3] = {f->position.x, f->position.y, f->position.z};
  const double u[3] = {f->u.x, f->u.y, f->u.z}, v[3] = {f->v.x, f->v.y, f->v.z};
  const double C[3] = {f->C.x, f->C.y, f->C.z};
  double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const double nn = std::sqrt(d3dot(n, n));
  if (!(nn > 1e-6)) return rt_set_error(RT_EINVAL, "degenerate camera (u parallel to v)");
  for (int a = 0; a < 3; a++) {
    cp.pos[a] = pos[a];
    cp.u[a] = u[a];
    cp.v[a] = v[a];
    cp.C[a] = C[a];
    cp.n[a] = n[a] / nn;
  }
  const double cpos[3] = {C[0] - pos[0], C[1] - pos[1], C[2] - pos[2]};
  cp.plane = d3dot(cpos, cp.n);
  if (!(std::fabs(cp.plane) > 1e-6)) return rt_set_error(RT_EINVAL, "degenerate camera (L = 0)");
  const double g00 = d3dot(u, u), g01 = d3dot(u, v), g11 = d3dot(v, v);
  const double det = g00 * g11 - g01 * g01;
  cp.ginv[0] = g11 / det;
  cp.ginv[1] = -g01 / det;
  cp.ginv[2] = g00 / det;
  cp.gscale = std::sqrt(cp.ginv[0] * cp.ginv[0] + 2 * cp.ginv[1] * cp.ginv[1] + cp.ginv[2] * cp.ginv[2]);
  {
    const double pc[3] = {-cpos[0], -cpos[1], -cpos[2]};
    const double pu = d3dot(pc, u), pv = d3dot(pc, v);
    cp.k0 = cp.ginv[0] * pu + cp.ginv[1] * pv;
    cp.l0 = cp.ginv[1] * pu + cp.ginv[2] * pv;
  }
  // a tile's sample rectangle (rt_cand_geom.h tile_keep): cpu/rt's samples k in
  // [W/2 - c, W/2 - c + 1/2] for the tile's columns c = 8 tx .. 8 tx + 7, so
  // centre W/2 - 8 tx - 3.25 and half side 3.75 (likewise l); compatibility
  // mode: k = c - W/2, centre 8 tx + 3.5 - W/2, half side 3.5
  {
    const double hw = (double)(f->width / 2), hh = (double)(f->height / 2);
    cp.tile_hk = cp.tile_hl = compat ? 3.5 : 3.75;
    cp.tile_k00 = compat ? 3.5 - hw : hw - 3.25;
    cp.tile_l00 = compat ? 3.5 - hh : hh - 3.25;
    cp.tile_dk = cp.tile_dl = compat ? 8.0 : -8.0;
    for (int a = 0; a < 3; a++) {
      cp.tile_p00[a] = pos[a] - (C[a] + cp.tile_k00 * u[a] + cp.tile_l00 * v[a]);
      cp.tile_du[a] = cp.tile_dk * u[a];
      cp.tile_dv[a] = cp.tile_dl * v[a];
      cp.tile_w[a] = std::fabs(u[a]) * cp.tile_hk + std::fabs(v[a]) * cp.tile_hl;
    }
    cp.tile_hd = (cp.tile_hk * std::sqrt(d3dot(u, u)) + cp.tile_hl * std::sqrt(d3dot(v, v))) * (1.0 + 1e-12);
  }
  const int W = f->width, H = f->height;
  cp.compat = compat;
  if (compat) {
    // gpu/rt: one sample per pixel of the 3x frame, k = px - W/2, px in
    // [0, W - 1] (gpu/raytracer.cu:97-103), likewise l
    cp.kmin = -(double)(W / 2);
    cp.kmax = (double)(W - 1 - W / 2);
    cp.lmin = -(double)(H / 2);
    cp.lmax_ = (double)(H - 1 - H / 2);
  } else {
    // samples: k = i + {0, 1/2}, i in [1 - W/2, W/2] (cpu/raytracer.c:50-58)
    cp.kmin = 1.0 - W / 2;
    cp.kmax = W / 2 + 0.5;
    cp.lmin = 1.0 - H / 2;
    cp.lmax_ = H / 2 + 0.5;
  }
  double lmax = 0, omax = 0;
  for (int ci = 0; ci < 4; ci++) {  // |o - pos| and |o| are convex: corners bound them
    const double k = (ci & 1) ? cp.kmax : cp.kmin, l = (ci & 2) ? cp.lmax_ : cp.lmin;
    double o[3], d[3];
    for (int a = 0; a < 3; a++) {
      o[a] = C[a] + u[a] * k + v[a] * l;
      d[a] = o[a] - pos[a];
    }
    lmax = std::fmax(lmax, std::sqrt(d3dot(d, d)));
    omax = std::fmax(omax, std::sqrt(d3dot(o, o)));
  }
  cp.lmax = lmax * (1 + 1e-9) + 1e-9;
  cp.omax = omax * (1 + 1e-9) + 1e-9;
  // float camera line (o_f, normalize(pos - o_f)): within 2.5 eps rad of the
  // direction towards pos, so within dline of pos; o_f within dorig of o
  cp.dline = 6.0 * eps * cp.lmax + 1e-12;
  cp.dorig = 8.0 * eps * (std::sqrt(d3dot(C, C)) + std::fabs(cp.kmin) + cp.kmax + std::fabs(cp.lmin) +
                          cp.lmax_) * 1.8;
  // smallest culling slack of a camera ray: rt_cull_eps with the max-norm
  // |o - c| bounded below per axis over the sample rectangle
  double mlb = 0;
  for (int a = 0; a < 3; a++) {
    double lo = 1e300, hi = -1e300;
    for (int ci = 0; ci < 4; ci++) {
      const double k = (ci & 1) ? cp.kmax : cp.kmin, l = (ci & 2) ? cp.lmax_ : cp.lmin;
      const double x = C[a] + u[a] * k + v[a] * l - scene_c[a];
      lo = std::fmin(lo, x);
      hi = std::fmax(hi, x);
    }
    const double m = (lo <= 0 && hi >= 0) ? 0.0 : std::fmin(std::fabs(lo), std::fabs(hi));
    mlb = std::fmax(mlb, m);
  }
  const double R = scene_r;
  const double cmag = std::fmax(std::fabs(scene_c[0]), std::fmax(std::fabs(scene_c[1]),
                                                                std::fabs(scene_c[2])));
  const double eps_rel = (double)(eps_ulps * kSlackUnit);
  const double eps_min = (eps_rel * (std::fmax(mlb - cp.dorig, 0.0) + R) +
                          (double)RT_CULL_PLANE * (cmag + R) + 1e-6) * (1.0 - 1e-5);
  // the slab test's own rounding (rt_cull.h: a few ulps of |o| and of |t d|)
  // takes 4 ulps of |o| + the scene's extent out of that slack
  cp.eps_avail = eps_min - 8.0 * eps * (cp.omax + 2.0 * (cmag + R));
  // tools/mt_bound.py: C_DOT = 6 sqrt 2 -> 8.6, C_A = 5 sqrt 2 -> 7.2 (scale 1 = the proven bound)
  cp.c_dot = 8.6 * bound_scale;
  cp.c_a = 7.2 * bound_scale;
  cp.W = W;
  cp.H = H;
  cp.tiles_x = tiles_x_of(W);
  cp.tiles_y = tiles_y_of(H);
  cp.rank = rank;
  cp.nranks = nranks;
  cp.tb = rt_block_side(nranks);
  cp.blocks_x = rt_blocks_x(cp.tiles_x, cp.tb);
  cp.ntiles_local = rank_tile_count(W, H, rank, nranks);
  return RT_OK;
}

extern "C" int rt_cand_survey_host(const CandParams* p, const float* tri, const float* node,
                                   const uint32_t* prim_leaf, int threads,
                                   unsigned long long out[88]) {
  // out: [0] safe, [1] footprint, [2] global, [3] entries, [4 + k] prims
  // with 2^k <= entries < 2^(k+1), [20 + k] their entries (k < 16);
  // [36 + k] footprint prims whose T_D box (grown by the distance error
  // beyond the pruning margin) reaches beyond the triangle's own box by
  // g with 2^(k-8) <= g / eps_avail < 2^(k-7) (k = 0: below 2^-7; k = 15:
  // 2^7 and more, or unbounded), [52 + k] their entries
  // [71..77]: quick_class's verdicts (listed; of those classify() SAFE
  // through the leaf box, SAFE otherwise, FOOTPRINT without a tile, GLOBAL;
  // Q_SAFE; Q_AWAY); [78] / [79] listed and SAFE by the reach / steepness
  // exits; [80] Q_SAFE that classify() does not confirm
  for (int k = 0; k < 88; k++) out[k] = 0;
  if (threads < 1) threads = 1;
  std::vector<unsigned long long> part(88 * (size_t)threads, 0);
  std::vector<unsigned long long> bad((size_t)threads, 0);
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++)
    th.emplace_back([&, t]() {
      unsigned long long* o = &part[88 * (size_t)t];
      for (uint32_t i = (uint32_t)t; i < p->nprim; i += (uint32_t)threads) {
        rtc::Footprint fp;
        const float* lb = prim_leaf ? node + 8 * (size_t)prim_leaf[i] : nullptr;
        double td[18];
        const float* rec = tri + 12 * (size_t)i;
        const int c = rtc::classify(*p, rec, lb, fp, td);
        o[c]++;
        const int qc = rtc::quick_class(*p, rec);
        if (qc == rtc::Q_LIST) {
          o[71]++;
          if (c == rtc::SAFE) {
            rtc::Footprint f2;
            int why = -1;
            o[rtc::classify(*p, rec, nullptr, f2, nullptr, &why) == rtc::SAFE ? 73 : 72]++;
            if (why == 1) o[78]++;  // the error region within the slack
            if (why == 3) o[79]++;  // no candidate line steep enough to be accepted
          } else if (c == rtc::GLOBAL) {
            o[75]++;
          }
        } else {
          o[qc == rtc::Q_SAFE ? 76 : 77]++;
          if (qc == rtc::Q_SAFE && c != rtc::SAFE) o[80]++;  // the fast path's proof must hold
        }
        if (c == rtc::FOOTPRINT) {
          unsigned long long v = 0, kept = 0;
          rtc::raster(*p, fp, [&](uint32_t tl) {
            v++;
            int tx, ty;
            rt_tile_xy(tl, (uint32_t)p->rank, (uint32_t)p->nranks, (uint32_t)p->blocks_x, (uint32_t)p->tb, &tx, &ty);
            kept += rtc::tile_keep(*p, rec, tx, ty) ? 1u : 0u;
          });
          if (rtc::refined_footprint(*p, fp)) {  // the device refines these (CandParams::refine)
            o[68] += kept;
            o[69] += v;
            o[70] += kept;
          } else {
            o[68] += v;
          }
          // big_count_kernel counts rows through row_ivs (big_item_kernel's intervals)
          unsigned long long vi = 0;
          int q0, q1;
          if (rtc::raster_rows(*p, fp, q0, q1))
            for (int ty = q0 >> 3; ty <= (q1 >> 3); ty++) {
              int x[6], fb[3];
              uint32_t cn[3];
              rtc::row_ivs(*p, fp, ty, q0, q1, x, fb, cn);
              vi += cn[0] + cn[1] + cn[2];
            }
          if (v != rtc::raster_count(*p, fp) || vi != v) bad[t]++;  // the device count pass must agree
          o[3] += v;
          if (!v && qc == rtc::Q_LIST) o[74]++;
          int k = 0;
          while (k < 15 && (2ull << k) <= v) k++;
          if (v) {
            o[4 + k]++;
            o[20 + k] += v;
          }
          double g = 1e300;
          if (td[6] >= 0.0) {
            g = fmax(0.0, td[6] - 2.0 * p->eps_avail);
            for (int a = 0; a < 3; a++) {
              const double lo = fmin((double)rec[a], fmin((double)rec[a] + rec[3 + a], (double)rec[a] + rec[6 + a]));
              const double hi = fmax((double)rec[a], fmax((double)rec[a] + rec[3 + a], (double)rec[a] + rec[6 + a]));
              g = fmax(g, fmax(lo - td[a], td[3 + a] - hi) + fmax(0.0, td[6] - 2.0 * p->eps_avail));
            }
          }
          int kg = 0;
          while (kg < 15 && g >= p->eps_avail * std::ldexp(1.0, kg - 7)) kg++;
          o[36 + kg]++;
          o[52 + kg] += v;
        }
      }
    });
  for (auto& x : th) x.join();
  for (int k = 0; k < 88; k++) {
    out[k] = 0;
    for (int t = 0; t < threads; t++) out[k] += part[88 * (size_t)t + k];
  }
  unsigned long long nbad = 0;
  for (int t = 0; t < threads; t++) nbad += bad[t];
  return nbad ? -1 : 0;
}

// Host sample of the per-tile refinement (tests: tests/test_exact.py checks
// each dropped entry against the reference's float test on every camera
// sample of its tile): every stride-th (prim, tile) entry of a refined
// footprint (rtc::refined_footprint; no leaf boxes), 4 words each: prim, tx,
// ty, kept.  Returns the entries written (at most cap); *total = all sampled.
extern "C" size_t rt_cand_refine_sample_host(const CandParams* p, const float* tri, uint32_t stride,
                                             uint32_t* out, size_t cap, size_t* total) {
  const int threads = 8;
  std::vector<std::vector<uint32_t>> part(threads);
  std::vector<std::thread> th;
  if (stride < 1) stride = 1;
  for (int t = 0; t < threads; t++)
    th.emplace_back([&, t]() {
      for (uint32_t i = (uint32_t)t; i < p->nprim; i += (uint32_t)threads) {
        rtc::Footprint fp;
        const float* rec = tri + 12 * (size_t)i;
        if (rtc::classify(*p, rec, nullptr, fp) != rtc::FOOTPRINT || !rtc::refined_footprint(*p, fp)) continue;
        uint64_t k = 0;
        rtc::raster(*p, fp, [&](uint32_t tl) {
          if (((uint64_t)i * 7919u + k++) % stride != 0) return;
          int tx, ty;
          rt_tile_xy(tl, (uint32_t)p->rank, (uint32_t)p->nranks, (uint32_t)p->blocks_x, (uint32_t)p->tb, &tx, &ty);
          const uint32_t e[4] = {i, (uint32_t)tx, (uint32_t)ty, rtc::tile_keep(*p, rec, tx, ty) ? 1u : 0u};
          part[t].insert(part[t].end(), e, e + 4);
        });
      }
    });
  for (auto& x : th) x.join();
  size_t n = 0, all = 0;
  for (auto& v : part) {
    all += v.size() / 4;
    for (size_t j = 0; j + 4 <= v.size() && n < cap; j += 4, n++) std::memcpy(out + 4 * n, &v[j], 16);
  }
  *total = all;
  return n;
}

// Host check of the device-built lists of one frame (tests): every prim the
// float fast path listed is re-classified on the host (same code, so the
// same f64 bits; the safe ones have no tiles), every kept footprint compared
// bit for bit, and every tile's list equal, as a multiset, to the tiles the
// host raster gives the listed footprints.  out: [0] listed prims, [1] entries,
// [2] footprint mismatches, [3] tile-list mismatches (tiles), [4] globals,
// [5] fast-path filter violations, [6] prims the rank/frame filter dropped.
extern "C" int rt_cand_verify_host(const CandParams* p, const float* tri, const float* node,
                                   const uint32_t* prim_leaf, const uint32_t* list, uint32_t nlist,
                                   const void* fp_dev, const uint32_t* start, const uint32_t* cand,
                                   uint32_t ntiles, unsigned long long out[7]) {
  for (int k = 0; k < 7; k++) out[k] = 0;
  out[0] = nlist;
  out[1] = start[ntiles];
  const rtc::Footprint* fpd = (const rtc::Footprint*)fp_dev;
  // host threads: the process's share (OMP_NUM_THREADS on the GPU box), at
  // most 64 -- C5 re-classifies ~10^7 prims in f64
  int threads = (int)std::thread::hardware_concurrency();
  if (const char* e = std::getenv("OMP_NUM_THREADS"))
    if (std::atoi(e) > 0) threads = std::atoi(e);
  threads = threads < 1 ? 1 : (threads > 64 ? 64 : threads);
  std::vector<std::vector<uint64_t>> pairs(threads);  // (tile << 32 | prim) the host raster gives
  std::vector<unsigned long long> cnt(7 * (size_t)threads, 0);
  auto leafbox = [&](uint32_t prim) { return prim_leaf ? node + 8 * (size_t)prim_leaf[prim] : nullptr; };
  std::vector<unsigned char> listed(p->nprim + 1, 0);
  for (uint32_t j = 0; j < nlist; j++) listed[list[j]] = 1;
  std::vector<std::thread> th;
  for (int ti = 0; ti < threads; ti++)
    th.emplace_back([&, ti]() {
      unsigned long long* o = &cnt[7 * (size_t)ti];
      // every prim the fast path listed: re-classified, its footprint
      // compared with the device's bit for bit, its tiles collected
      for (uint32_t j = (uint32_t)ti; j < nlist; j += (uint32_t)threads) {
        const uint32_t prim = list[j];
        rtc::Footprint fp;
        std::memset(&fp, 0, sizeof fp);
        const int c = rtc::classify(*p, tri + 12 * (size_t)prim, leafbox(prim), fp);
        if (c == rtc::GLOBAL) {
          o[4]++;
          continue;
        }
        if (c != rtc::FOOTPRINT) continue;  // safe after all (leaf box): no tiles
        // a tall footprint's tiles (rtc::refined_footprint) refined per tile when p->refine
        const bool refine = p->refine && rtc::refined_footprint(*p, fp);
        const float* rec = tri + 12 * (size_t)prim;
        uint32_t n = 0;
        rtc::raster(*p, fp, [&](uint32_t t) {
          int tx, ty;
          rt_tile_xy(t, (uint32_t)p->rank, (uint32_t)p->nranks, (uint32_t)p->blocks_x, (uint32_t)p->tb, &tx, &ty);
          if (t < ntiles && (!refine || rtc::tile_keep(*p, rec, tx, ty))) pairs[ti].push_back((uint64_t)t << 32 | prim);
          n++;
        });
        if (n == 0) continue;  // the device keeps no footprint without tiles
        const rtc::Footprint& d = fpd[j];
        // (k, l, dimg are only set -- and only read -- with tri_ok)
        bool same = d.tri_ok == fp.tri_ok && d.b0 == fp.b0 && d.b1 == fp.b1 && d.b2 == fp.b2 &&
                    d.hw == fp.hw && d.hw0 == fp.hw0 && d.skip == fp.skip;
        if (same && fp.tri_ok) same = d.dimg == fp.dimg;
        for (int k = 0; k < 3 && same && fp.tri_ok; k++) same = d.k[k] == fp.k[k] && d.l[k] == fp.l[k];
        if (!same) o[2]++;
      }
      // prims the fast path did not list: proven safe, or their footprint has
      // no tile of this rank (the rank/frame filter must never drop a needed one)
      const uint32_t chunk = (p->nprim + (uint32_t)threads - 1) / (uint32_t)threads;
      const uint32_t b = (uint32_t)ti * chunk, e = b + chunk < p->nprim ? b + chunk : p->nprim;
      for (uint32_t prim = b; prim < e; prim++) {
        const int qc = rtc::quick_class(*p, tri + 12 * (size_t)prim);
        if (listed[prim]) {
          if (qc != rtc::Q_LIST) o[5]++;
          continue;
        }
        if (qc == rtc::Q_LIST) {  // the device should have listed it
          o[5]++;
          continue;
        }
        // Q_SAFE: the float fast path's proof checked against the f64 one --
        // a prim it calls safe must have no tile here by classify() either;
        // Q_AWAY: the rank/frame filter's drop, likewise
        rtc::Footprint fp;
        const int c = rtc::classify(*p, tri + 12 * (size_t)prim, leafbox(prim), fp);
        if (c == rtc::GLOBAL || (c == rtc::FOOTPRINT && rtc::raster_count(*p, fp) != 0)) o[5]++;
        if (qc != rtc::Q_SAFE) o[6]++;
      }
    });
  for (auto& x : th) x.join();
  for (int ti = 0; ti < threads; ti++)
    for (int k = 2; k < 7; k++) out[k] += cnt[7 * (size_t)ti + k];
  // every tile's list as a multiset: the host pairs sorted (tile, prim)
  // against each tile's sorted device entries
  size_t np = 0;
  for (auto& v : pairs) np += v.size();
  std::vector<uint64_t> want;
  want.reserve(np);
  for (auto& v : pairs) {
    want.insert(want.end(), v.begin(), v.end());
    std::vector<uint64_t>().swap(v);
  }
  std::sort(want.begin(), want.end());
  size_t w = 0;
  std::vector<uint32_t> got;
  for (uint32_t t = 0; t < ntiles; t++) {
    got.assign(cand + start[t], cand + start[t + 1]);
    std::sort(got.begin(), got.end());
    bool same = true;
    size_t k = 0;
    for (; w < want.size() && (uint32_t)(want[w] >> 32) == t; w++, k++)
      same = same && k < got.size() && got[k] == (uint32_t)want[w];
    if (!same || k != got.size()) out[3]++;
  }
  return 0;
}
