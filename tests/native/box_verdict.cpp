// box_verdict.cpp -- the packet walk's box verdicts of host/rt_cull.h
// (rt_box_wants, rt_box_within) against the formulas they replaced, on the CPU
// (tests/test_box_verdict.py builds it plain and with g++
// -fsanitize=address,undefined; no GPU, no HIP).
//
// Before, a miss was folded into an entry parameter of +inf and asked about
// again:
//   push:     t0 = hit ? tmin : +inf;  t0 != +inf && !(t0 * dlen > limit)
//   re-test:  t0 = hit ? tmin : +inf;  !(t0 * dlen > limit)
// Now the push is rt_box_wants(hit, tmin, dlen, limit) and the re-test, made
// only by lanes whose push verdict on the same floats was yes, is
// rt_box_within(tmin, dlen, limit).  Checked, bit for bit of the decision:
//   1. a full cross of special values at the verdict's own inputs (hit, tmin,
//      dlen, limit), reachable or not;
//   2. a cross of special values through rt_box_hit: box and origin components
//      of +-0, denormals, +-1, planes and origins at +-3e38, inv at rt_inv's
//      +-1e30 clamp and tiny, which produce tmin = +-inf and NaN;
//   3. two million random slabs (rays from rt_inv of random directions, some
//      components zero), with limits of 0, finite and +inf.
// In 2 and 3 every input whose push verdict is yes is also re-tested under
// every limit of the cross: the old re-test equals rt_box_within there.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "rt_cull.h"

static int failures = 0;
static long cases = 0;

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

static const float kInf = __builtin_inff();

// the formulas before the change, literally
static int old_push(int hit, float tmin, float dlen, float limit) {
  float t0 = hit ? tmin : kInf;
  return t0 != kInf && !(t0 * dlen > limit);
}
static int old_retest(int hit, float tmin, float dlen, float limit) {
  float t0 = hit ? tmin : kInf;
  return !(t0 * dlen > limit);
}

static void check(int hit, float tmin, float dlen, float limit, const std::vector<float>& relimits) {
  cases++;
  const int o = old_push(hit, tmin, dlen, limit), n = rt_box_wants(hit, tmin, dlen, limit);
  if ((o != 0) != (n != 0)) {
    if (failures++ < 20)
      std::printf("FAIL push: hit %d tmin %08x dlen %08x limit %08x: old %d new %d\n", hit, bits(tmin), bits(dlen),
                  bits(limit), o, n);
    return;
  }
  if (!n) return;
  if (!hit) {  // a wanted box was hit: what the re-test relies on
    if (failures++ < 20) std::printf("FAIL wanted without a hit: tmin %08x\n", bits(tmin));
    return;
  }
  for (float l2 : relimits) {
    cases++;
    const int ro = old_retest(hit, tmin, dlen, l2), rn = rt_box_within(tmin, dlen, l2);
    if ((ro != 0) != (rn != 0) && failures++ < 20)
      std::printf("FAIL re-test: tmin %08x dlen %08x limit %08x: old %d new %d\n", bits(tmin), bits(dlen), bits(l2),
                  ro, rn);
  }
}

// xorshift64*: the same sequence everywhere
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
static float urand(float lo, float hi) { return lo + (hi - lo) * (float)((rnd() >> 40) * (1.0 / 16777216.0)); }

int main() {
  const float nan = __builtin_nanf("");
  const float den = 1e-42f;
  const std::vector<float> limits = {0.0f, 1e-3f, 1.0f, 7.5f, 1e30f, 3.4e38f, kInf};
  const std::vector<float> dlens = {1e-42f, 1e-30f, 1e-3f, 1.0f, 3.5f, 1e30f, 3.4e38f};

  // 1. the verdict's own inputs (limits and dlens here also 0, negative, NaN)
  {
    const std::vector<float> t = {nan, -kInf, -3.4e38f, -1.0f, -den, -0.0f, 0.0f, den, 1e-30f, 0.5f, 1.0f, 2.0f,
                                  1e30f, 3.4e38f, kInf};
    std::vector<float> dl = dlens, lim = limits;
    for (float x : {0.0f, -0.0f, -1.0f, kInf, nan}) dl.push_back(x);
    for (float x : {-0.0f, -1.0f, -kInf, nan}) lim.push_back(x);
    for (int hit = 0; hit < 2; hit++)
      for (float tm : t)
        for (float d : dl)
          for (float l : lim) {
            cases++;
            const int o = old_push(hit, tm, d, l), n = rt_box_wants(hit, tm, d, l);
            if ((o != 0) != (n != 0) && failures++ < 20)
              std::printf("FAIL cross: hit %d tmin %08x dlen %08x limit %08x: old %d new %d\n", hit, bits(tm), bits(d),
                          bits(l), o, n);
            if (hit) {  // the re-test's claim needs only the hit
              const int ro = old_retest(hit, tm, d, l), rn = rt_box_within(tm, d, l);
              if ((ro != 0) != (rn != 0) && failures++ < 20)
                std::printf("FAIL cross re-test: tmin %08x dlen %08x limit %08x\n", bits(tm), bits(d), bits(l));
            }
          }
  }

  // 2. special values through the slab test: per axis the distinct (t0, t1)
  // pairs of the planes, then every triple of them through rt_box_hit's own
  // min / max network (one axis at a time: the other two axes' planes are
  // fed as origin 0, inv 1, so that lo = t0 and hi = t1 reproduce the pair)
  {
    const std::vector<float> plane = {-3e38f, -1.0f, -den, -0.0f, 0.0f, den, 1.0f, 3e38f};
    const std::vector<float> org = {-3e38f, -1.0f, -den, -0.0f, 0.0f, den, 1.0f, 3e38f};
    const std::vector<float> eps = {0.0f, 1e-6f};
    const std::vector<float> dir = {0.0f, -0.0f, den, -den, 1e-30f, -1e-30f, 1.0f, -1.0f, 3e38f, -3e38f};
    std::set<uint64_t> pairs;
    for (float l : plane)
      for (float h : plane)
        for (float o : org)
          for (float e : eps)
            for (float d : dir) {
              const float inv = rt_inv(d), oh = o + e, ol = o - e;
              const float t0 = fmaf(l, inv, -(oh * inv)), t1 = fmaf(h, inv, -(ol * inv));
              pairs.insert((uint64_t)bits(t0) << 32 | bits(t1));
            }
    // the verdict sees a pair only through min and max: keep one pair per (min, max)
    std::set<uint64_t> mm;
    std::vector<std::pair<float, float>> pv;
    for (uint64_t k : pairs) {
      float a, b;
      const uint32_t ua = (uint32_t)(k >> 32), ub = (uint32_t)k;
      std::memcpy(&a, &ua, 4);
      std::memcpy(&b, &ub, 4);
      const float lo = fminf(a, b), hi = fmaxf(a, b);
      if (mm.insert((uint64_t)bits(lo) << 32 | bits(hi)).second) pv.push_back({a, b});
    }
    std::printf("slab pairs %zu, distinct (min, max) %zu\n", pairs.size(), pv.size());
    std::set<uint64_t> seen;  // distinct (hit, tmin) out of the triples
    // (unordered triples: the network treats the three axes alike)
    for (size_t i = 0; i < pv.size(); i++)
      for (size_t j = i; j < pv.size(); j++)
        for (size_t k = j; k < pv.size(); k++) {
          const std::pair<float, float>&x = pv[i], &y = pv[j], &z = pv[k];
          float tmin;
          // origin 0, eps 0, inv 1: fma(lo, 1, -(0 * 1)) = lo exactly (x + -0 = x)
          const int hit = rt_box_hit(0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, x.first, y.first, z.first,
                                     x.second, y.second, z.second, &tmin);
          if (!seen.insert((uint64_t)(hit != 0) << 32 | bits(tmin)).second) continue;
          for (float d : dlens)
            for (float l : limits) check(hit, tmin, d, l, limits);
        }
    std::printf("distinct (hit, tmin) %zu\n", seen.size());
  }

  // 3. random slabs
  {
    for (int i = 0; i < 2000000; i++) {
      float d[3], o[3], lo[3], hi[3];
      const uint64_t r = rnd();
      for (int a = 0; a < 3; a++) {
        d[a] = urand(-1.0f, 1.0f);
        if (((r >> (4 * a)) & 15) == 0) d[a] = (r >> (4 * a + 3) & 16) ? -0.0f : 0.0f;  // axis-parallel rays
        o[a] = urand(-20.0f, 20.0f);
        const float c = urand(-20.0f, 20.0f), w = urand(0.0f, 8.0f);
        lo[a] = c - w;
        hi[a] = c + w;
        if (((r >> (12 + 4 * a)) & 15) == 0) o[a] = lo[a];  // an origin on a plane
      }
      const float e = urand(1e-6f, 1e-3f);
      const float dlen = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      float tmin;
      const int hit = rt_box_hit(o[0] + e, o[1] + e, o[2] + e, o[0] - e, o[1] - e, o[2] - e, rt_inv(d[0]), rt_inv(d[1]),
                                 rt_inv(d[2]), lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], &tmin);
      const int k = (int)((r >> 40) % 4);
      const float best = k == 0 ? kInf : k == 1 ? 0.0f : urand(0.0f, 60.0f);
      const float limit = k == 0 ? kInf : rt_prune_limit(best, e);
      const std::vector<float> re = {limit, rt_prune_limit(urand(0.0f, 60.0f), e), 0.0f};
      check(hit, tmin, dlen, limit, re);
    }
  }

  if (failures) {
    std::printf("box verdict: %d failures\n", failures);
    return 1;
  }
  std::printf("box verdict ok (%ld cases)\n", cases);
  return 0;
}
