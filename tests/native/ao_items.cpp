// ao_items.cpp -- the ray rule of ambient occlusion from G-buffer records
// (csrc/rt_ao_items.h) on the CPU (tests/test_ao_host.py builds it plain and
// with g++ -fsanitize=address,undefined; no GPU, no HIP).
//
//   ao_items                 the header's own checks: the hash, the frame's
//                            orthonormality, the lane -> sample map, the items
//   ao_items IN OUT          evaluate the rule on a file of records and write
//                            the rays, for the numpy twin to be compared with
//
// IN:  u64 n, u64 base, u32 k, u32 m, u32 seed, u32 0, then n records of 10
//      words (rt_gsample), then m rows of 3 floats.
// OUT: n k origins (3 floats each), n k directions, n shot bytes; a record that
//      does not shoot writes zeros, as ao_rays_kernel does.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_ao_items.h"

static int failures = 0;
#define CHECK(cond, ...)                                         \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
      failures++;                                                \
    }                                                            \
  } while (0)

struct Sample {
  int32_t prim, obj, queries;
  float dist, P[3], N[3];
};
static_assert(sizeof(Sample) == 40, "rt_gsample is 10 words");

static void rays_of(const Sample& s, unsigned long long g, uint32_t k, const float* table, uint32_t m, uint32_t seed,
                    float* o, float* d, unsigned char* shot) {
  const float l = rt_ao_length(s.N);
  *shot = rt_ao_shoots(s.prim, l) ? 1 : 0;
  if (!*shot) {
    std::memset(o, 0, 3 * k * sizeof(float));
    std::memset(d, 0, 3 * k * sizeof(float));
    return;
  }
  rt_ao_frame f;
  rt_ao_frame_of(s.N, l, &f);
  const uint32_t h = rt_ao_hash(g, seed);
  for (uint32_t r = 0; r < k; r++) {
    rt_ao_dir(&f, table + 3 * (size_t)rt_ao_row(h, m, r), h, d + 3 * r);
    std::memcpy(o + 3 * r, s.P, 3 * sizeof(float));
  }
}

static int run_file(const char* in, const char* out) {
  std::FILE* fi = std::fopen(in, "rb");
  if (!fi) return 2;
  uint64_t head[2];
  uint32_t par[4];
  if (std::fread(head, 8, 2, fi) != 2 || std::fread(par, 4, 4, fi) != 4) return 2;
  const uint64_t n = head[0], base = head[1];
  const uint32_t k = par[0], m = par[1], seed = par[2];
  if (k == 0 || k > RT_AO_KMAX_D || m == 0 || n > (1u << 24)) return 2;
  std::vector<Sample> smp(n);
  std::vector<float> table(3 * (size_t)m);
  if (n && std::fread(smp.data(), sizeof(Sample), n, fi) != n) return 2;
  if (std::fread(table.data(), 12, m, fi) != m) return 2;
  std::fclose(fi);
  std::vector<float> o(3 * n * k), d(3 * n * k);
  std::vector<unsigned char> shot(n);
  for (uint64_t i = 0; i < n; i++)
    rays_of(smp[i], base + i, k, table.data(), m, seed, o.data() + 3 * i * k, d.data() + 3 * i * k, &shot[i]);
  std::FILE* fo = std::fopen(out, "wb");
  if (!fo) return 2;
  std::fwrite(o.data(), 4, o.size(), fo);
  std::fwrite(d.data(), 4, d.size(), fo);
  std::fwrite(shot.data(), 1, shot.size(), fo);
  std::fclose(fo);
  std::printf("ao items ok\n");
  return 0;
}

static void self_checks() {
  // the hash: the stated mixer, 64-bit g
  CHECK(rt_ao_mix32(0u) == 0u, "mix32(0)");
  CHECK(rt_ao_mix32(1u) == 0x688990c0u, "mix32(1) = %08x", rt_ao_mix32(1u));
  CHECK(rt_ao_hash(5ull, 9u) != rt_ao_hash((1ull << 32) + 5ull, 9u), "the high word takes part");
  CHECK(rt_ao_hash(5ull, 9u) != rt_ao_hash(5ull, 10u), "the seed takes part");
  // who shoots
  const float inf = __builtin_inff(), qnan = __builtin_nanf("");
  const float rows[][3] = {{0, 0, 1}, {0, 0, 0}, {-0.0f, 0, -0.0f}, {qnan, 0, 1}, {inf, 0, 0}, {1e-30f, 0, 0},
                           {1e30f, 0, 0}, {0, 0, -1}, {3, -4, 12}};
  const int want[] = {1, 0, 0, 0, 0, 0, 0, 1, 1};
  for (int i = 0; i < 9; i++) {
    CHECK(rt_ao_shoots(0, rt_ao_length(rows[i])) == want[i], "row %d", i);
    CHECK(!rt_ao_shoots(-1, rt_ao_length(rows[i])), "a miss does not shoot (row %d)", i);
  }
  // the frame is orthonormal to float rounding, at the poles too
  const float ns[][3] = {{0, 0, 1}, {0, 0, -1}, {1, 0, 0}, {0, 1, -0.0f}, {0.6f, 0, -0.8f}, {1, 1, 1}, {-2, 3, -1e-20f}};
  for (const auto& N : ns) {
    rt_ao_frame f;
    rt_ao_frame_of(N, rt_ao_length(N), &f);
    double tt = 0, bb = 0, tb = 0, tn = 0, bn = 0;
    for (int c = 0; c < 3; c++) {
      tt += (double)f.T[c] * f.T[c], bb += (double)f.B[c] * f.B[c], tb += (double)f.T[c] * f.B[c];
      tn += (double)f.T[c] * f.n[c], bn += (double)f.B[c] * f.n[c];
    }
    CHECK(std::fabs(tt - 1) < 1e-6 && std::fabs(bb - 1) < 1e-6 && std::fabs(tb) < 1e-6 && std::fabs(tn) < 1e-6 &&
              std::fabs(bn) < 1e-6, "frame of (%g %g %g): %g %g %g %g %g", N[0], N[1], N[2], tt, bb, tb, tn, bn);
  }
  // the lane -> sample map is lane / k, and the items cover n samples exactly
  for (uint32_t k = 1; k <= 64; k++) {
    const uint32_t kinv = rt_ao_kinv(k), spi = rt_ao_spi(k);
    CHECK(spi >= 1 && spi * k <= 64 && (spi + 1) * k > 64, "spi of k = %u", k);
    for (uint32_t lane = 0; lane < 64; lane++) CHECK(rt_ao_lane_sample(lane, kinv) == lane / k, "lane %u k %u", lane, k);
  }
  for (uint32_t k : {1u, 3u, 5u, 64u, 65u, 100u, 1024u}) {
    CHECK(rt_ao_rounds(k) == (k + 63) / 64 && (k <= 64 || rt_ao_spi(k) == 1), "k = %u", k);
    for (unsigned long long n : {0ull, 1ull, 20ull, 21ull, 22ull, 2304ull, (unsigned long long)RT_RAY_BATCH_MAX / k}) {
      const unsigned long long items = rt_ao_item_count(n, k), spi = rt_ao_spi(k);
      CHECK(items * spi >= n && (items == 0 || (items - 1) * spi < n), "n %llu k %u", n, k);
      CHECK(items <= 0xffffffffull / 8, "8 q + x fits 32 bits: n %llu k %u", n, k);
    }
  }
  // rows wrap the table
  CHECK(rt_ao_row(8u * 36u, 37u, 0) == 36u && rt_ao_row(8u * 36u, 37u, 1) == 0u && rt_ao_row(8u * 36u, 37u, 38) == 0u, "wrap");
}

int main(int argc, char** argv) {
  if (argc == 3) return run_file(argv[1], argv[2]);
  self_checks();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ao items ok\n");
  return 0;
}
