// path_items.cpp -- the arithmetic of the path export (csrc/rt_path_items.h)
// on the CPU (tests/test_paths_host.py builds it plain and with g++
// -fsanitize=address,undefined; no GPU, no HIP).  For ragged n, one chunk of
// the block-total scan +- 1 and the largest batch: the blocks cover every ray
// once, the scratch holds a word per block, the chunks cover every block once,
// a scan done in the kernels' three steps (block totals, chunked scan with a
// carry, block-local scan on the base) is the plain exclusive scan, and a
// record index addresses region * hit_cap + slot inside the buffers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt_path_items.h"

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

static void check_counts(unsigned long long n) {
  const uint32_t blocks = rt_path_blocks(n), chunks = rt_path_chunks(blocks);
  CHECK((unsigned long long)blocks * RT_PATH_BLOCK >= n, "blocks of %llu rays cover them", n);
  CHECK(n == 0 ? blocks == 0 : (unsigned long long)(blocks - 1) * RT_PATH_BLOCK < n, "no idle block: n %llu", n);
  CHECK(rt_path_scratch_words(n) == blocks, "a scratch word per block: n %llu", n);
  CHECK((unsigned long long)chunks * RT_PATH_CHUNK >= blocks, "chunks of %u blocks cover them", blocks);
  CHECK(blocks == 0 ? chunks == 0 : (unsigned long long)(chunks - 1) * RT_PATH_CHUNK < blocks, "no idle chunk: n %llu", n);
  // the last thread of the last chunk forms this block index: it must not wrap
  CHECK((unsigned long long)chunks * RT_PATH_CHUNK <= 0xffffffffull, "block indices of n %llu fit 32 bits", n);
}

// the three steps of csrc/rt_paths.hip on the host, against the plain scan
static void check_scan(unsigned long long n) {
  std::vector<uint32_t> len(n), off(n + 1), want(n + 1);
  uint32_t x = 12345u;
  for (unsigned long long i = 0; i < n; i++) {
    x = x * 1664525u + 1013904223u;
    len[i] = (x >> 24) % 5u == 0 ? (x >> 16) % 45u : (x >> 20) % 3u;
  }
  uint32_t run = 0;
  for (unsigned long long i = 0; i < n; i++) want[i] = run, run += len[i];
  want[n] = run;
  const uint32_t blocks = rt_path_blocks(n);
  std::vector<uint32_t> btot(rt_path_scratch_words(n), 0xdeadbeefu);
  for (uint32_t b = 0; b < blocks; b++) {  // 1: lengths
    uint32_t t = 0;
    for (uint32_t k = 0; k < RT_PATH_BLOCK; k++) {
      const unsigned long long i = (unsigned long long)b * RT_PATH_BLOCK + k;
      if (i < n) off[i] = len[i], t += len[i];
    }
    btot[b] = t;
  }
  uint32_t carry = 0;  // 2: block totals, chunk by chunk
  for (uint32_t c = 0; c < rt_path_chunks(blocks); c++) {
    uint32_t before = 0;
    for (uint32_t k = 0; k < RT_PATH_CHUNK; k++) {
      const uint32_t b = c * RT_PATH_CHUNK + k;
      if (b >= blocks) continue;
      const uint32_t v = btot[b];
      btot[b] = carry + before;
      before += v;
    }
    carry += before;
  }
  off[n] = carry;
  for (uint32_t b = 0; b < blocks; b++) {  // 3: the block-local scan on its base
    uint32_t before = 0;
    for (uint32_t k = 0; k < RT_PATH_BLOCK; k++) {
      const unsigned long long i = (unsigned long long)b * RT_PATH_BLOCK + k;
      if (i >= n) break;
      const uint32_t l = off[i];
      off[i] = btot[b] + before;
      before += l;
    }
  }
  unsigned long long bad = 0;
  for (unsigned long long i = 0; i <= n; i++) bad += off[i] != want[i];
  CHECK(bad == 0, "the three steps give the exclusive scan: n %llu, %llu words differ", n, bad);
}

static void check_addr(uint32_t hit_cap) {
  // every (region, slot) once, inside RT_REC_REGIONS * hit_cap records
  std::vector<unsigned char> seen((size_t)RT_REC_REGIONS * hit_cap, 0);
  for (uint32_t region = 0; region < RT_REC_REGIONS; region++)
    for (uint32_t slot = 0; slot < hit_cap; slot++) {
      const uint32_t idx = region | (slot << RT_PATH_REGION_BITS);
      CHECK(rt_path_region(idx) == region && rt_path_slot(idx) == slot, "fields of index %u", idx);
      const size_t at = rt_path_rec_addr(idx, hit_cap);
      CHECK(at == (size_t)region * hit_cap + slot && at < seen.size(), "address of index %u", idx);
      if (at >= seen.size()) return;
      CHECK(!seen[at], "address %zu twice", at);
      seen[at] = 1;
    }
}

int main() {
  const unsigned long long one = rt_path_chunk_rays();
  CHECK(one == 262144ull, "a chunk's rays: %llu", one);
  for (unsigned long long n : {0ull, 1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, one - 1, one, one + 1}) {
    check_counts(n);
    check_scan(n);
  }
  // the largest batch: nothing wraps
  const unsigned long long big = RT_RAY_BATCH_MAX;
  check_counts(big);
  CHECK(rt_path_blocks(big) == 0x1000000u, "blocks of the largest batch: %u", rt_path_blocks(big));
  CHECK(rt_path_chunks(rt_path_blocks(big)) == 0x4000u, "its chunks: %u", rt_path_chunks(rt_path_blocks(big)));
  CHECK(rt_path_scratch_words(big) * sizeof(uint32_t) == (size_t)1 << 26, "its scratch bytes");
  CHECK((unsigned long long)(rt_path_blocks(big) - 1) * RT_PATH_BLOCK + (RT_PATH_BLOCK - 1) >= big - 1,
        "its last ray has a lane");
  // the record index: the last slot of the last region, and NO_REC's slot is past every buffer
  for (uint32_t cap : {1u, 2u, 1000u}) check_addr(cap);
  const uint32_t last = (RT_REC_REGIONS - 1u) | ((uint32_t)RT_REC_SLOT_MAX - 1u) << RT_PATH_REGION_BITS;
  CHECK(rt_path_rec_addr(last, (uint32_t)RT_REC_SLOT_MAX) == (size_t)RT_REC_REGIONS * RT_REC_SLOT_MAX - 1,
        "the last record of the largest buffers");
  CHECK(rt_path_slot(0xffffffffu) == RT_REC_SLOT_MAX, "no record's slot lies past every buffer");
  CHECK(RT_PATH_PRIM_D == 0x7fffffffu && (int32_t)RT_PATH_PRIM_D > 0, "the exported prim reads as a hit");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("path items ok\n");
  return 0;
}
