// rt_tiles.h -- how the frame's 8x8-pixel tiles are dealt to ranks, shared
// by the device kernels (render, candidate lists, assemble) and their host
// mirrors (rt_hip.cpp, the host re-derivation of the candidate lists in
// rt_cand_host.cpp, rtgpu.py's tile_xy / tile_local).
//
// Tiles are grouped into blocks of tb x tb tiles, tb = rt_block_side(nranks):
// 4 (32 x 32 pixels) when the frame is split, 1 (plain scanline tile order)
// for one rank.  Block (bx, by) (blocks_x = ceil(tiles_x / tb) per row)
// belongs to rank (bx + by) mod n: diagonals.  A rank's tile buffer holds its
// blocks in scanline order, each as tb^2 tiles in row-major order (tiles past
// the frame's edge are padding: their pixels are invalid and written as 0).
//
// Why whole blocks: a camera-ray candidate footprint (csrc/rt_cand_geom.h) of a
// few tiles touches one or two ranks instead of one rank per 8-pixel column
// (round 2's interleave t mod n made every rank classify every footprint
// wider than 8 n pixels).  Why diagonals: rounds 3-4 dealt block b (scanline)
// to rank b mod n, and at 4K blocks_x = 120 is a multiple of 2, 4 and 8, so
// every rank owned the same block columns in every block row -- pure 32-pixel
// column stripes, and a scene whose cost varies by column (C5's grid of
// spheres) loaded one rank 25 % above the mean at N = 8 (VERDICT r04 weak
// #5).  On diagonals every rank holds 1/n of every block row (up to one
// block) and of every block column (up to one block per n rows) whatever
// blocks_x is, so a cost that varies by row or by column alone spreads
// evenly.  Every n consecutive block rows give each rank exactly blocks_x
// blocks, which keeps the rank-local index arithmetic O(1).
//
// cpu/rt splits the frame into 4 quadrants for its 4 pthreads
// (cpu/raytracer.c:92-127); this is the same idea sized for 8 GPUs x 256 CUs.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_TILES_FN __host__ __device__ inline
#else
#define RT_TILES_FN static inline
#endif

#define RT_TB 4  // block side of a split frame, in tiles

RT_TILES_FN int rt_block_side(int nranks) { return nranks > 1 ? RT_TB : 1; }
RT_TILES_FN int rt_blocks_x(int tiles_x, int tb) { return (tiles_x + tb - 1) / tb; }
RT_TILES_FN int rt_blocks_y(int tiles_y, int tb) { return (tiles_y + tb - 1) / tb; }

// the first block column of rank r in block row by (then every n-th)
RT_TILES_FN uint32_t rt_row_res(uint32_t by, uint32_t n, uint32_t r) { return (r + n - by % n) % n; }

// #{t in [0, x) : t mod n < rm}
RT_TILES_FN uint32_t rt_count_low(uint32_t x, uint32_t n, uint32_t rm) {
  const uint32_t k = x % n;
  return (x / n) * rm + (k < rm ? k : rm);
}

// Blocks of rank r in block rows [0, by): row y holds q + [res(y) < rm] of
// them (blocks_x = q n + rm), and n consecutive rows hold blocks_x in all.
RT_TILES_FN uint32_t rt_rank_rows_blocks(uint32_t by, uint32_t blocks_x, uint32_t n, uint32_t r) {
  if (n == 1) return by * blocks_x;
  const uint32_t q = blocks_x / n, rm = blocks_x % n, L = by % n;
  // the last L rows of [0, by) have res = r - y' (mod n) for y' = 0 .. L-1:
  // the integers r - L + 1 .. r, shifted by n to stay >= 0
  const uint32_t part = rt_count_low(r + n + 1, n, rm) - rt_count_low(r + n + 1 - L, n, rm);
  return (by / n) * blocks_x + (by % n) * q + part;
}

// blocks of rank r in a frame of blocks_x x blocks_y blocks
RT_TILES_FN uint32_t rt_rank_blocks(uint32_t blocks_x, uint32_t blocks_y, uint32_t n, uint32_t r) {
  return rt_rank_rows_blocks(blocks_y, blocks_x, n, r);
}

// tiles per row and per column of a W x H frame (a ragged edge is a whole tile)
RT_TILES_FN int tiles_x_of(int W) { return (W + 7) / 8; }
RT_TILES_FN int tiles_y_of(int H) { return (H + 7) / 8; }

// tiles rank `rank` renders (whole blocks, edge padding included)
RT_TILES_FN int rank_tile_count(int W, int H, int rank, int nranks) {
  const int tb = rt_block_side(nranks);
  return (int)(rt_rank_blocks((uint32_t)rt_blocks_x(tiles_x_of(W), tb), (uint32_t)rt_blocks_y(tiles_y_of(H), tb),
                              (uint32_t)nranks, (uint32_t)rank) * tb * tb);
}

// the most blocks any rank holds (the tile buffers' stride; host side, O(n))
RT_TILES_FN uint32_t rt_max_rank_blocks(uint32_t blocks_x, uint32_t blocks_y, uint32_t n) {
  uint32_t m = 0;
  for (uint32_t r = 0; r < n; r++) {
    const uint32_t c = rt_rank_blocks(blocks_x, blocks_y, n, r);
    m = c > m ? c : m;
  }
  return m;
}

// (tx, ty) of rank-local tile t of rank r: block j = t / tb^2 of the rank,
// its row found by bisection over the rank's per-row prefix counts
RT_TILES_FN void rt_tile_xy(uint32_t t, uint32_t r, uint32_t n, uint32_t blocks_x, uint32_t tb,
                            int* tx, int* ty) {
  const uint32_t j = t / (tb * tb), k = t % (tb * tb);
  if (n == 1) {  // one rank: scanline order
    *tx = (int)((j % blocks_x) * tb + k % tb);
    *ty = (int)((j / blocks_x) * tb + k / tb);
    return;
  }
  // j lies in the period of n rows m = j / blocks_x (blocks_x blocks each)
  uint32_t lo = (j / blocks_x) * n, hi = lo + n;  // rows(lo) <= j < rows(hi)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (rt_rank_rows_blocks(mid, blocks_x, n, r) <= j) lo = mid; else hi = mid;
  }
  const uint32_t by = lo, bx = rt_row_res(by, n, r) + (j - rt_rank_rows_blocks(by, blocks_x, n, r)) * n;
  *tx = (int)(bx * tb + k % tb);
  *ty = (int)(by * tb + k / tb);
}

// ---- trace work items: which rays of a tile one wave takes
// A tile's 256 camera rays (64 pixels x the 4 supersamples of
// cpu/raytracer.c:55-58, sample smp = 2 * (k step) + (l step)) are traced as 4
// work items of 64 lanes, item 4t + q of rank-local tile t.  Item q is the
// tile's 4x4-pixel quarter q = 2 * (row >= 4) + (col >= 4) with all four
// samples of its 16 pixels: lane = 4 * (4 * (row & 3) + (col & 3)) + smp.
// The rays of a wave then span a quarter of the tile's cone, so the packet
// walk's union of nodes and leaves is close to what each ray needs (DESIGN.md
// §4), and a pixel's four slots of the per-(item, lane) arrays
// (KParams::last, KParams::capture) are contiguous in sample order:
// rt_pixel_slots.  This header is the only place that spells the layout out.
#define RT_TILE_ITEMS 4  // work items per tile

// lane `lane` of a tile's item q: its pixel (row, col) in the 8x8 tile, its sample
RT_TILES_FN void rt_item_pixel(uint32_t q, uint32_t lane, int* row, int* col, int* smp) {
  const uint32_t px = lane >> 2;  // pixel of the quarter, row-major
  *row = (int)(((q >> 1) << 2) | (px >> 2));
  *col = (int)(((q & 1u) << 2) | (px & 3u));
  *smp = (int)(lane & 3u);
}

// index of tile t's pixel (row, col), sample 0, in the per-(item, lane)
// arrays; samples 1..3 follow it (the index is a multiple of 4)
RT_TILES_FN size_t rt_pixel_slots(uint32_t t, int row, int col) {
  const uint32_t q = 2u * (uint32_t)(row >= 4) + (uint32_t)(col >= 4);
  const uint32_t lane = 4u * (4u * ((uint32_t)row & 3u) + ((uint32_t)col & 3u));
  return ((size_t)t * RT_TILE_ITEMS + q) * 64 + lane;
}

// the inverse of rt_item_pixel: index of (tile t, pixel (row, col), sample smp)
RT_TILES_FN size_t rt_item_slot(uint32_t t, int row, int col, int smp) {
  return rt_pixel_slots(t, row, col) + (size_t)smp;
}

// rank and rank-local index of tile (tx, ty)
RT_TILES_FN uint32_t rt_tile_local(int tx, int ty, uint32_t n, uint32_t blocks_x, uint32_t tb,
                                   uint32_t* rank) {
  const uint32_t bx = (uint32_t)tx / tb, by = (uint32_t)ty / tb;
  const uint32_t r = (bx + by) % n;
  *rank = r;
  return (rt_rank_rows_blocks(by, blocks_x, n, r) + bx / n) * tb * tb + ((uint32_t)ty % tb) * tb +
         (uint32_t)tx % tb;
}

// rank-local index of block column bx of block row by, for the rank owning it
RT_TILES_FN uint32_t rt_block_local(uint32_t bx, uint32_t by, uint32_t n, uint32_t blocks_x, uint32_t r) {
  return rt_rank_rows_blocks(by, blocks_x, n, r) + bx / n;
}

// Rank r's tiles in tile row ty, columns [x0, x1] (x0 <= x1): the blocks of
// the row whose column is res(by) mod n, each contributing its columns
// inside the interval.  first_bx (out, optional) = the first such block
// column; the next ones follow every n columns.  O(1).
RT_TILES_FN uint32_t rt_rank_row_tiles(int ty, int x0, int x1, uint32_t n, uint32_t r,
                                       uint32_t blocks_x, uint32_t tb, int* first_bx) {
  (void)blocks_x;
  const uint32_t by = (uint32_t)ty / tb;
  const uint32_t bx0 = (uint32_t)x0 / tb, bx1 = (uint32_t)x1 / tb;
  // block columns bx with (bx + by) mod n == r: bx = res + m n
  const uint32_t res = rt_row_res(by, n, r);
  const uint32_t f = bx0 <= res ? res : bx0 + (res + n - bx0 % n) % n;  // first match >= bx0
  if (first_bx) *first_bx = (int)f;
  if (f > bx1) return 0;
  const uint32_t m = (bx1 - f) / n + 1;  // matching blocks
  uint32_t c = m * tb;
  if (f == bx0) c -= (uint32_t)x0 - bx0 * tb;                 // cut on the left
  const uint32_t last = f + (m - 1) * n;
  if (last == bx1) c -= bx1 * tb + tb - 1 - (uint32_t)x1;     // cut on the right
  return c;
}
