// rt_path_items.h -- the arithmetic of the path export (rt_hip_path_records,
// csrc/rt_paths.hip, csrc/rt_paths.cpp) that needs no device: the blocks of
// rays the length and write passes run over, the scratch words that hold their
// totals, the chunks in which one workgroup scans those, and where a hit
// record index points.  Plain C++ (host and device): the kernels, the host
// layer and tests/native/path_items.cpp include it.
#pragma once

#include "rt_ray_items.h"

// rt_gsample::prim of an exported vertex (include/rt_hip.h RT_PATH_PRIM): a
// hit whose triangle the hit records do not keep; consumers read its sign
#define RT_PATH_PRIM_D 0x7fffffffu
// rays of one block of the length and write passes: one lane per ray
#define RT_PATH_BLOCK 256u
// block totals one step of the one-workgroup scan covers: one per thread
#define RT_PATH_CHUNK 1024u
// a record index is region | (slot << RT_PATH_REGION_BITS) (rt_kernels.h)
#define RT_PATH_REGION_BITS 3
static_assert((1u << RT_PATH_REGION_BITS) == RT_REC_REGIONS, "a record index's region field holds every region");

// blocks of n rays (n <= RT_RAY_BATCH_MAX): block b holds rays [256 b, 256 b + 256)
RT_TILES_FN uint32_t rt_path_blocks(unsigned long long n) {
  return (uint32_t)((n + RT_PATH_BLOCK - 1) / RT_PATH_BLOCK);
}
// scratch words of n rays: one per block, its total, then scanned in place
RT_TILES_FN size_t rt_path_scratch_words(unsigned long long n) { return (size_t)rt_path_blocks(n); }
// steps of the one-workgroup scan over `blocks` totals
RT_TILES_FN uint32_t rt_path_chunks(uint32_t blocks) { return (blocks + RT_PATH_CHUNK - 1) / RT_PATH_CHUNK; }
// the rays one step of that scan accounts for
RT_TILES_FN unsigned long long rt_path_chunk_rays(void) { return (unsigned long long)RT_PATH_CHUNK * RT_PATH_BLOCK; }

// region and slot of a record index, and the record's place in buffers of
// hit_cap records per region (rt_render.hip rec_addr: region * hit_cap + slot)
RT_TILES_FN uint32_t rt_path_region(uint32_t idx) { return idx & (RT_REC_REGIONS - 1u); }
RT_TILES_FN uint32_t rt_path_slot(uint32_t idx) { return idx >> RT_PATH_REGION_BITS; }
RT_TILES_FN size_t rt_path_rec_addr(uint32_t idx, uint32_t hit_cap) {
  return (size_t)rt_path_region(idx) * hit_cap + rt_path_slot(idx);
}
