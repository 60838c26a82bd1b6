// Per-wave cache of coarse hash-grid cells in LDS: the keys (nerf_device.h encode_issue_cached / cell_cache_fill use them; plain C++,
// so that tests/aux/cell_tag_check.cpp can check them on the host).
//
// A line holds one CELL of one of the levels 0 .. CELL_CACHE_LEVELS - 1: its 8 corner entries in tcnn corner order (64 B). The tag is the
// cell's low corner packed 8 bits per coordinate; a lane whose cell has a coordinate above CELL_COORD_MAX (a level finer than 256 cells
// across, a position outside the unit cube on a hashed level) is not cacheable and gathers as it always did, so two cells that the cache
// can hold never share a tag whatever N_min and per_level_scale the model has.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGP_CELL_FN __host__ __device__ __forceinline__
#else
#define NGP_CELL_FN inline
#endif

namespace ngp {

constexpr int CELL_CACHE_LEVELS = 4;            // lane group h looks up level h; its second level, h + 4, is never cached
constexpr uint32_t CELL_COORD_MAX = 255u;       // 8 bits per coordinate
constexpr uint32_t CELL_TAG_NONE = 0xFFFFFFFFu; // no cell (bits 24..31 of a real tag are zero)

NGP_CELL_FN bool cell_cacheable(uint32_t gx, uint32_t gy, uint32_t gz) { return ((gx | gy | gz) >> 8) == 0u; }
NGP_CELL_FN uint32_t cell_tag(uint32_t gx, uint32_t gy, uint32_t gz) { return gx | (gy << 8) | (gz << 16); }
// direct-mapped: the low bit of every coordinate (a 2 x 2 x 2 neighbourhood of cells never collides), then the second bits folded together
NGP_CELL_FN uint32_t cell_set(uint32_t tag, uint32_t n_sets) {
	const uint32_t lo = (tag & 1u) | ((tag >> 7) & 2u) | ((tag >> 14) & 4u);
	const uint32_t hi = ((tag >> 1) ^ (tag >> 9) ^ (tag >> 17)) & 1u;
	return (lo | (hi << 3)) & (n_sets - 1u);
}

} // namespace ngp
