// csrc/cell_cache.h on the host: prints the number of violations (0 = pass).
//  - every cell with all coordinates <= CELL_COORD_MAX is cacheable, its tag is below 2^24 (so never CELL_TAG_NONE) and unpacks to the cell;
//  - a cell with any coordinate above it -- up to 2^32 - 1: a hashed level's coord_max, a level finer than 256 cells across at any
//    N_min / per_level_scale the loader accepts -- is not cacheable, so it never meets the tag at all;
//  - cell_set stays inside the cache for 4, 8 and 16 sets, and from 8 sets on the 8 cells of a 2 x 2 x 2 neighbourhood take 8 different sets.
#include <cstdint>
#include <cstdio>
#include "cell_cache.h"

int main() {
	using namespace ngp;
	unsigned long long bad = 0;
	for (uint32_t z = 0; z <= CELL_COORD_MAX; ++z)
		for (uint32_t y = 0; y <= CELL_COORD_MAX; ++y)
			for (uint32_t x = 0; x <= CELL_COORD_MAX; ++x) {
				const uint32_t t = cell_tag(x, y, z);
				bad += !cell_cacheable(x, y, z);
				bad += t >= (1u << 24) || t == CELL_TAG_NONE;
				bad += (t & 255u) != x || ((t >> 8) & 255u) != y || (t >> 16) != z; // one-to-one: the tag is the cell
				for (uint32_t s = 4; s <= 16; s *= 2) bad += cell_set(t, s) >= s;
			}
	const uint32_t beyond[] = {256u, 257u, 511u, 512u, 65535u, 65536u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFF00u, 0xFFFFFFFFu};
	for (uint32_t b : beyond)
		for (uint32_t o = 0; o <= CELL_COORD_MAX; o += 51) {
			bad += cell_cacheable(b, o, o);
			bad += cell_cacheable(o, b, o);
			bad += cell_cacheable(o, o, b);
			bad += cell_cacheable(b, b, b);
		}
	for (uint32_t s = 8; s <= 16; s *= 2)
		for (uint32_t z = 0; z < CELL_COORD_MAX; z += 3)
			for (uint32_t y = 0; y < CELL_COORD_MAX; y += 5)
				for (uint32_t x = 0; x < CELL_COORD_MAX; ++x) {
					uint32_t seen = 0;
					for (int c = 0; c < 8; ++c) seen |= 1u << cell_set(cell_tag(x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2)), s);
					bad += __builtin_popcount(seen) != 8;
				}
	printf("%llu\n", bad);
	return bad ? 1 : 0;
}
