// csrc/occ_index.h on the host: prints the number of violations (0 = pass).
// The reference layout is the Morton-ordered bitfield: cell (x, y, z) of cascade mip is bit morton3D(x, y, z) & 7 of byte
// mip * 128^3 / 8 + morton3D(x, y, z) / 8. A bitfield with a pattern of its own in every byte is laid out as coarse_occupancy_kernel
// lays out the block words (word occ_block4_of_block(bx, by, bz) of a cascade = the 8 bytes at Morton block morton3D(bx, by, bz)); then, for
// every cell of the 128^3 grid and every cascade,
//  - the word occ_block_word(mip, occ_block4(x, y, z)) and the bit occ_bit_in_block(x, y, z) address the cell's own bit: the same VALUE as
//    the reference, and -- with a single bit set per probe cell -- the same bit;
//  - occ_block4 is the low 15 bits of the march's block key, below 32768, and one-to-one with the Morton block (so a summary bit stands for
//    exactly the 64 cells of one Morton block); occ_block16 is below 512 and constant exactly over the 64 blocks of a 16^3 block;
//  - occ_summary4_word / occ_summary16_word stay inside [mip][1024] / [mip][16].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "occ_index.h"

int main() {
	using namespace ngp;
	const uint32_t G = OCC_GRIDSIZE, N = G * G * G, MIPS = 8;
	unsigned long long bad = 0;
	std::vector<uint8_t> bitfield((size_t)N / 8 * MIPS);
	uint32_t r = 12345u;
	for (auto& b : bitfield) { r = r * 1664525u + 1013904223u; b = (uint8_t)(r >> 24); }
	std::vector<uint64_t> words((size_t)OCC_BLOCKS_PER_MIP * MIPS);
	std::vector<uint32_t> to_morton(OCC_BLOCKS_PER_MIP, 0xffffffffu);
	for (uint32_t mip = 0; mip < MIPS; ++mip)
		for (uint32_t bz = 0; bz < 32; ++bz)
			for (uint32_t by = 0; by < 32; ++by)
				for (uint32_t bx = 0; bx < 32; ++bx) {
					const uint32_t b = occ_block4_of_block(bx, by, bz), m = occ_morton3D(bx, by, bz);
					bad += b >= OCC_BLOCKS_PER_MIP;
					if (mip == 0) { bad += to_morton[b] != 0xffffffffu; to_morton[b] = m; } // one-to-one
					memcpy(&words[occ_block_word(mip, b)], &bitfield[(size_t)N / 8 * mip + (size_t)m * 8], 8);
				}
	for (uint32_t mip = 0; mip < MIPS; ++mip)
		for (uint32_t z = 0; z < G; ++z)
			for (uint32_t y = 0; y < G; ++y)
				for (uint32_t x = 0; x < G; ++x) {
					const uint32_t idx = occ_morton3D(x, y, z);
					const uint32_t ref = (bitfield[idx / 8 + (size_t)(N / 8) * mip] >> (idx % 8)) & 1u;
					const uint32_t b4 = occ_block4(x, y, z), b16 = occ_block16(x, y, z), bit = occ_bit_in_block(x, y, z);
					bad += b4 >= OCC_BLOCKS_PER_MIP || b16 >= 512u || bit >= 64u;
#ifndef NGP_ROUND_V1
					bad += b4 != (((x >> 2) | ((y >> 2) << 5) | ((z >> 2) << 10))); // the low 15 bits of OccBlock::key
#endif
					bad += to_morton[b4] != idx >> 6;          // the block of the summary is the cell's Morton block ...
					bad += bit != (idx & 63u);                 // ... and the bit inside its word is the cell's
					bad += ((words[occ_block_word(mip, b4)] >> bit) & 1u) != ref;
					bad += occ_block_word(mip, b4) >= words.size();
					bad += occ_summary4_word(mip, b4) != mip * 1024u + (b4 >> 5) || occ_summary16_word(mip, b16) != mip * 16u + (b16 >> 5);
					// a 16^3 block: the same for two cells iff their Morton codes agree above bit 12
					bad += b16 != occ_block16(x & ~15u, y & ~15u, z & ~15u);
					if (mip == 0 && (x & 15u) == 0 && (y & 15u) == 0 && (z & 15u) == 0)
						for (uint32_t o = 0; o < 3; ++o) { // the neighbouring 16^3 blocks are other blocks
							const uint32_t nx = x + (o == 0 ? 16u : 0u), ny = y + (o == 1 ? 16u : 0u), nz = z + (o == 2 ? 16u : 0u);
							if (nx < G && ny < G && nz < G) bad += occ_block16(nx, ny, nz) == b16;
						}
				}
	// single-bit probes: setting the addressed bit of an all-zero table sets exactly the reference bit
	for (uint32_t k = 0; k < 4096; ++k) {
		r = r * 1664525u + 1013904223u;
		const uint32_t x = (r >> 3) & 127u, y = (r >> 11) & 127u, z = (r >> 19) & 127u, mip = r >> 29;
		const uint64_t w = 1ull << occ_bit_in_block(x, y, z);
		uint8_t bytes[8];
		memcpy(bytes, &w, 8);
		const uint32_t idx = occ_morton3D(x, y, z);
		for (uint32_t j = 0; j < 8; ++j) bad += bytes[j] != ((idx / 8) % 8 == j ? (uint8_t)(1u << (idx % 8)) : 0);
		(void)mip;
	}
	printf("%llu\n", bad);
	return bad ? 1 : 0;
}
