// Where the march finds a cell's occupancy without a Morton code: the indices of the derived occupancy tables (plain C++, so that
// tests/aux/occ_index_check.cpp can check them on the host against morton3D and the Morton-ordered bitfield).
//
// The bitfield itself (ModelParams::bitfield, what the API and the snapshots see) stays in Morton order: cell (x, y, z) of cascade `mip`
// is bit morton3D(x, y, z) of that cascade's 128^3 bits, so a 4^3 block of cells is one aligned 8-byte word of it. Derived from it when
// it changes (coarse_occupancy_kernel) and indexed by the block's COORDINATES instead:
//   - the 4^3 summary, [mip][1024] words: bit occ_block4(x, y, z) = the block around the cell holds an occupied cell;
//   - the 16^3 summary, [mip][16] words: bit occ_block16(x, y, z);
//   - a copy of the bitfield's block words, [mip][32768] x 8 bytes: word occ_block4(x, y, z) of a cascade is the word
//     morton3D(x >> 2, y >> 2, z >> 2) of the bitfield, bit for bit, so the cell is still bit occ_bit_in_block(x, y, z) of it.
// occ_block4 is also the low 15 bits of the key under which a marching lane keeps its block (nerf_device.h OccBlock).
// -DNGP_ROUND_V1: the tables in Morton order, as they were (no copy of the block words: the bitfield is read).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGP_OCC_FN __host__ __device__ __forceinline__
#else
#define NGP_OCC_FN inline
#endif

namespace ngp {

constexpr uint32_t OCC_GRIDSIZE = 128u;                                                             // cells per side of a cascade (NERF_GRIDSIZE)
constexpr uint32_t OCC_BLOCKS_PER_MIP = (OCC_GRIDSIZE / 4u) * (OCC_GRIDSIZE / 4u) * (OCC_GRIDSIZE / 4u); // 32768 4^3 blocks = 8-byte words
constexpr uint32_t OCC_SUMMARY4_WORDS_PER_MIP = OCC_BLOCKS_PER_MIP / 32u;                           // 1024
constexpr uint32_t OCC_SUMMARY16_WORDS_PER_MIP = 16u;                                               // 8^3 blocks of 16^3 cells = 512 bits

NGP_OCC_FN uint32_t occ_expand_bits(uint32_t v) { // tcnn's expand_bits: bit i of a 10-bit value moves to bit 3 i
	v = (v * 0x00010001u) & 0xFF0000FFu;
	v = (v * 0x00000101u) & 0x0F00F00Fu;
	v = (v * 0x00000011u) & 0xC30C30C3u;
	v = (v * 0x00000005u) & 0x49249249u;
	return v;
}
NGP_OCC_FN uint32_t occ_morton3D(uint32_t x, uint32_t y, uint32_t z) { return occ_expand_bits(x) | (occ_expand_bits(y) << 1) | (occ_expand_bits(z) << 2); }

// cell coordinates (each below OCC_GRIDSIZE) -> index of the cell's 4^3 block / 16^3 block within its cascade
#ifdef NGP_ROUND_V1
NGP_OCC_FN uint32_t occ_block4(uint32_t x, uint32_t y, uint32_t z) { return occ_morton3D(x >> 2, y >> 2, z >> 2); }
NGP_OCC_FN uint32_t occ_block16(uint32_t x, uint32_t y, uint32_t z) { return occ_morton3D(x >> 4, y >> 4, z >> 4); }
#else
NGP_OCC_FN uint32_t occ_block4(uint32_t x, uint32_t y, uint32_t z) { return (x >> 2) | ((y >> 2) << 5) | ((z >> 2) << 10); }
NGP_OCC_FN uint32_t occ_block16(uint32_t x, uint32_t y, uint32_t z) { return (x >> 4) | ((y >> 4) << 3) | ((z >> 4) << 6); }
#endif
// the same from the coordinates of a 4^3 block (each below 32)
NGP_OCC_FN uint32_t occ_block4_of_block(uint32_t bx, uint32_t by, uint32_t bz) { return occ_block4(bx << 2, by << 2, bz << 2); }
NGP_OCC_FN uint32_t occ_block16_of_block(uint32_t bx, uint32_t by, uint32_t bz) { return occ_block16(bx << 2, by << 2, bz << 2); }
// the cell's bit in its block's 8-byte word: the Morton code of the coordinates' low two bits (in either layout)
NGP_OCC_FN uint32_t occ_bit_in_block(uint32_t x, uint32_t y, uint32_t z) {
	return (x & 1u) | ((y & 1u) << 1) | ((z & 1u) << 2) | ((x & 2u) << 2) | ((y & 2u) << 3) | ((z & 2u) << 4);
}
// index of a block's 8-byte word in the copy of the block words / of the word and bit of a summary that answer for a block
NGP_OCC_FN uint32_t occ_block_word(uint32_t mip, uint32_t block) { return mip * OCC_BLOCKS_PER_MIP + block; }
NGP_OCC_FN uint32_t occ_summary4_word(uint32_t mip, uint32_t block4) { return mip * OCC_SUMMARY4_WORDS_PER_MIP + (block4 >> 5); }
NGP_OCC_FN uint32_t occ_summary16_word(uint32_t mip, uint32_t block16) { return mip * OCC_SUMMARY16_WORDS_PER_MIP + (block16 >> 5); }

} // namespace ngp
