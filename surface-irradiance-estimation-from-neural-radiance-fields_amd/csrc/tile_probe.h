// Does any ray of an 8 x 8 camera tile meet an occupied cell of cascade 0? A conservative test that the unit render kernels run once per
// tile, right after ray setup (nerf_kernels.hip, refill): a tile that provably emits no sample is dropped before it marches. Plain C++, so
// that tests/aux/tile_probe_check.cpp runs the same functions on the host against a float64 traversal of every ray.
//
// Tables ("near occupancy", built by near_occupancy_kernel behind the block words of ModelParams::coarse, cascade 0 only, plain coordinates):
//   near4: 32^3 bits, bit bx | by << 5 | bz << 10 = some 4^3 block of cells in the 3 x 3 x 3 neighbourhood of block (bx, by, bz) holds an occupied cell;
//   near2: 64^3 bits, bit bx | by << 6 | bz << 12 = the same for 2^3 blocks.
//
// The probe, for the (up to 64) rays o_j + d_j t of a tile, |d_j| = 1, marched from t >= t0_j; the axis ray a is the ray of a central pixel:
//   1. every ray clips itself to the cube [-1/128 - eps, 1 + eps]^3 (the march truncates pos * 128 towards zero, so cell 0 also answers for
//      (-1/128, 0)), from t0_j on: [tn_j, tf_j]; rays that miss it take no further part, and a tile without any other is empty. The axis ray
//      clips itself to that cube padded by four more cells, from t = 0 on: [T_n, T_f]. If the axis ray is no ray of the frame, or misses the
//      padded cube, or some [tn_j, tf_j] is not inside [T_n, T_f], the tile is kept. (The distance between two lines is bounded by its
//      values at the ends of an interval only inside that interval, hence the test; a ray within four cells of the axis passes it.)
//   2. dev_j = max over t in {T_n, T_f} of |(o_j + d_j t) - (o_a + d_a t)|_inf: the difference is affine in t, so this bounds it on all
//      of [T_n, T_f]. D = max dev_j.
//   3. N points on the axis, t_k = T_n + (k + 1/2) s, s = (T_f - T_n) / N: every t of the range is within s / 2 of one.
//   4. r = D + s / 2 + eps. r <= 2/128: g = 2 cells; else r <= 4/128: g = 4 cells; else the tile is kept. N = 64 if that reaches the finer
//      granularity, else 128.
//   5. the tile is empty iff no point lies in a set bit of near_g. A point's block is floor(q * 128 / g) per coordinate; below -2 or above
//      128 / g the point is too far from the grid to matter, -2, -1 and 128 / g are clamped into the table.
// Nothing in it is reduced across the rays but by votes (all rays inside the range, all rays within r): a wave decides it with ballots.
// Why no occupied cell is missed: a point p of ray j in an occupied cell has t in [tn_j, tf_j], so in [T_n, T_f], lies within dev_j of the
// axis point at t and so within r - eps < g / 128 of some probe point q. Then floor(q / g) differs from floor(p / g) by at most one per coordinate, p's block
// under truncation is max(floor(p / g), 0), and clamping floor(q / g) keeps it within one of that: the dilated bit of q's block is set.
// eps = 1/1024 (an eighth of a cell) stands for the fp32 error of o + d t, of the clip and of the block index, ~1e-6 each for |t| <= 4.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGP_PROBE_FN __host__ __device__ __forceinline__
#else
#define NGP_PROBE_FN inline
#endif

namespace ngp {

constexpr uint32_t NEAR4_SIDE = 32u, NEAR2_SIDE = 64u;
constexpr uint32_t NEAR4_WORDS = NEAR4_SIDE * NEAR4_SIDE * NEAR4_SIDE / 32u; // 1024
constexpr uint32_t NEAR2_WORDS = NEAR2_SIDE * NEAR2_SIDE * NEAR2_SIDE / 32u; // 8192
constexpr uint32_t NEAR_WORDS = NEAR4_WORDS + NEAR2_WORDS;                   // near4 first
constexpr float TILE_PROBE_EPS = 1.0f / 1024.0f;
constexpr float TILE_PROBE_CELL = 1.0f / 128.0f;

NGP_PROBE_FN uint32_t probe_expand_bits(uint32_t v) { // tcnn's expand_bits
	v = (v * 0x00010001u) & 0xFF0000FFu;
	v = (v * 0x00000101u) & 0x0F00F00Fu;
	v = (v * 0x00000011u) & 0xC30C30C3u;
	v = (v * 0x00000005u) & 0x49249249u;
	return v;
}
NGP_PROBE_FN uint32_t probe_morton3D(uint32_t x, uint32_t y, uint32_t z) { return probe_expand_bits(x) | (probe_expand_bits(y) << 1) | (probe_expand_bits(z) << 2); }

// does the g^3 block (bx, by, bz) of cascade 0 hold an occupied cell? (g = 2: one byte of the Morton-ordered bitfield, g = 4: eight)
NGP_PROBE_FN bool near_block_occupied(const uint8_t* bitfield, uint32_t g, uint32_t bx, uint32_t by, uint32_t bz) {
	const uint32_t m = probe_morton3D(bx, by, bz);
	if (g == 2u) return bitfield[m] != 0;
	uint32_t any = 0;
	for (uint32_t k = 0; k < 8u; ++k) any |= bitfield[m * 8u + k];
	return any != 0u;
}
// word w of near_g: its 32 bits are the blocks bx = 32 (w % (side / 32)) .., by, bz in the table's order.
// Cost: written for the host check to share, not for speed -- a thread of near_occupancy_kernel reads up to 32 x 27 blocks (x 8 bytes at g = 4)
// of the 256 KB of cascade 0, which the caches hold, with an early exit at the first occupied neighbour; 9216 threads, once per model load
// and per training occupancy refresh (every 16 steps: the training rate did not move, 1227 / 1228 steps/s). Block bits first and a
// dilation by shifts would read each byte once; not done while the refresh does not show it.
NGP_PROBE_FN uint32_t near_table_word(const uint8_t* bitfield, uint32_t g, uint32_t w) {
	const uint32_t side = 128u / g, wx = side / 32u;
	const uint32_t bx0 = (w % wx) * 32u, by = (w / wx) % side, bz = w / (wx * side);
	uint32_t bits = 0;
	for (uint32_t b = 0; b < 32u; ++b) {
		const uint32_t bx = bx0 + b;
		bool any = false;
		for (int dz = -1; dz <= 1 && !any; ++dz)
			for (int dy = -1; dy <= 1 && !any; ++dy)
				for (int dx = -1; dx <= 1 && !any; ++dx) {
					const uint32_t x = bx + (uint32_t)dx, y = by + (uint32_t)dy, z = bz + (uint32_t)dz; // (a negative coordinate wraps above side)
					if (x < side && y < side && z < side) any = near_block_occupied(bitfield, g, x, y, z);
				}
		bits |= (any ? 1u : 0u) << b;
	}
	return bits;
}

NGP_PROBE_FN float probe_min(float a, float b) { return a < b ? a : b; }
NGP_PROBE_FN float probe_max(float a, float b) { return a > b ? a : b; }
NGP_PROBE_FN float probe_abs(float a) { return a < 0.0f ? -a : a; }

// step 1: the ray's [tn, tf] inside the inflated cube, from t0 on (false: it misses the cube), and its [Tn, Tf] inside the padded cube,
// from 0 on (Tn > Tf: it misses that one): what the ray contributes if it is the tile's axis
constexpr float TILE_PROBE_PAD = 4.0f / 128.0f;
NGP_PROBE_FN bool tile_probe_ray_range(float ox, float oy, float oz, float dx, float dy, float dz, float t0, float& tn, float& tf, float& Tn, float& Tf) {
	const float lo = -(TILE_PROBE_CELL + TILE_PROBE_EPS), hi = 1.0f + TILE_PROBE_EPS;
	const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
	bool hit = true;
	tn = t0;
	tf = 1e30f;
	Tn = 0.0f;
	Tf = 1e30f;
	for (int k = 0; k < 3; ++k) {
		if (probe_abs(d[k]) < 1e-12f) { // parallel to the slab (and no division whose result may be infinite)
			if (o[k] < lo || o[k] > hi) hit = false;
			if (o[k] < lo - TILE_PROBE_PAD || o[k] > hi + TILE_PROBE_PAD) Tf = -1e30f;
		} else {
			const float inv = 1.0f / d[k];
			const float t1 = (lo - o[k]) * inv, t2 = (hi - o[k]) * inv;
			tn = probe_max(tn, probe_min(t1, t2));
			tf = probe_min(tf, probe_max(t1, t2));
			const float T1 = (lo - TILE_PROBE_PAD - o[k]) * inv, T2 = (hi + TILE_PROBE_PAD - o[k]) * inv;
			Tn = probe_max(Tn, probe_min(T1, T2));
			Tf = probe_min(Tf, probe_max(T1, T2));
		}
	}
	return hit && tn <= tf;
}
// step 2: |ray - axis|_inf at t
NGP_PROBE_FN float tile_probe_dev_at(float ox, float oy, float oz, float dx, float dy, float dz, float ax, float ay, float az, float adx, float ady, float adz, float t) {
	const float ex = (ox + dx * t) - (ax + adx * t), ey = (oy + dy * t) - (ay + ady * t), ez = (oz + dz * t) - (az + adz * t);
	return probe_max(probe_max(probe_abs(ex), probe_abs(ey)), probe_abs(ez));
}
// step 4: the granularity (2 or 4 cells; 0: keep the tile) and the number of points (64 or 128) for deviation D and range length len
NGP_PROBE_FN uint32_t tile_probe_plan(float D, float len, uint32_t& n_points) {
	const float r64 = D + len * (0.5f / 64.0f) + TILE_PROBE_EPS, r128 = D + len * (0.5f / 128.0f) + TILE_PROBE_EPS;
	n_points = 128u;
	if (r128 <= 2.0f * TILE_PROBE_CELL) {
		if (r64 <= 2.0f * TILE_PROBE_CELL) n_points = 64u;
		return 2u;
	}
	if (r128 <= 4.0f * TILE_PROBE_CELL) {
		if (r64 <= 4.0f * TILE_PROBE_CELL) n_points = 64u;
		return 4u;
	}
	return 0u;
}
// step 5 for one point: the index of its bit in `near` (the two tables, near4 first), or 0xffffffff where the point is too far from the grid
NGP_PROBE_FN uint32_t tile_probe_bit(float qx, float qy, float qz, uint32_t g) {
	const float scale = g == 2u ? 64.0f : 32.0f, side = scale;
	const float q[3] = {qx * scale, qy * scale, qz * scale};
	uint32_t b[3];
	for (int k = 0; k < 3; ++k) {
		if (!(q[k] >= -2.0f && q[k] < side + 1.0f)) return 0xffffffffu; // floor(q) in [-2, side]; a NaN is too far as well
		const float c = probe_min(probe_max(q[k], 0.0f), side - 1.0f);  // floor of the clamped value == the clamped floor
		b[k] = (uint32_t)(int)c;
	}
	return g == 2u ? NEAR4_WORDS * 32u + (b[0] | (b[1] << 6) | (b[2] << 12)) : (b[0] | (b[1] << 5) | (b[2] << 10));
}
NGP_PROBE_FN bool tile_probe_point_set(const uint32_t* near, float qx, float qy, float qz, uint32_t g) {
	const uint32_t bit = tile_probe_bit(qx, qy, qz, g);
	return bit != 0xffffffffu && ((near[bit >> 5] >> (bit & 31u)) & 1u) != 0u;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole probe for one tile on the host, step for step what the kernel does with a wave (lane j = ray j; `central`: the lane of the
// central pixel). valid[j]: the ray is alive after ray setup. Returns 1: the tile is empty.
struct TileProbeResult {
	int empty;
	uint32_t g, n_points;
	float D, Tn, Tf;
};
inline TileProbeResult tile_probe_host(const float (*o)[3], const float (*d)[3], const float* t0, const bool* valid, uint32_t central, const uint32_t* near) {
	TileProbeResult R = {1, 0u, 0u, 0.0f, 0.0f, 0.0f};
	bool in[64], any = false;
	float tn[64], tf[64], Tn[64], Tf[64];
	for (int j = 0; j < 64; ++j) {
		in[j] = valid[j] && tile_probe_ray_range(o[j][0], o[j][1], o[j][2], d[j][0], d[j][1], d[j][2], t0[j], tn[j], tf[j], Tn[j], Tf[j]);
		any = any || in[j];
	}
	if (!any) return R; // no ray reaches the cube
	R.empty = 0;
	const int a = (int)central;
	if (!in[a]) return R;
	R.Tn = Tn[a];
	R.Tf = Tf[a];
	for (int j = 0; j < 64; ++j) {
		if (!in[j]) continue;
		if (!(tn[j] >= R.Tn && tf[j] <= R.Tf)) return R; // a ray crosses the cube where the axis ray is outside the padded one
		for (int e = 0; e < 2; ++e)
			R.D = probe_max(R.D, tile_probe_dev_at(o[j][0], o[j][1], o[j][2], d[j][0], d[j][1], d[j][2], o[a][0], o[a][1], o[a][2], d[a][0], d[a][1], d[a][2], e ? R.Tf : R.Tn));
	}
	R.g = tile_probe_plan(R.D, R.Tf - R.Tn, R.n_points);
	if (R.g == 0u) return R;
	const float s = (R.Tf - R.Tn) / (float)R.n_points;
	for (uint32_t k = 0; k < R.n_points; ++k) {
		const float t = R.Tn + ((float)k + 0.5f) * s;
		if (tile_probe_point_set(near, o[a][0] + d[a][0] * t, o[a][1] + d[a][1] * t, o[a][2] + d[a][2] * t, R.g)) return R;
	}
	R.empty = 1;
	return R;
}
#endif

} // namespace ngp
