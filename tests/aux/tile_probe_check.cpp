// csrc/tile_probe.h on the host: tile_probe_check <in> <out>.
// in:  uint32 n_cameras; 128^3 bytes, cell (x, y, z) at x + 128 y + 128^2 z (0 / 1: occupied); per camera 12 floats (the 3 x 4 matrix, column
//      by column), int32 width, height, float focal_x, focal_y.
// out: NEAR_WORDS uint32 (near4, then near2, as near_table_word builds them from the Morton-ordered bitfield); per camera uint32 n_tiles,
//      uint32 false_culls, then one byte a tile: 0 kept, 1 no ray reaches the cube, 2 / 4 culled at that granularity.
// Every pixel's ray is formed as init_ray forms a plain pinhole camera's (pixel centres, unit direction, render box = the unit cube, a ray
// that misses it is not alive) and the tile's 64 rays are laid out lane by lane as the render kernel deals them (four 4 x 4 strips).
// false_culls: rays of culled tiles that, traversed in float64 through the 128^3 grid from their start on -- cell by cell, the cell of a
// position being its coordinates times 128 truncated towards zero, as in the march -- meet an occupied cell. It must be 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tile_probe.h"

using namespace ngp;

static const std::vector<uint8_t>* g_occ;

static bool cell_occupied(int x, int y, int z) { // truncation towards zero: (-1, 0) is cell 0
	if (x < 0) x = 0;
	if (y < 0) y = 0;
	if (z < 0) z = 0;
	if (x > 127 || y > 127 || z > 127) return false;
	return (*g_occ)[(size_t)x + 128u * (size_t)y + 16384u * (size_t)z] != 0;
}

// float64 traversal of o + d t, t >= t0, through the cells whose floor index is in [-1, 127]: true if one of them is occupied
static bool ray_meets_occupied(const float* of, const float* df, float t0f) {
	const double o[3] = {of[0], of[1], of[2]}, d[3] = {df[0], df[1], df[2]};
	const double lo = -1.0 / 128.0, hi = 1.0;
	double tn = t0f, tf = 1e300;
	for (int k = 0; k < 3; ++k) {
		if (d[k] == 0.0) {
			if (o[k] <= lo || o[k] >= hi) return false;
		} else {
			const double a = (lo - o[k]) / d[k], b = (hi - o[k]) / d[k];
			tn = std::fmax(tn, std::fmin(a, b));
			tf = std::fmin(tf, std::fmax(a, b));
		}
	}
	if (!(tn < tf)) return false;
	double t = tn;
	for (int guard = 0; guard < 1000 && t < tf; ++guard) {
		// the next plane k / 128 that the ray crosses behind t, per axis
		double t_next = tf;
		for (int k = 0; k < 3; ++k) {
			if (d[k] == 0.0) continue;
			const double p = (o[k] + d[k] * t) * 128.0;
			double plane = d[k] > 0.0 ? std::floor(p) + 1.0 : std::ceil(p) - 1.0;
			double tc = (plane / 128.0 - o[k]) / d[k];
			if (tc <= t) { plane += d[k] > 0.0 ? 1.0 : -1.0; tc = (plane / 128.0 - o[k]) / d[k]; } // (t sits on a plane)
			if (tc < t_next) t_next = tc;
		}
		const double tm = 0.5 * (t + t_next);
		const int x = (int)std::floor((o[0] + d[0] * tm) * 128.0), y = (int)std::floor((o[1] + d[1] * tm) * 128.0), z = (int)std::floor((o[2] + d[2] * tm) * 128.0);
		if (cell_occupied(x, y, z)) return true;
		t = t_next;
	}
	return false;
}

int main(int argc, char** argv) {
	if (argc != 3) return 2;
	FILE* f = fopen(argv[1], "rb");
	if (!f) return 2;
	uint32_t n_cams = 0;
	std::vector<uint8_t> occ(128u * 128u * 128u);
	if (fread(&n_cams, 4, 1, f) != 1 || fread(occ.data(), 1, occ.size(), f) != occ.size()) return 2;
	g_occ = &occ;
	std::vector<uint8_t> bitfield(128u * 128u * 128u / 8u, 0);
	for (uint32_t z = 0; z < 128; ++z)
		for (uint32_t y = 0; y < 128; ++y)
			for (uint32_t x = 0; x < 128; ++x)
				if (occ[x + 128u * y + 16384u * z]) {
					const uint32_t m = probe_morton3D(x, y, z);
					bitfield[m >> 3] |= (uint8_t)(1u << (m & 7u));
				}
	std::vector<uint32_t> near(NEAR_WORDS);
	for (uint32_t w = 0; w < NEAR_WORDS; ++w) near[w] = w < NEAR4_WORDS ? near_table_word(bitfield.data(), 4u, w) : near_table_word(bitfield.data(), 2u, w - NEAR4_WORDS);
	FILE* out = fopen(argv[2], "wb");
	if (!out) return 2;
	fwrite(near.data(), 4, near.size(), out);
	for (uint32_t c = 0; c < n_cams; ++c) {
		float m[12], focal[2];
		int32_t wh[2];
		if (fread(m, 4, 12, f) != 12 || fread(wh, 4, 2, f) != 2 || fread(focal, 4, 2, f) != 2) return 2;
		const uint32_t W = (uint32_t)wh[0], H = (uint32_t)wh[1], tiles_x = (W + 7u) / 8u, tiles_y = (H + 7u) / 8u, n_tiles = tiles_x * tiles_y;
		std::vector<uint8_t> decision(n_tiles);
		uint32_t false_culls = 0;
		for (uint32_t tile = 0; tile < n_tiles; ++tile) {
			float o[64][3], d[64][3], t0[64];
			bool valid[64];
			for (uint32_t lane = 0; lane < 64; ++lane) {
				const uint32_t s4 = lane >> 4, i16 = lane & 15u, slot = ((s4 >> 1) * 4u + (i16 >> 2)) * 8u + (s4 & 1u) * 4u + (i16 & 3u);
				const uint32_t x = (tile % tiles_x) * 8u + (slot & 7u), y = (tile / tiles_x) * 8u + (slot >> 3);
				valid[lane] = false;
				for (int k = 0; k < 3; ++k) o[lane][k] = d[lane][k] = 0.0f;
				t0[lane] = 0.0f;
				if (x >= W || y >= H) continue;
				const float u = ((float)x + 0.5f) / (float)W, v = ((float)y + 0.5f) / (float)H;
				const float cx = (u - 0.5f) * (float)W / focal[0], cy = (v - 0.5f) * (float)H / focal[1];
				float dir[3];
				for (int k = 0; k < 3; ++k) dir[k] = m[k] * cx + m[3 + k] * cy + m[6 + k];
				const float len = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
				float tn = 0.0f, tf = 1e30f;
				for (int k = 0; k < 3; ++k) {
					dir[k] /= len;
					o[lane][k] = m[9 + k];
					d[lane][k] = dir[k];
					const float a = (0.0f - m[9 + k]) / dir[k], b = (1.0f - m[9 + k]) / dir[k]; // (the render box: the unit cube)
					tn = std::fmax(tn, std::fmin(a, b));
					tf = std::fmin(tf, std::fmax(a, b));
				}
				if (!(tn < tf)) continue;
				t0[lane] = tn + 1e-6f;
				valid[lane] = true;
			}
			const TileProbeResult R = tile_probe_host(o, d, t0, valid, 15u, near.data());
			decision[tile] = !R.empty ? 0 : (R.g == 0u ? 1 : (uint8_t)R.g);
			if (R.empty)
				for (uint32_t lane = 0; lane < 64; ++lane)
					if (valid[lane] && ray_meets_occupied(o[lane], d[lane], t0[lane])) ++false_culls;
		}
		fwrite(&n_tiles, 4, 1, out);
		fwrite(&false_culls, 4, 1, out);
		fwrite(decision.data(), 1, decision.size(), out);
	}
	fclose(out);
	fclose(f);
	return 0;
}
