// Marching cubes: the 256-case triangle table and the lattice descriptions shared by mc_kernels.hip and ngp_mc.cpp.
#pragma once

#include <stdint.h>

namespace ngp {

// The 256-case table, generated at compile time by one rule so that it can be restated exactly (tests/test_marching_cubes.py):
//   corner c = x + 2y + 4z; edge 4a + u + 2v runs along axis a from the corner whose other two coordinates, in axis order, are (u, v).
//   On each face, walked counter-clockwise about its outward normal, every maximal run of dense corners contributes one segment
//   from the crossing where the walk enters the run to the crossing where it leaves it. A face with two dense corners on a diagonal
//   therefore keeps them apart -- a decision that depends on the face's four corners alone, so the two cells that share the face make
//   the same one and a closed surface comes out watertight.
//   The segments join into loops (each crossed edge starts one segment and ends another); loops are taken in the order of their
//   smallest edge id and fanned from it into triangles, whose counter-clockwise normal then points from the dense side to the empty one.
// At most 5 triangles per case, as in the classic table.
struct McTable {
	uint8_t n[256];      // triangles of the case
	uint8_t e[256][15];  // their edges, three per triangle
};

constexpr int mc_edge_id(int p, int q) {
	const int x = p ^ q, a = x == 1 ? 0 : (x == 2 ? 1 : 2), lo = p & q;
	const int c0 = lo & 1, c1 = (lo >> 1) & 1, c2 = (lo >> 2) & 1;
	const int u = a == 0 ? c1 : c0, v = a == 2 ? c1 : c2;
	return 4 * a + u + 2 * v;
}

constexpr McTable make_mc_table() {
	McTable T{};
	int cyc[6][4] = {};
	for (int a = 0; a < 3; ++a) {
		const int b = a == 0 ? 1 : 0, c = a == 2 ? 1 : 2;
		for (int s = 0; s < 2; ++s) {
			const int pu[4] = {0, 1, 1, 0}, pv[4] = {0, 0, 1, 1}; // counter-clockwise about +a when (b, c, a) is right-handed (a != 1)
			const bool reverse = (a != 1) != (s == 1);
			for (int i = 0; i < 4; ++i) {
				const int k = reverse ? 3 - i : i;
				int xyz[3] = {0, 0, 0};
				xyz[a] = s; xyz[b] = pu[k]; xyz[c] = pv[k];
				cyc[2 * a + s][i] = xyz[0] + 2 * xyz[1] + 4 * xyz[2];
			}
		}
	}
	for (int cs = 0; cs < 256; ++cs) {
		int nxt[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
		for (int f = 0; f < 6; ++f) {
			int ins[4] = {};
			int n_in = 0;
			for (int i = 0; i < 4; ++i) { ins[i] = (cs >> cyc[f][i]) & 1; n_in += ins[i]; }
			if (n_in == 0 || n_in == 4) continue;
			for (int i = 0; i < 4; ++i) {
				if (!ins[i] || ins[(i + 3) % 4]) continue;
				int j = i;
				while (ins[(j + 1) % 4]) ++j;
				nxt[mc_edge_id(cyc[f][(i + 3) % 4], cyc[f][i])] = mc_edge_id(cyc[f][j % 4], cyc[f][(j + 1) % 4]);
			}
		}
		bool seen[12] = {};
		int nt = 0;
		for (int s = 0; s < 12; ++s) {
			if (nxt[s] < 0 || seen[s]) continue;
			int loop[12] = {}, len = 0;
			for (int e = s; !seen[e]; e = nxt[e]) { seen[e] = true; loop[len++] = e; }
			for (int k = 1; k + 1 < len; ++k) {
				T.e[cs][3 * nt + 0] = (uint8_t)loop[0];
				T.e[cs][3 * nt + 1] = (uint8_t)loop[k];
				T.e[cs][3 * nt + 2] = (uint8_t)loop[k + 1];
				++nt;
			}
		}
		T.n[cs] = (uint8_t)nt;
	}
	return T;
}

// the lattice of the contract (include/ngp_hip.h): point (i, j, k) at R^T (lo + ext * (i, j, k) / rm1), R column-major
struct McLattice {
	uint32_t res[3];
	float lo[3], ext[3], rm1[3]; // rm1 = res - 1
	float r2l[9];                // row r of R^T = column r of R: r2l[3 r + k]
};
// a lattice of densities in device memory (x fastest), padded with zeros to a multiple of 4 values
struct McGrid {
	const float* d;
	uint32_t rx, ry, rz, n;
	float thresh;
};

} // namespace ngp
