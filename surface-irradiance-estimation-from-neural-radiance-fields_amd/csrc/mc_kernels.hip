// Marching-cubes mesh extraction from the NeRF density (Testbed::compute_marching_cubes_mesh; contract in include/ngp_hip.h).
//
//   mc_density_grid_kernel   the activated density on a res_x x res_y x res_z lattice (grid models): one wave per 4x4x4 brick of
//                            lattice points, hash-grid encode + density head on MFMA as density_grid_samples_kernel runs them
//   mc_lattice_positions_kernel / mc_density_from_logits_kernel   the same lattice for the wide (Frequency / Identity) architecture,
//                            around network_inference_wide*
//   mc_count_kernel          per 1024-point block: vertices the block's points own (one per crossed edge to +x, +y, +z) and
//                            triangles its cells emit
//   mc_scan_kernel           one workgroup: exclusive scan of the block totals, 64-bit grand totals
//   mc_emit_vertices_kernel  per-point vertex offset + crossing mask, the vertices themselves
//   mc_emit_triangles_kernel the triangles; a corner edge's vertex index is its owner's offset plus the edge's rank among the
//                            owner's crossed axes
//   mc_vertex_inputs_kernel / mc_vertex_attributes_kernel   network inputs at the vertices, then normals and colours from the
//                            density-gradient and network-inference stages
// Every order is fixed by the scan: no atomics, so the output is bit-identical from run to run.
#include "render_common.h"
#include "mc_table.h"

namespace ngp {

void launch_network_inference_wide(const ModelParams& M, uint32_t n, const float* pos01, const float* dir01, uint16_t* out, int n_cus, hipStream_t stream); // wide_kernels.hip

namespace {
constexpr int MC_BLOCK = 256;
constexpr uint32_t MC_PTS = 4;                          // lattice points per thread (one float4 of the lattice)
constexpr uint32_t MC_BLOCK_PTS = MC_BLOCK * MC_PTS;    // points per block of the count / emit kernels
__constant__ McTable MC_TABLE = make_mc_table();

// the lattice point's position in ngp space: R^T (lo + ext * q / (res - 1))
NGP_DEV f3 mc_position(const McLattice& L, float qx, float qy, float qz) {
	const float lx = L.lo[0] + L.ext[0] * (qx / L.rm1[0]);
	const float ly = L.lo[1] + L.ext[1] * (qy / L.rm1[1]);
	const float lz = L.lo[2] + L.ext[2] * (qz / L.rm1[2]);
	return mk3(L.r2l[0] * lx + L.r2l[1] * ly + L.r2l[2] * lz, L.r2l[3] * lx + L.r2l[4] * ly + L.r2l[5] * lz,
	           L.r2l[6] * lx + L.r2l[7] * ly + L.r2l[8] * lz);
}
// (mc_warp, warp_position, lives in render_common.h: the frames' surface-normal pass forms its positions with it too)

// the values at flat indices base .. base + 4 (zero beyond the lattice): a float4 when base is 16-byte aligned
NGP_DEV void mc_load5(const float* __restrict__ d, uint32_t n, uint32_t base, float (&v)[5]) {
	if ((base & 3u) == 0 && base + 4u <= ((n + 3u) & ~3u)) { // (the lattice buffer is padded to a multiple of 4 values)
		const float4 a = *reinterpret_cast<const float4*>(d + base);
		v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
	} else {
#pragma unroll
		for (int x = 0; x < 4; ++x) v[x] = base + x < n ? d[base + x] : 0.0f;
	}
	v[4] = base + 4u < n ? d[base + 4u] : 0.0f;
}

// the four points p0 .. p0 + 3 of a thread: inside bits of the rows at +0, +rx, +rx*ry, +rx*ry+rx (5 values each) and coordinates
struct McQuad {
	uint32_t in[4]; // bit x of in[r]: value at p0 + row_offset(r) + x is above the threshold
	uint32_t i[4], j[4], k[4];
	float v0[5], vy[4], vz[4]; // values of row 0 and of the +y / +z neighbours (vertex positions)
};
template <int ROWS>
NGP_DEV void mc_load_quad(const McGrid& G, uint32_t p0, McQuad& Q) {
	const uint32_t sxy = G.rx * G.ry;
	const uint32_t offs[4] = {0u, G.rx, sxy, sxy + G.rx};
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		Q.in[r] = 0;
		if (r >= ROWS) continue;
		float v[5];
		mc_load5(G.d, G.n, p0 + offs[r], v);
#pragma unroll
		for (int x = 0; x < 5; ++x) Q.in[r] |= (v[x] > G.thresh ? 1u : 0u) << x;
		if (r == 0) for (int x = 0; x < 5; ++x) Q.v0[x] = v[x];
		if (r == 1) for (int x = 0; x < 4; ++x) Q.vy[x] = v[x];
		if (r == 2) for (int x = 0; x < 4; ++x) Q.vz[x] = v[x];
	}
	const uint32_t p = p0 < G.n ? p0 : 0u;
	uint32_t i = p % G.rx, jk = p / G.rx, j = jk % G.ry, k = jk / G.ry;
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		Q.i[q] = i; Q.j[q] = j; Q.k[q] = k;
		if (++i == G.rx) { i = 0; if (++j == G.ry) { j = 0; ++k; } }
	}
}
// crossed edges to +x, +y, +z of point q (bit a = axis a)
NGP_DEV uint32_t mc_vmask(const McGrid& G, const McQuad& Q, int q, uint32_t p0) {
	if (p0 + q >= G.n) return 0u;
	const uint32_t b = (Q.in[0] >> q) & 1u;
	uint32_t m = 0;
	if (Q.i[q] + 1 < G.rx && ((Q.in[0] >> (q + 1)) & 1u) != b) m |= 1u;
	if (Q.j[q] + 1 < G.ry && ((Q.in[1] >> q) & 1u) != b) m |= 2u;
	if (Q.k[q] + 1 < G.rz && ((Q.in[2] >> q) & 1u) != b) m |= 4u;
	return m;
}
// the cell whose lowest corner is point q: its case (corner c = x + 2y + 4z), or -1 where the point is on a far face
NGP_DEV int mc_case(const McGrid& G, const McQuad& Q, int q, uint32_t p0) {
	if (p0 + q >= G.n || Q.i[q] + 1 >= G.rx || Q.j[q] + 1 >= G.ry || Q.k[q] + 1 >= G.rz) return -1;
	int c = 0;
#pragma unroll
	for (int r = 0; r < 4; ++r) c |= (int)((Q.in[r] >> q) & 3u) << (2 * r);
	return c;
}

// exclusive prefix of a per-thread count below 2^BITS over the workgroup (ranks inside a wave by ballot + mbcnt), and the block total
template <int BITS>
NGP_DEV uint32_t mc_block_prefix(uint32_t v, uint32_t* s_wave, uint32_t& total) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint32_t below = 0, wsum = 0;
#pragma unroll
	for (int b = 0; b < BITS; ++b) {
		const unsigned long long m = __ballot((v >> b) & 1u);
		const uint32_t lo = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
		below += lo << b;
		wsum += (uint32_t)__popcll(m) << b;
	}
	__syncthreads();
	if (lane == 0) s_wave[wave] = wsum;
	__syncthreads();
	uint32_t before = 0;
	total = 0;
#pragma unroll
	for (int w = 0; w < MC_BLOCK / 64; ++w) {
		before += w < wave ? s_wave[w] : 0u;
		total += s_wave[w];
	}
	return before + below;
}
} // namespace

// ---- the lattice, grid models. Wave w takes brick (bx, by, bz) = w in x-fastest order, lane l its point (l & 3, (l >> 2) & 3, l >> 4):
// the 64 points of a wave are neighbours and their hash-grid gathers share cache lines
template <bool DLIN>
__global__ __launch_bounds__(MC_BLOCK) void mc_density_grid_kernel(const ModelParams M, const McLattice L, uint32_t n_bricks, float* __restrict__ out) {
	__shared__ uint4 s_w[FRAG_R0 * 64];
	__shared__ LevelInfo s_lv[N_LEVELS];
	for (int i = threadIdx.x; i < FRAG_R0 * 64; i += MC_BLOCK) s_w[i] = M.wfrags[i];
	if (threadIdx.x < N_LEVELS) s_lv[threadIdx.x] = M.levels[threadIdx.x];
	__syncthreads();
	const int lane = threadIdx.x & 63, c = lane & 15;
	const uint32_t brick = (blockIdx.x * MC_BLOCK + threadIdx.x) >> 6;
	if (brick >= n_bricks) return; // (wave-uniform)
	const GridRsrc t_grid = make_grid_rsrc(M.grid, M.grid_bytes), t_xgrid = make_grid_rsrc(M.xgrid, M.xgrid_bytes);
	const uint32_t nbx = (L.res[0] + 3) / 4, nby = (L.res[1] + 3) / 4;
	const uint32_t i = 4 * (brick % nbx) + (lane & 3), j = 4 * ((brick / nbx) % nby) + ((lane >> 2) & 3), k = 4 * (brick / (nbx * nby)) + (lane >> 4);
	const bool valid = i < L.res[0] && j < L.res[1] && k < L.res[2];
	const uint32_t idx = valid ? i + L.res[0] * (j + L.res[1] * k) : 0u;
	const f3 w = mc_warp(M, mc_position(L, (float)(valid ? i : 0), (float)(valid ? j : 0), (float)(valid ? k : 0)));
	for (int p = 0; p < 4; ++p) {
		const int src = 16 * p + c;
		const float sx = __shfl(w.x, src, 64), sy = __shfl(w.y, src, 64), sz = __shfl(w.z, src, 64);
		const uint32_t s_idx = (uint32_t)__shfl((int)idx, src, 64);
		const int s_valid = __shfl(valid ? 1 : 0, src, 64);
		EncodeInFlight e;
		encode_issue(t_grid, t_xgrid, s_lv, lane >> 4, sx, sy, sz, e);
		const half8 enc = encode_finish(e);
		const half_t logit = density_pass<DLIN>(s_w, lane, enc);
		if (lane < 16 && s_valid) out[s_idx] = network_to_density((float)logit, M.density_act);
	}
}

// ---- the lattice, wide models: positions of points [first, first + n), the network, the activated density of its logit
__global__ void mc_lattice_positions_kernel(const ModelParams M, const McLattice L, uint32_t first, uint32_t n, float* __restrict__ pos01) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	const uint32_t p = first + t, i = p % L.res[0], jk = p / L.res[0], j = jk % L.res[1], k = jk / L.res[1];
	const f3 w = mc_warp(M, mc_position(L, (float)i, (float)j, (float)k));
	pos01[3 * t + 0] = w.x; pos01[3 * t + 1] = w.y; pos01[3 * t + 2] = w.z;
}
__global__ void mc_density_from_logits_kernel(uint32_t n, uint32_t density_act, const uint16_t* __restrict__ net, float* __restrict__ out) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	union { uint16_t u; half_t h; } cv;
	cv.u = net[4 * (size_t)t + 3];
	out[t] = network_to_density((float)cv.h, density_act);
}

// ---- marching cubes
__global__ __launch_bounds__(MC_BLOCK) void mc_count_kernel(const McGrid G, uint2* __restrict__ block_counts) {
	__shared__ uint32_t s_v[MC_BLOCK / 64], s_t[MC_BLOCK / 64];
	const uint32_t p0 = (blockIdx.x * MC_BLOCK + threadIdx.x) * MC_PTS;
	McQuad Q;
	mc_load_quad<4>(G, p0, Q);
	uint32_t nv = 0, nt = 0;
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		nv += __popc(mc_vmask(G, Q, q, p0));
		const int c = mc_case(G, Q, q, p0);
		nt += c >= 0 ? MC_TABLE.n[c] : 0u;
	}
	// block totals: wave sums, then the four waves
	for (int o = 32; o > 0; o >>= 1) {
		nv += __shfl_xor(nv, o, 64);
		nt += __shfl_xor(nt, o, 64);
	}
	if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = nv; s_t[threadIdx.x >> 6] = nt; }
	__syncthreads();
	if (threadIdx.x == 0) {
		uint2 r = make_uint2(0, 0);
		for (int w = 0; w < MC_BLOCK / 64; ++w) { r.x += s_v[w]; r.y += s_t[w]; }
		block_counts[blockIdx.x] = r;
	}
}

// one workgroup of 1024 threads: block_counts -> exclusive offsets in place, totals[0..1] = vertices, triangles (64-bit: the host refuses
// a mesh whose 32-bit indices would wrap before anything is emitted)
__global__ __launch_bounds__(1024) void mc_scan_kernel(uint32_t n_blocks, uint2* __restrict__ counts, unsigned long long* __restrict__ totals) {
	__shared__ unsigned long long s_v[16], s_t[16];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned long long run_v = 0, run_t = 0;
	for (uint32_t base = 0; base < n_blocks; base += 1024) {
		const uint32_t b = base + threadIdx.x;
		const uint2 c = b < n_blocks ? counts[b] : make_uint2(0, 0);
		unsigned long long iv = c.x, it = c.y; // inclusive scan inside the wave
		for (int o = 1; o < 64; o <<= 1) {
			const unsigned long long uv = __shfl_up(iv, o, 64), ut = __shfl_up(it, o, 64);
			if (lane >= o) { iv += uv; it += ut; }
		}
		if (lane == 63) { s_v[wave] = iv; s_t[wave] = it; }
		__syncthreads();
		unsigned long long bv = run_v, bt = run_t, sv = 0, st = 0;
		for (int w = 0; w < 16; ++w) {
			if (w < wave) { bv += s_v[w]; bt += s_t[w]; }
			sv += s_v[w]; st += s_t[w];
		}
		if (b < n_blocks) counts[b] = make_uint2((uint32_t)(bv + iv - c.x), (uint32_t)(bt + it - c.y));
		run_v += sv; run_t += st;
		__syncthreads();
	}
	if (threadIdx.x == 0) { totals[0] = run_v; totals[1] = run_t; }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_emit_vertices_kernel(const McGrid G, const McLattice L, const uint2* __restrict__ block_offsets,
                                                                    uint32_t* __restrict__ vofs, uint32_t* __restrict__ vmask4, float* __restrict__ V) {
	__shared__ uint32_t s_wave[MC_BLOCK / 64];
	const uint32_t p0 = (blockIdx.x * MC_BLOCK + threadIdx.x) * MC_PTS;
	McQuad Q;
	mc_load_quad<3>(G, p0, Q);
	uint32_t m[4], nv = 0;
#pragma unroll
	for (int q = 0; q < 4; ++q) { m[q] = mc_vmask(G, Q, q, p0); nv += __popc(m[q]); }
	uint32_t total;
	uint32_t o = block_offsets[blockIdx.x].x + mc_block_prefix<4>(nv, s_wave, total);
	if (p0 >= G.n) return;
	uint4 ofs;
	uint32_t* po = &ofs.x;
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		po[q] = o;
		const float d0 = Q.v0[q];
#pragma unroll
		for (int a = 0; a < 3; ++a) {
			if (!((m[q] >> a) & 1u)) continue;
			const float d1 = a == 0 ? Q.v0[q + 1] : (a == 1 ? Q.vy[q] : Q.vz[q]);
			const float t = (G.thresh - d0) / (d1 - d0);
			const f3 p = mc_position(L, (float)Q.i[q] + (a == 0 ? t : 0.0f), (float)Q.j[q] + (a == 1 ? t : 0.0f), (float)Q.k[q] + (a == 2 ? t : 0.0f));
			V[3 * (size_t)o + 0] = p.x; V[3 * (size_t)o + 1] = p.y; V[3 * (size_t)o + 2] = p.z;
			++o;
		}
	}
	// (both arrays are padded to a multiple of 4 points)
	*reinterpret_cast<uint4*>(vofs + p0) = ofs;
	vmask4[p0 / 4] = m[0] | m[1] << 8 | m[2] << 16 | m[3] << 24;
}

__global__ __launch_bounds__(MC_BLOCK) void mc_emit_triangles_kernel(const McGrid G, const uint2* __restrict__ block_offsets, const uint32_t* __restrict__ vofs,
                                                                     const uint8_t* __restrict__ vmask, uint32_t* __restrict__ F) {
	__shared__ uint32_t s_wave[MC_BLOCK / 64];
	const uint32_t p0 = (blockIdx.x * MC_BLOCK + threadIdx.x) * MC_PTS;
	McQuad Q;
	mc_load_quad<4>(G, p0, Q);
	int cs[4];
	uint32_t nt = 0;
#pragma unroll
	for (int q = 0; q < 4; ++q) { cs[q] = mc_case(G, Q, q, p0); nt += cs[q] >= 0 ? MC_TABLE.n[cs[q]] : 0u; }
	uint32_t total;
	uint32_t o = block_offsets[blockIdx.x].y + mc_block_prefix<5>(nt, s_wave, total);
	const uint32_t sxy = G.rx * G.ry;
	for (int q = 0; q < 4; ++q) {
		if (cs[q] < 0) continue;
		const uint32_t p = p0 + q, n = MC_TABLE.n[cs[q]];
		for (uint32_t e = 0; e < 3 * n; ++e) {
			const uint32_t id = MC_TABLE.e[cs[q]][e], a = id >> 2, u = id & 1u, v = (id >> 1) & 1u;
			// edge 4a + u + 2v: along axis a from the corner whose other two coordinates, in axis order, are (u, v)
			const uint32_t owner = p + (a == 0 ? u * G.rx + v * sxy : (a == 1 ? u + v * sxy : u + v * G.rx));
			F[3 * (size_t)o + e] = vofs[owner] + (uint32_t)__popc(vmask[owner] & ((1u << a) - 1u));
		}
		o += n;
	}
}

// ---- normals and colours at the vertices: inputs of the density-gradient / network stages, then their outputs in the mesh's terms
__global__ void mc_vertex_inputs_kernel(const ModelParams M, uint32_t n, const float* __restrict__ V, float* __restrict__ pos01, float* __restrict__ dir01) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	const f3 p = mk3(V[3 * t], V[3 * t + 1], V[3 * t + 2]);
	const f3 w = mc_warp(M, p);
	pos01[3 * t] = w.x; pos01[3 * t + 1] = w.y; pos01[3 * t + 2] = w.z;
	// generate_nerf_network_inputs_from_positions: the direction from the centre of the unit cube outward, (d + 1) / 2 as the network takes it
	const float dx = p.x - 0.5f, dy = p.y - 0.5f, dz = p.z - 0.5f, len = sqrtf(dx * dx + dy * dy + dz * dz);
	const float il = len > 0.0f ? 1.0f / len : 0.0f;
	dir01[3 * t] = dx * il * 0.5f + 0.5f; dir01[3 * t + 1] = dy * il * 0.5f + 0.5f; dir01[3 * t + 2] = dz * il * 0.5f + 0.5f;
}
__global__ void mc_vertex_attributes_kernel(const ModelParams M, uint32_t n, const float* __restrict__ grad01, const uint16_t* __restrict__ net, float* __restrict__ N,
                                            float* __restrict__ C) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	density_normal(M, grad01 + 3 * t, N + 3 * t); // (render_common.h: the rule the frames' surface-normal pass shares)
	union { uint16_t u; half_t h; } cv;
	for (int c = 0; c < 3; ++c) {
		cv.u = net[4 * (size_t)t + c];
		C[3 * t + c] = 1.0f / (1.0f + expf(-(float)cv.h));
	}
}

// ---- launchers
void launch_mc_density(const ModelParams& M, const McLattice& L, float* d_out, float* d_scratch_pos, uint16_t* d_scratch_net, uint32_t chunk, int n_cus, hipStream_t stream) {
	const uint32_t n = L.res[0] * L.res[1] * L.res[2];
	if (!M.wide.width) {
		const uint32_t n_bricks = ((L.res[0] + 3) / 4) * ((L.res[1] + 3) / 4) * ((L.res[2] + 3) / 4);
		const dim3 grid((n_bricks + MC_BLOCK / 64 - 1) / (MC_BLOCK / 64));
		if (M.density_linear) hipLaunchKernelGGL(mc_density_grid_kernel<true>, grid, dim3(MC_BLOCK), 0, stream, M, L, n_bricks, d_out);
		else hipLaunchKernelGGL(mc_density_grid_kernel<false>, grid, dim3(MC_BLOCK), 0, stream, M, L, n_bricks, d_out);
		return;
	}
	for (uint32_t first = 0; first < n; first += chunk) { // the wide network on chunks of the lattice (its rgb head runs along)
		const uint32_t m = n - first < chunk ? n - first : chunk;
		hipLaunchKernelGGL(mc_lattice_positions_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, M, L, first, m, d_scratch_pos);
		launch_network_inference_wide(M, m, d_scratch_pos, d_scratch_pos, d_scratch_net, n_cus, stream);
		hipLaunchKernelGGL(mc_density_from_logits_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, m, M.density_act, d_scratch_net, d_out + first);
	}
}
uint32_t mc_n_blocks(uint32_t n_points) { return (n_points + MC_BLOCK_PTS - 1) / MC_BLOCK_PTS; }
void launch_mc_count_scan(const McGrid& G, uint2* d_blocks, unsigned long long* d_totals, hipStream_t stream) {
	const uint32_t nb = mc_n_blocks(G.n);
	hipLaunchKernelGGL(mc_count_kernel, dim3(nb), dim3(MC_BLOCK), 0, stream, G, d_blocks);
	hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(1024), 0, stream, nb, d_blocks, d_totals);
}
void launch_mc_emit(const McGrid& G, const McLattice& L, const uint2* d_blocks, uint32_t* d_vofs, uint32_t* d_vmask, float* d_V, uint32_t* d_F, hipStream_t stream) {
	const uint32_t nb = mc_n_blocks(G.n);
	hipLaunchKernelGGL(mc_emit_vertices_kernel, dim3(nb), dim3(MC_BLOCK), 0, stream, G, L, d_blocks, d_vofs, d_vmask, d_V);
	hipLaunchKernelGGL(mc_emit_triangles_kernel, dim3(nb), dim3(MC_BLOCK), 0, stream, G, d_blocks, d_vofs, (const uint8_t*)d_vmask, d_F);
}
void launch_mc_vertex_inputs(const ModelParams& M, uint32_t n, const float* d_V, float* d_pos01, float* d_dir01, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(mc_vertex_inputs_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, M, n, d_V, d_pos01, d_dir01);
}
void launch_mc_vertex_attributes(const ModelParams& M, uint32_t n, const float* d_grad, const uint16_t* d_net, float* d_N, float* d_C, hipStream_t stream) {
	if (n) hipLaunchKernelGGL(mc_vertex_attributes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, M, n, d_grad, d_net, d_N, d_C);
}

} // namespace ngp
