// Marching-cubes mesh extraction (Testbed::compute_marching_cubes_mesh / compute_and_save_marching_cubes_mesh): the C ABI over
// mc_kernels.hip. Contract: include/ngp_hip.h.
#include "ngp_host.h"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace ngp;

namespace {

// device buffers of one call; never empty, so that an empty mesh still passes valid pointers
template <class T> DevArray<T> scratch(size_t n) { return DevArray<T>(n ? n : 1); }

constexpr const char* NEEDS = "marching cubes runs on the GPU";

McLattice make_lattice(const ngp_ctx* ctx, const uint32_t* res3, const float* aabb6) {
	if (!res3) throw std::runtime_error("null argument");
	uint64_t n = 1;
	for (int a = 0; a < 3; ++a) {
		if (res3[a] < 2 || res3[a] > 1024) throw std::runtime_error("marching cubes: every resolution must lie in [2, 1024]");
		n *= res3[a];
	}
	if (n > (1ull << 30)) throw std::runtime_error("marching cubes: the lattice may hold at most 2^30 points");
	McLattice L{};
	for (int a = 0; a < 3; ++a) {
		const float lo = aabb6 ? aabb6[a] : ctx->M.raabb_min[a], hi = aabb6 ? aabb6[3 + a] : ctx->M.raabb_max[a];
		if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) throw std::runtime_error("marching cubes: the aabb must be finite and not empty (max > min on every axis)");
		L.res[a] = res3[a];
		L.lo[a] = lo;
		L.ext[a] = hi - lo;
		L.rm1[a] = (float)(res3[a] - 1);
	}
	memcpy(L.r2l, ctx->M.r2l, sizeof(L.r2l));
	return L;
}

void check_thresh(float thresh) {
	if (!std::isfinite(thresh)) throw std::runtime_error("marching cubes: thresh must be finite");
}

uint32_t n_points(const McLattice& L) { return L.res[0] * L.res[1] * L.res[2]; }
size_t padded(uint32_t n) { return ((size_t)n + 3) & ~(size_t)3; }

// the activated density on the lattice into d_out (padded with zeros to a multiple of 4 values)
void density_on_grid(ngp_ctx* ctx, const McLattice& L, float* d_out) {
	const uint32_t n = n_points(L);
	NGP_HIP_CHECK(hipMemsetAsync(d_out, 0, padded(n) * sizeof(float), ctx->stream));
	if (!ctx->M.wide.width) {
		launch_mc_density(ctx->M, L, d_out, nullptr, nullptr, 0, ctx->n_cus, ctx->stream);
	} else {
		const uint32_t chunk = std::min<uint32_t>(n, 1u << 22);
		auto pos = scratch<float>((size_t)chunk * 3);
		auto net = scratch<uint16_t>((size_t)chunk * 4);
		launch_mc_density(ctx->M, L, d_out, pos.get(), net.get(), chunk, ctx->n_cus, ctx->stream);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (the scratch goes out of scope)
	}
	NGP_HIP_CHECK(hipGetLastError());
}

// marching cubes on the lattice at d_density into device buffers of the vertices and triangles (the two totals that size them are read back
// in between); after_emit (nullable) is recorded behind the emit kernels
struct DevMesh {
	uint32_t nv = 0, nt = 0;
	DevArray<float> V;
	DevArray<uint32_t> F;
};
DevMesh marching_cubes(ngp_ctx* ctx, const McLattice& L, const float* d_density, float thresh, hipEvent_t after_emit = nullptr) {
	const uint32_t n = n_points(L);
	const McGrid G{d_density, L.res[0], L.res[1], L.res[2], n, thresh};
	const uint32_t nb = mc_n_blocks(n);
	auto blocks = scratch<uint2>(nb);
	auto totals = scratch<unsigned long long>(2);
	launch_mc_count_scan(G, blocks.get(), totals.get(), ctx->stream);
	unsigned long long tot[2] = {0, 0};
	NGP_HIP_CHECK(hipMemcpyAsync(tot, totals.get(), sizeof(tot), hipMemcpyDeviceToHost, ctx->stream));
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	if (tot[0] > 0xffffffffull || tot[1] > 0xffffffffull / 3) throw std::runtime_error("marching cubes: the mesh would exceed 32-bit indices; lower the resolution");
	DevMesh m;
	m.nv = (uint32_t)tot[0];
	m.nt = (uint32_t)tot[1];
	auto vofs = scratch<uint32_t>(padded(n));
	auto vmask = scratch<uint32_t>(padded(n) / 4);
	m.V = scratch<float>((size_t)m.nv * 3);
	m.F = scratch<uint32_t>((size_t)m.nt * 3);
	launch_mc_emit(G, L, blocks.get(), vofs.get(), vmask.get(), m.V.get(), m.F.get(), ctx->stream);
	NGP_HIP_CHECK(hipGetLastError());
	if (after_emit) NGP_HIP_CHECK(hipEventRecord(after_emit, ctx->stream));
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (vofs / vmask go out of scope)
	return m;
}

void read_back(ngp_ctx* ctx, const DevMesh& m) {
	ctx->mc_V.resize((size_t)m.nv * 3);
	ctx->mc_F.resize((size_t)m.nt * 3);
	NGP_HIP_CHECK(hipMemcpyAsync(ctx->mc_V.data(), m.V.get(), ctx->mc_V.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
	NGP_HIP_CHECK(hipMemcpyAsync(ctx->mc_F.data(), m.F.get(), ctx->mc_F.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void clear_mesh(ngp_ctx* ctx) {
	ctx->mc_valid = ctx->mc_attrs = false;
	ctx->mc_V.clear(); ctx->mc_N.clear(); ctx->mc_C.clear(); ctx->mc_F.clear();
}

bool ends_with_ci(const std::string& s, const char* suf) {
	const size_t n = strlen(suf);
	if (s.size() < n) return false;
	for (size_t i = 0; i < n; ++i) if (tolower((unsigned char)s[s.size() - n + i]) != tolower((unsigned char)suf[i])) return false;
	return true;
}

} // namespace

extern "C" {

int ngp_density_on_grid(ngp_ctx* ctx, const uint32_t* res3, const float* aabb6, float* out) {
	return guarded(ctx, [&] {
		require_model(ctx, NEEDS);
		const McLattice L = make_lattice(ctx, res3, aabb6);
		if (!out) throw std::runtime_error("null argument");
		ngp::sync_inference_model(ctx);
		const uint32_t n = n_points(L);
		auto d = scratch<float>(padded(n));
		density_on_grid(ctx, L, d.get());
		NGP_HIP_CHECK(hipMemcpyAsync(out, d.get(), (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	});
}

int ngp_marching_cubes(ngp_ctx* ctx, const uint32_t* res3, const float* aabb6, float thresh, const float* density, uint32_t* n_verts, uint32_t* n_tris) {
	return guarded(ctx, [&] {
		require_model(ctx, NEEDS);
		const McLattice L = make_lattice(ctx, res3, aabb6);
		check_thresh(thresh);
		if (!density) throw std::runtime_error("null argument");
		clear_mesh(ctx);
		const uint32_t n = n_points(L);
		auto d = scratch<float>(padded(n));
		NGP_HIP_CHECK(hipMemsetAsync(d.get(), 0, d.bytes(), ctx->stream));
		NGP_HIP_CHECK(hipMemcpyAsync(d.get(), density, (size_t)n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
		read_back(ctx, marching_cubes(ctx, L, d.get(), thresh));
		ctx->mc_valid = true;
		if (n_verts) *n_verts = (uint32_t)(ctx->mc_V.size() / 3);
		if (n_tris) *n_tris = (uint32_t)(ctx->mc_F.size() / 3);
	});
}

int ngp_compute_marching_cubes_mesh(ngp_ctx* ctx, const uint32_t* res3, const float* aabb6, float thresh, uint32_t* n_verts, uint32_t* n_tris) {
	return guarded(ctx, [&] {
		require_model(ctx, NEEDS);
		const McLattice L = make_lattice(ctx, res3, aabb6);
		check_thresh(thresh);
		if (ctx->M.wide.width && (!ctx->M.wide.layers_t[0].n_mtiles || ctx->M.wide.enc_dims > ctx->M.wide.width))
			throw std::runtime_error("the normals of a Frequency / Identity-encoding model's mesh need the density gradient: implemented for up to 8 hidden density layers and an encoding no wider than the network");
		clear_mesh(ctx);
		ngp::sync_inference_model(ctx);
		const uint32_t n = n_points(L);
		const Event ev[4] = {new_event(), new_event(), new_event(), new_event()};
		auto d = scratch<float>(padded(n));
		NGP_HIP_CHECK(hipEventRecord(ev[0], ctx->stream));
		density_on_grid(ctx, L, d.get());
		NGP_HIP_CHECK(hipEventRecord(ev[1], ctx->stream));
		const DevMesh mesh = marching_cubes(ctx, L, d.get(), thresh, ev[2]);
		const uint32_t nv = mesh.nv;
		auto pos = scratch<float>((size_t)nv * 3), dir = scratch<float>((size_t)nv * 3), grad = scratch<float>((size_t)nv * 3);
		auto net = scratch<uint16_t>((size_t)nv * 4);
		auto N = scratch<float>((size_t)nv * 3), C = scratch<float>((size_t)nv * 3);
		if (nv) {
			launch_mc_vertex_inputs(ctx->M, nv, mesh.V.get(), pos.get(), dir.get(), ctx->stream);
			if (ctx->M.wide.width) {
				launch_density_gradient_wide(ctx->M, nv, pos.get(), grad.get(), ctx->n_cus, ctx->stream);
				launch_network_inference_wide(ctx->M, nv, pos.get(), dir.get(), net.get(), ctx->n_cus, ctx->stream);
			} else {
				launch_density_gradient(ctx->M, nv, pos.get(), grad.get(), ctx->stream);
				launch_network_inference(ctx->M, nv, pos.get(), dir.get(), net.get(), ctx->stream);
			}
			launch_mc_vertex_attributes(ctx->M, nv, grad.get(), net.get(), N.get(), C.get(), ctx->stream);
			NGP_HIP_CHECK(hipGetLastError());
		}
		NGP_HIP_CHECK(hipEventRecord(ev[3], ctx->stream));
		read_back(ctx, mesh);
		ctx->mc_N.resize((size_t)nv * 3);
		ctx->mc_C.resize((size_t)nv * 3);
		NGP_HIP_CHECK(hipMemcpyAsync(ctx->mc_N.data(), N.get(), ctx->mc_N.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
		NGP_HIP_CHECK(hipMemcpyAsync(ctx->mc_C.data(), C.get(), ctx->mc_C.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		// lattice; marching cubes (count, scan, the read-back of the two totals, emit); normals + colours. The host copies of the mesh follow.
		for (int s = 0; s < 3; ++s) NGP_HIP_CHECK(hipEventElapsedTime(&ctx->mc_ms[s], ev[s], ev[s + 1]));
		ctx->mc_valid = ctx->mc_attrs = true;
		if (n_verts) *n_verts = nv;
		if (n_tris) *n_tris = (uint32_t)(ctx->mc_F.size() / 3);
	});
}

int ngp_get_marching_cubes_mesh(ngp_ctx* ctx, float* V, float* N, float* C, uint32_t* F) {
	return guarded(ctx, [&] {
		require_device(ctx, NEEDS);
		if (!ctx->mc_valid) throw std::runtime_error("no marching-cubes mesh has been computed");
		if ((N || C) && !ctx->mc_attrs) throw std::runtime_error("a mesh of a caller's lattice (ngp_marching_cubes) has no normals or colours");
		if (V) memcpy(V, ctx->mc_V.data(), ctx->mc_V.size() * sizeof(float));
		if (N) memcpy(N, ctx->mc_N.data(), ctx->mc_N.size() * sizeof(float));
		if (C) memcpy(C, ctx->mc_C.data(), ctx->mc_C.size() * sizeof(float));
		if (F) memcpy(F, ctx->mc_F.data(), ctx->mc_F.size() * sizeof(uint32_t));
	});
}

int ngp_get_marching_cubes_timings(ngp_ctx* ctx, float* ms3) {
	return guarded(ctx, [&] {
		require_device(ctx, NEEDS);
		if (!ms3) throw std::runtime_error("null argument");
		memcpy(ms3, ctx->mc_ms, sizeof(ctx->mc_ms));
	});
}

int ngp_save_marching_cubes_mesh(ngp_ctx* ctx, const char* path) {
	return guarded(ctx, [&] {
		require_device(ctx, NEEDS);
		if (!path) throw std::runtime_error("null argument");
		const std::string p(path);
		const bool obj = ends_with_ci(p, ".obj"), ply = ends_with_ci(p, ".ply");
		if (!obj && !ply) throw std::runtime_error("marching cubes: the mesh file must end in .obj or .ply");
		if (!ctx->mc_valid) throw std::runtime_error("no marching-cubes mesh has been computed");
		const size_t nv = ctx->mc_V.size() / 3, nt = ctx->mc_F.size() / 3;
		const bool attrs = ctx->mc_attrs;
		const float scale = ctx->dataset.scale;
		const float* off = ctx->dataset.offset;
		FILE* f = fopen(path, "w");
		if (!f) throw std::runtime_error("cannot write " + p);
		auto pos = [&](size_t i, int a) { return (ctx->mc_V[3 * i + a] - off[a]) / scale; };
		auto u8 = [&](size_t i, int a) {
			const float c = ctx->mc_C[3 * i + a];
			return (int)std::lround((c < 0.f ? 0.f : (c > 1.f ? 1.f : c)) * 255.f);
		};
		if (obj) {
			for (size_t i = 0; i < nv; ++i) {
				if (attrs) fprintf(f, "v %.9g %.9g %.9g %.3f %.3f %.3f\n", pos(i, 0), pos(i, 1), pos(i, 2), ctx->mc_C[3 * i], ctx->mc_C[3 * i + 1], ctx->mc_C[3 * i + 2]);
				else fprintf(f, "v %.9g %.9g %.9g\n", pos(i, 0), pos(i, 1), pos(i, 2));
			}
			if (attrs)
				for (size_t i = 0; i < nv; ++i) fprintf(f, "vn %.9g %.9g %.9g\n", ctx->mc_N[3 * i], ctx->mc_N[3 * i + 1], ctx->mc_N[3 * i + 2]);
			for (size_t t = 0; t < nt; ++t) {
				const uint32_t a = ctx->mc_F[3 * t] + 1, b = ctx->mc_F[3 * t + 1] + 1, c = ctx->mc_F[3 * t + 2] + 1;
				if (attrs) fprintf(f, "f %u//%u %u//%u %u//%u\n", a, a, b, b, c, c);
				else fprintf(f, "f %u %u %u\n", a, b, c);
			}
		} else {
			fprintf(f, "ply\nformat ascii 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n", nv);
			if (attrs) fprintf(f, "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n");
			fprintf(f, "element face %zu\nproperty list uchar int vertex_index\nend_header\n", nt);
			for (size_t i = 0; i < nv; ++i) {
				if (attrs)
					fprintf(f, "%.9g %.9g %.9g %.9g %.9g %.9g %d %d %d\n", pos(i, 0), pos(i, 1), pos(i, 2), ctx->mc_N[3 * i], ctx->mc_N[3 * i + 1], ctx->mc_N[3 * i + 2],
					        u8(i, 0), u8(i, 1), u8(i, 2));
				else fprintf(f, "%.9g %.9g %.9g\n", pos(i, 0), pos(i, 1), pos(i, 2));
			}
			for (size_t t = 0; t < nt; ++t) fprintf(f, "3 %u %u %u\n", ctx->mc_F[3 * t], ctx->mc_F[3 * t + 1], ctx->mc_F[3 * t + 2]);
		}
		const bool ok = ferror(f) == 0;
		if (fclose(f) != 0 || !ok) throw std::runtime_error("writing " + p + " failed");
	});
}

} // extern "C"
