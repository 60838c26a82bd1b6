// Geometry mode, host side of the C ABI: Testbed::load_scene / load_mesh (reference
// src/testbed_geometry_training.cu:2751-2866, 3101-3210), the BVH4 build (src/triangle_bvh.cu:425-508) and the
// .obj reader that replaces the vendored tinyobjloader wrapper (src/tinyobj_loader_wrapper.cu).
#include "ngp_host.h"
#include "bvh4_build.h"
#include "sh9.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

using namespace ngp;

namespace {

using namespace ngp::bvh4; // V3 and its helpers, bounds, build_bvh4

// after any change of the mesh list: scene AABB (load_scene :3183-3189) and the device-side MeshRef table
void rebuild_scene(ngp_ctx* ctx) {
	++ctx->mesh_generation;
	ctx->d_meshrefs.reset();
	ctx->mesh_scene = MeshSceneParams{};
	if (ctx->meshes.empty()) return;
	V3 lo = ld(ctx->meshes[0].bmin), hi = ld(ctx->meshes[0].bmax);
	for (auto& m : ctx->meshes) {
		lo = vmin(lo, ld(m.bmin));
		hi = vmax(hi, ld(m.bmax));
	}
	st(ctx->mesh_scene.scene_min, {lo.x - 4.0f, lo.y - 4.0f, lo.z - 4.0f});
	st(ctx->mesh_scene.scene_max, {hi.x + 4.0f, hi.y + 4.0f, hi.z + 4.0f});
	ctx->mesh_scene.n_meshes = (uint32_t)ctx->meshes.size();
	if (ctx->device < 0) return;
	std::vector<MeshRef> refs(ctx->meshes.size());
	for (size_t i = 0; i < refs.size(); ++i) {
		HostMesh& m = ctx->meshes[i];
		if (!m.d_tris) {
			m.d_tris.upload(m.tris.data(), m.tris.size());
			m.d_nodes.upload(m.nodes.data(), m.nodes.size());
		}
		refs[i].nodes = m.d_nodes.get();
		refs[i].tris = m.d_tris.get();
		memcpy(refs[i].bmin, m.bmin, sizeof(m.bmin));
		memcpy(refs[i].bmax, m.bmax, sizeof(m.bmax));
		refs[i].n_tris = (uint32_t)m.d_tris.size();
		refs[i].n_nodes = (uint32_t)m.d_nodes.size();
	}
	ctx->d_meshrefs.upload(refs.data(), refs.size());
	ctx->mesh_scene.meshes = ctx->d_meshrefs.get();
}

// Testbed::load_mesh (:2786-2866): normalise into the unit cube around `center`, build the BVH
void add_mesh_impl(ngp_ctx* ctx, const float* vertices, uint32_t n_tris, const float* center3) {
	if (!vertices || n_tris == 0) throw std::runtime_error("mesh has no triangles");
	const size_t n_vertices = (size_t)n_tris * 3;
	const float inf = std::numeric_limits<float>::infinity();
	V3 lo{inf, inf, inf}, hi{-inf, -inf, -inf};
	for (size_t i = 0; i < n_vertices; ++i) {
		lo = vmin(lo, ld(vertices + 3 * i));
		hi = vmax(hi, ld(vertices + 3 * i));
	}
	const float inflation = 0.005f;
	V3 d0 = hi - lo;
	float amount = std::sqrt((d0.x * d0.x + d0.y * d0.y) + d0.z * d0.z) * inflation;
	lo = {lo.x - amount, lo.y - amount, lo.z - amount};
	hi = {hi.x + amount, hi.y + amount, hi.z + amount};
	V3 diag = hi - lo;
	float mesh_scale = std::max(std::max(diag.x, diag.y), diag.z);
	V3 center = center3 ? ld(center3) : V3{0.f, 0.f, 0.f};
	HostMesh mesh;
	mesh.tris.resize(n_tris);
	st(mesh.center, center);
	for (size_t i = 0; i < n_vertices; ++i) {
		V3 p = ld(vertices + 3 * i);
		V3 q = (p - lo - V3{diag.x * 0.5f, diag.y * 0.5f, diag.z * 0.5f}) / mesh_scale;
		q = {q.x + 0.5f, q.y + 0.5f, q.z + 0.5f};
		q = q + center;
		Triangle& t = mesh.tris[i / 3];
		st(i % 3 == 0 ? t.a : (i % 3 == 1 ? t.b : t.c), q);
	}
	build_bvh4(mesh.tris, 8, mesh.nodes);
	bounds(mesh.tris.data(), mesh.tris.data() + mesh.tris.size(), mesh.bmin, mesh.bmax); // BoundingBox(MeshData*), geometry_bvh.cu:14-34
	ctx->meshes.push_back(std::move(mesh));
	rebuild_scene(ctx);
}

// ascii .obj: 'v' and 'f' records; polygons are fan-triangulated (tinyobj triangulate=true), non-triangle faces kept
std::vector<float> load_obj(const std::string& path) {
	std::string text = read_file(path);
	std::vector<float> verts, out;
	size_t pos = 0;
	while (pos < text.size()) {
		size_t eol = text.find('\n', pos);
		if (eol == std::string::npos) eol = text.size();
		const char* p = text.data() + pos;
		const char* end = text.data() + eol;
		while (p < end && (*p == ' ' || *p == '\t')) ++p;
		if (end - p > 2 && p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
			char* q = nullptr;
			p += 2;
			for (int k = 0; k < 3; ++k) {
				verts.push_back(strtof(p, &q));
				p = q;
			}
		} else if (end - p > 2 && p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
			p += 2;
			std::vector<long> idx;
			while (p < end) {
				while (p < end && (*p == ' ' || *p == '\t' || *p == '\r')) ++p;
				if (p >= end) break;
				char* q = nullptr;
				long i = strtol(p, &q, 10);
				if (q == p) break;
				long nv = (long)(verts.size() / 3);
				idx.push_back(i > 0 ? i - 1 : nv + i);
				p = q;
				while (p < end && *p != ' ' && *p != '\t') ++p; // skip /vt/vn
			}
			for (size_t k = 1; k + 1 < idx.size(); ++k) {
				for (long vi : {idx[0], idx[k], idx[k + 1]}) {
					if (vi < 0 || (size_t)vi * 3 + 2 >= verts.size()) throw std::runtime_error("Error loading '" + path + "': face index out of range");
					out.insert(out.end(), verts.begin() + vi * 3, verts.begin() + vi * 3 + 3);
				}
			}
		}
		pos = eol + 1;
	}
	return out;
}

// geometry_load_stl (:2751-2784): binary STL
std::vector<float> load_stl(const std::string& path) {
	std::string data = read_file(path);
	if (data.size() < 84) throw std::runtime_error("Mesh file '" + path + "' too small for STL header");
	uint32_t nfaces;
	memcpy(&nfaces, data.data() + 80, 4);
	if (memcmp(data.data(), "solid", 5) == 0 || nfaces == 0) throw std::runtime_error("ASCII STL file '" + path + "' not supported");
	std::vector<float> out;
	for (uint32_t i = 0; i < nfaces; ++i) {
		size_t off = 84 + (size_t)i * 50;
		if (off + 50 > data.size()) break;
		float v[9];
		memcpy(v, data.data() + off + 12, 36);
		out.insert(out.end(), v, v + 9);
	}
	return out;
}

void load_mesh_file_impl(ngp_ctx* ctx, const std::string& path, const float* center3) {
	std::vector<float> v;
	if (ends_with_ci(path, ".obj")) v = load_obj(path);
	else if (ends_with_ci(path, ".stl")) v = load_stl(path);
	else throw std::runtime_error("mesh data path must be a mesh in ascii .obj or binary .stl format.");
	add_mesh_impl(ctx, v.data(), (uint32_t)(v.size() / 9), center3);
}

} // namespace

extern "C" {

int ngp_clear_meshes(ngp_ctx* ctx) {
	return guarded(ctx, [&] {
		ctx->meshes.clear();
		rebuild_scene(ctx);
	});
}

int ngp_add_mesh(ngp_ctx* ctx, const float* vertices, uint32_t n_tris, const float* center3) {
	return guarded(ctx, [&] { add_mesh_impl(ctx, vertices, n_tris, center3); });
}

int ngp_load_mesh_file(ngp_ctx* ctx, const char* path, const float* center3) {
	return guarded(ctx, [&] {
		if (!path) throw std::runtime_error("null path");
		load_mesh_file_impl(ctx, path, center3);
	});
}

int ngp_load_scene(ngp_ctx* ctx, const char* json_path) {
	return guarded(ctx, [&] {
		if (!json_path) throw std::runtime_error("null path");
		mj::Value json = mj::parse_json(read_file(json_path));
		if (!json.is_object() || json.size() == 0) throw std::runtime_error("Geometry file must contain an array of geometry metadata.");
		const mj::Value& geometries = json.at("geometry");
		const std::string base = parent_dir(json_path);
		ctx->meshes.clear();
		for (const mj::Value& g : geometries.arr) {
			std::string path = g.at("path").str();
			if (!path.empty() && path[0] != '/') path = base + "/" + path;
			const std::string& type = g.at("type").str();
			float center[3];
			for (int i = 0; i < 3; ++i) center[i] = (float)g.at("center").at((size_t)i).num();
			if (type == "Mesh") load_mesh_file_impl(ctx, path, center);
			else if (type == "Nerf") load_snapshot_path(ctx, path);
			else throw std::runtime_error("Geometry type must be either 'Mesh' or 'Nerf'.");
		}
		rebuild_scene(ctx);
	});
}

int ngp_n_meshes(const ngp_ctx* ctx) { return ctx ? (int)ctx->meshes.size() : -1; }

int ngp_get_mesh_info(const ngp_ctx* ctx, int mesh, uint32_t* n_tris, uint32_t* n_nodes, float* aabb6) {
	if (!ctx || ctx->meshes.empty()) return -1;
	if (mesh == -1) {
		if (aabb6) { memcpy(aabb6, ctx->mesh_scene.scene_min, 12); memcpy(aabb6 + 3, ctx->mesh_scene.scene_max, 12); }
		if (n_tris) { *n_tris = 0; for (auto& m : ctx->meshes) *n_tris += (uint32_t)m.tris.size(); }
		if (n_nodes) { *n_nodes = 0; for (auto& m : ctx->meshes) *n_nodes += (uint32_t)m.nodes.size(); }
		return 0;
	}
	if (mesh < 0 || mesh >= (int)ctx->meshes.size()) return -1;
	const HostMesh& m = ctx->meshes[(size_t)mesh];
	if (n_tris) *n_tris = (uint32_t)m.tris.size();
	if (n_nodes) *n_nodes = (uint32_t)m.nodes.size();
	if (aabb6) { memcpy(aabb6, m.bmin, 12); memcpy(aabb6 + 3, m.bmax, 12); }
	return 0;
}

int ngp_get_mesh_bvh(const ngp_ctx* ctx, int mesh, void* nodes_out, void* triangles_out) {
	if (!ctx || mesh < 0 || mesh >= (int)ctx->meshes.size()) return -1;
	const HostMesh& m = ctx->meshes[(size_t)mesh];
	if (nodes_out) memcpy(nodes_out, m.nodes.data(), m.nodes.size() * sizeof(TriangleBvhNode));
	if (triangles_out) memcpy(triangles_out, m.tris.data(), m.tris.size() * sizeof(Triangle));
	return 0;
}

int ngp_set_geometry_opts(ngp_ctx* ctx, const ngp_geometry_opts* o) {
	if (!ctx || !o) return -1;
	static_assert(sizeof(ngp_geometry_opts) == sizeof(MeshShadeParams), "geometry opts layout");
	memcpy(&ctx->shade, o, sizeof(MeshShadeParams));
	return 0;
}

int ngp_trace_mesh_rays(ngp_ctx* ctx, uint32_t n, float* positions, float* directions) {
	return guarded(ctx, [&] {
		require_device(ctx);
		if (ctx->meshes.empty()) throw std::runtime_error("no meshes loaded");
		if (n == 0) return;
		if (!positions || !directions) throw std::runtime_error("null argument");
		DevArray<float> d_p, d_d;
		d_p.upload(positions, (size_t)n * 3);
		d_d.upload(directions, (size_t)n * 3);
		launch_trace_mesh_rays(ctx->mesh_scene, n, d_p.get(), d_d.get(), ctx->stream);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		NGP_HIP_CHECK(hipMemcpy(positions, d_p.get(), d_p.bytes(), hipMemcpyDeviceToHost));
		NGP_HIP_CHECK(hipMemcpy(directions, d_d.get(), d_d.bytes(), hipMemcpyDeviceToHost));
		NGP_HIP_CHECK(hipGetLastError());
	});
}


// ------------------------------------------------------------------------------------------------ irradiance probes
namespace {
// trace the fan(s) described by P in ONE persistent launch, reduce to the probe texture(s), tabulate E(n) at the texel directions
// the models the probe tracer serves: base.json's heads and the Frequency architecture (`what` names the caller's work in the refusal)
void require_probe_model(ngp_ctx* ctx, const char* what) {
	require_model(ctx);
	ngp::sync_inference_model(ctx);
	if (ctx->M.rgb_mid != 1 && !ctx->M.wide.width) throw std::runtime_error(std::string(what) + " are built for the configs/nerf/base.json rgb head (2 hidden layers)");
	ensure_frame_buffers(ctx, 0);
}
// the model as probe rays see it: in Geometry mode load_scene made the inflated mesh box the render box (testbed_geometry_training.cu:3185-3189)
ngp::ModelParams probe_model(const ngp_ctx* ctx) {
	ngp::ModelParams M = ctx->M;
	if (!ctx->meshes.empty()) {
		for (int i = 0; i < 3; ++i) { M.raabb_min[i] = ctx->mesh_scene.scene_min[i]; M.raabb_max[i] = ctx->mesh_scene.scene_max[i]; }
		const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
		memcpy(M.r2l, ident, sizeof(ident));
		M.r2l_identity = 1u;
	}
	return M;
}

void compute_probes(ngp_ctx* ctx, ngp::ProbeParams P, float min_transmittance) {
	using namespace ngp;
	require_probe_model(ctx, "irradiance probes");
	for (int i = 0; i < 3; ++i) P.center[i] = 0.5f * (ctx->M.raabb_max[i] + ctx->M.raabb_min[i]); // render_aabb.center()
	const uint32_t no = P.mode == NGP_PROBE_MULTI_CENTER ? P.n_origin : 1u;
	const uint32_t n_probes = P.mode == 3 ? P.grid_x * P.grid_y : 1u;
	const uint64_t n_rays64 = (uint64_t)P.n_theta * P.n_phi * no * no * n_probes;
	if (n_rays64 > (1ull << 28)) throw std::runtime_error("probe too large");
	P.n_rays = (uint32_t)n_rays64;
	const uint32_t n_texels = P.n_theta * P.n_phi * n_probes;
	DevArray<float4> ray_rgba(P.n_rays);
	P.ray_rgba = ray_rgba.get();
	ctx->d_envmap.reset(), ctx->d_irradiance.reset();
	ctx->d_envmap.reset(n_texels);
	ctx->d_irradiance.reset(n_texels);
	hipStream_t stream = ctx->stream;
	if (ctx->last_stream && ctx->last_stream != stream) NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
	const int slot = (int)(ctx->n_calls % ngp_ctx::HISTORY);
	if (ctx->n_calls >= (uint64_t)ngp_ctx::HISTORY) NGP_HIP_CHECK(hipStreamWaitEvent(stream, ctx->ev_frame1[slot], 0)); // the slot's previous launch (render_frames, ngp_render.cpp)
	FrameParams F{};
	ctx->bind_slot(F, slot);
	F.n_local_tiles = (P.n_rays + 63) / 64;
	F.shard_index = 0;
	F.shard_count = 1;
	F.min_transmittance = min_transmittance > 0.f ? min_transmittance : 0.01f;
	F.linear_colors = ctx->desc.linear_colors;
	memcpy(F.tune, ctx->tune, sizeof(F.tune));
	NGP_HIP_CHECK(hipEventRecord(ctx->ev_frame0[slot], stream));
	NGP_HIP_CHECK(hipMemsetAsync(P.ray_rgba, 0, (size_t)P.n_rays * sizeof(float4), stream));
	NGP_HIP_CHECK(hipEventRecord(ctx->ev_kern0[slot], stream));
	launch_trace_probe(probe_model(ctx), F, P, ctx->n_cus, stream); // (Geometry mode: the shell positions lie inside the mesh box)
	NGP_HIP_CHECK(hipEventRecord(ctx->ev_kern1[slot], stream));
	launch_probe_reduce(P, ctx->d_envmap.get(), stream);
	launch_irradiance(P, ctx->d_envmap.get(), n_texels, nullptr, ctx->d_irradiance.get(), stream);
	NGP_HIP_CHECK(hipEventRecord(ctx->ev_frame1[slot], stream));
	ctx->hist_n_rays[slot] = P.n_rays;
	ctx->hist_mesh_pass[slot] = false;
	ctx->last_stream = stream;
	++ctx->n_calls;
	NGP_HIP_CHECK(hipStreamSynchronize(stream));
	NGP_HIP_CHECK(hipGetLastError());
	P.ray_rgba = nullptr; // (ray_rgba goes out of scope)
	++ctx->probe_generation;
	ctx->env_probe = P;
	ctx->env_n_theta = P.n_theta;
	ctx->env_n_phi = P.n_phi;
}
size_t env_texels(const ngp_ctx* ctx) {
	const ngp::ProbeParams& P = ctx->env_probe;
	return (size_t)P.n_theta * P.n_phi * (P.mode == 3 ? P.grid_x * P.grid_y : 1u);
}
} // namespace

int ngp_compute_envmap(ngp_ctx* ctx, const ngp_probe_desc* d, float* rgba_out) {
	return guarded(ctx, [&] {
		if (!d || d->n_theta == 0 || d->n_phi == 0 || d->mode < 0 || d->mode > 2) throw std::runtime_error("invalid probe descriptor");
		if (d->mode == NGP_PROBE_MULTI_CENTER && d->n_origin == 0) throw std::runtime_error("invalid probe descriptor: n_origin");
		ngp::ProbeParams P{};
		P.mode = d->mode;
		P.n_theta = d->n_theta;
		P.n_phi = d->n_phi;
		P.n_origin = d->mode == NGP_PROBE_MULTI_CENTER ? d->n_origin : 1u;
		for (int i = 0; i < 3; ++i) P.origin[i] = d->origin[i];
		compute_probes(ctx, P, d->min_transmittance);
		if (rgba_out) NGP_HIP_CHECK(hipMemcpy(rgba_out, ctx->d_envmap.get(), env_texels(ctx) * sizeof(float4), hipMemcpyDeviceToHost));
	});
}

int ngp_compute_envmap_grid(ngp_ctx* ctx, const ngp_probe_grid_desc* d, float* rgba_out) {
	return guarded(ctx, [&] {
		if (!d || d->n_theta == 0 || d->n_phi == 0 || d->grid_x == 0 || d->grid_y == 0 || !(d->shell_radius > 0.f)) throw std::runtime_error("invalid probe grid descriptor");
		if ((uint64_t)d->grid_x * d->grid_y > 65536ull) throw std::runtime_error("probe grid too large");
		ngp::ProbeParams P{};
		P.mode = 3;
		P.n_theta = d->n_theta;
		P.n_phi = d->n_phi;
		P.n_origin = 1;
		P.grid_x = d->grid_x;
		P.grid_y = d->grid_y;
		P.shell_radius = d->shell_radius;
		compute_probes(ctx, P, d->min_transmittance);
		if (rgba_out) NGP_HIP_CHECK(hipMemcpy(rgba_out, ctx->d_envmap.get(), env_texels(ctx) * sizeof(float4), hipMemcpyDeviceToHost));
	});
}

int ngp_get_envmap(ngp_ctx* ctx, uint32_t* n_theta, uint32_t* n_phi, float* rgba_out, float* irradiance_rgba_out) {
	return guarded(ctx, [&] {
		if (!ctx->d_envmap) throw std::runtime_error("no probe texture: call ngp_compute_envmap first");
		if (n_theta) *n_theta = ctx->env_n_theta;
		if (n_phi) *n_phi = ctx->env_n_phi;
		const size_t bytes = env_texels(ctx) * sizeof(float4); // a grid returns grid_x * grid_y textures back to back (ngp_get_envmap_grid tells how many)
		if (rgba_out) NGP_HIP_CHECK(hipMemcpy(rgba_out, ctx->d_envmap.get(), bytes, hipMemcpyDeviceToHost));
		if (irradiance_rgba_out) NGP_HIP_CHECK(hipMemcpy(irradiance_rgba_out, ctx->d_irradiance.get(), bytes, hipMemcpyDeviceToHost));
	});
}

int ngp_get_envmap_grid(ngp_ctx* ctx, ngp_probe_grid_desc* desc_out, float* origins_out) {
	return guarded(ctx, [&] {
		if (!ctx->d_envmap || ctx->env_probe.mode != 3) throw std::runtime_error("no probe grid: call ngp_compute_envmap_grid first");
		const ngp::ProbeParams& P = ctx->env_probe;
		if (desc_out) {
			desc_out->grid_x = P.grid_x; desc_out->grid_y = P.grid_y; desc_out->n_theta = P.n_theta; desc_out->n_phi = P.n_phi;
			desc_out->shell_radius = P.shell_radius;
			desc_out->min_transmittance = 0.f;
		}
		if (origins_out) { // shell positions, for callers that place things: the same arithmetic as the kernel's probe_grid_origin
			const float PI = 3.14159265358979323846f;
			for (uint32_t g = 0; g < P.grid_x * P.grid_y; ++g) {
				const uint32_t i = g % P.grid_x, j = g / P.grid_x;
				const float px = ((float)i + 0.5f) / (float)P.grid_x, py = ((float)j + 0.5f) / (float)P.grid_y;
				const float cos_theta = -2.0f * px + 1.0f, phi = 2.0f * PI * (py - 0.5f);
				const float sin_theta = sqrtf(fmaxf(1.0f - cos_theta * cos_theta, 0.0f));
				origins_out[3 * g] = P.center[0] + sin_theta * cosf(phi) * P.shell_radius;
				origins_out[3 * g + 1] = P.center[1] + sin_theta * sinf(phi) * P.shell_radius;
				origins_out[3 * g + 2] = P.center[2] + cos_theta * P.shell_radius;
			}
		}
	});
}

namespace {
void download_rgb(ngp_ctx* ctx, const float4* d_o, uint32_t n, float* rgb_out) {
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	std::vector<float4> tmp(n);
	NGP_HIP_CHECK(hipMemcpy(tmp.data(), d_o, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < n; ++i) { rgb_out[3 * i] = tmp[i].x; rgb_out[3 * i + 1] = tmp[i].y; rgb_out[3 * i + 2] = tmp[i].z; }
}
} // namespace

int ngp_irradiance(ngp_ctx* ctx, uint32_t n, const float* normals, float* rgb_out) {
	return guarded(ctx, [&] {
		if (!ctx->d_envmap) throw std::runtime_error("no probe texture: call ngp_compute_envmap first");
		if (ctx->env_probe.mode == 3) throw std::runtime_error("the probe texture is a grid: use ngp_irradiance_at (position + normal)");
		if (n == 0) return;
		if (!normals || !rgb_out) throw std::runtime_error("null argument");
		DevArray<float> d_n;
		d_n.upload(normals, (size_t)n * 3);
		DevArray<float4> d_o(n);
		launch_irradiance(ctx->env_probe, ctx->d_envmap.get(), n, d_n.get(), d_o.get(), ctx->stream);
		download_rgb(ctx, d_o.get(), n, rgb_out);
		NGP_HIP_CHECK(hipGetLastError());
	});
}

int ngp_irradiance_at(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, float* rgb_out) {
	return guarded(ctx, [&] {
		if (!ctx->d_irradiance) throw std::runtime_error("no probe texture: call ngp_compute_envmap / ngp_compute_envmap_grid first");
		if (n == 0) return;
		if (!positions || !normals || !rgb_out) throw std::runtime_error("null argument");
		DevArray<float> d_p, d_n;
		d_p.upload(positions, (size_t)n * 3);
		d_n.upload(normals, (size_t)n * 3);
		DevArray<float4> d_o(n);
		launch_irradiance_lookup(ngp::irradiance_map_of(ctx), n, d_p.get(), d_n.get(), d_o.get(), ctx->stream);
		download_rgb(ctx, d_o.get(), n, rgb_out);
		NGP_HIP_CHECK(hipGetLastError());
	});
}

} // extern "C"

// ------------------------------------------------------------------------------------------------ traced irradiance
namespace {
// rays per tracer launch: bounds the ray-list workspace (48 B a ray). Every ray is traced on its own, so chunking changes no result.
constexpr uint32_t RAY_CHUNK = 1u << 21;
constexpr uint64_t MAX_TRACED_RAYS = 1ull << 28;

bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
bool nonzero3(const float* p) { return p[0] != 0.0f || p[1] != 0.0f || p[2] != 0.0f; }

// the launches of one call of a ray-list entry: one history slot, reported by ngp_get_render_stats like a probe launch (the chunks'
// counters and device ticks add up; kernel_ms spans the first chunk's trace to the last one's)
class RayListTrace {
public:
	RayListTrace(ngp_ctx* ctx, uint64_t n_rays, float min_transmittance) : ctx_(ctx), n_rays_(n_rays) {
		stream_ = ctx->stream;
		if (ctx->last_stream && ctx->last_stream != stream_) NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		slot_ = (int)(ctx->n_calls % ngp_ctx::HISTORY);
		if (ctx->n_calls >= (uint64_t)ngp_ctx::HISTORY) NGP_HIP_CHECK(hipStreamWaitEvent(stream_, ctx->ev_frame1[slot_], 0));
		ctx->bind_slot(F_, slot_);
		F_.shard_index = 0;
		F_.shard_count = 1;
		F_.min_transmittance = min_transmittance > 0.f ? min_transmittance : 0.01f;
		F_.linear_colors = ctx->desc.linear_colors;
		memcpy(F_.tune, ctx->tune, sizeof(F_.tune));
		M_ = probe_model(ctx);
		NGP_HIP_CHECK(hipEventRecord(ctx->ev_frame0[slot_], stream_));
	}
	const ngp::ModelParams& model() const { return M_; }
	// n rays of P (ray_o, ray_d, ray_t prepared; ray_rgba and ray_depth are cleared here)
	void trace(ngp::ProbeParams P, uint32_t n) {
		P.mode = ngp::PROBE_RAY_LIST;
		P.n_rays = n;
		NGP_HIP_CHECK(hipMemsetAsync(P.ray_rgba, 0, (size_t)n * sizeof(float4), stream_));
		if (P.ray_depth) NGP_HIP_CHECK(hipMemsetAsync(P.ray_depth, 0, (size_t)n * sizeof(float), stream_));
		if (!traced_) NGP_HIP_CHECK(hipEventRecord(ctx_->ev_kern0[slot_], stream_));
		F_.n_local_tiles = (n + 63) / 64;
		F_.add_results = traced_ ? 1 : 0;
		launch_trace_probe(M_, F_, P, ctx_->n_cus, stream_);
		NGP_HIP_CHECK(hipEventRecord(ctx_->ev_kern1[slot_], stream_));
		traced_ = true;
	}
	void finish() {
		if (!traced_) {
			NGP_HIP_CHECK(hipEventRecord(ctx_->ev_kern0[slot_], stream_));
			NGP_HIP_CHECK(hipEventRecord(ctx_->ev_kern1[slot_], stream_));
		}
		NGP_HIP_CHECK(hipEventRecord(ctx_->ev_frame1[slot_], stream_));
		ctx_->hist_n_rays[slot_] = n_rays_;
		ctx_->hist_mesh_pass[slot_] = false;
		ctx_->last_stream = stream_;
		++ctx_->n_calls;
		NGP_HIP_CHECK(hipStreamSynchronize(stream_));
		NGP_HIP_CHECK(hipGetLastError());
	}

private:
	ngp_ctx* ctx_;
	uint64_t n_rays_;
	hipStream_t stream_;
	int slot_ = 0;
	bool traced_ = false;
	ngp::FrameParams F_{};
	ngp::ModelParams M_{};
};

void download(ngp_ctx* ctx, void* dst, const void* src, size_t bytes) {
	NGP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}
void upload(ngp_ctx* ctx, void* dst, const void* src, size_t bytes) {
	NGP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
}

// the points' checks shared by ngp_irradiance_rays and ngp_irradiance_traced; returns K
uint32_t check_irradiance_request(uint32_t n, const float* positions, const float* normals, const ngp_irradiance_trace_desc* d) {
	if (!d) throw std::runtime_error("null argument");
	if (d->n_u == 0 || d->n_v == 0) throw std::runtime_error("invalid irradiance descriptor: n_u and n_v must be at least 1");
	if (!std::isfinite(d->offset) || d->offset < 0.0f) throw std::runtime_error("invalid irradiance descriptor: offset must be finite and >= 0");
	const uint64_t K = (uint64_t)d->n_u * d->n_v;
	if (K * n > MAX_TRACED_RAYS) throw std::runtime_error("irradiance request too large: n * n_u * n_v > 2^28 rays");
	if (n && (!positions || !normals)) throw std::runtime_error("null argument");
	for (uint32_t i = 0; i < n; ++i) {
		if (!finite3(positions + 3 * (size_t)i)) throw std::runtime_error("position " + std::to_string(i) + " is not finite");
		if (!finite3(normals + 3 * (size_t)i) || !nonzero3(normals + 3 * (size_t)i)) throw std::runtime_error("normal " + std::to_string(i) + " is zero or not finite");
	}
	return (uint32_t)K;
}

// the chunks of an irradiance request: whole points while K <= RAY_CHUNK, else RAY_CHUNK-ray pieces of one point. f(r0, n_rays).
template <typename F>
void for_each_irradiance_chunk(uint32_t n, uint32_t K, F&& f) {
	if (K <= RAY_CHUNK) {
		const uint32_t per = RAY_CHUNK / K;
		for (uint32_t p = 0; p < n; p += per) f((uint64_t)p * K, (std::min(per, n - p)) * K);
	} else {
		for (uint32_t p = 0; p < n; ++p)
			for (uint32_t k = 0; k < K; k += RAY_CHUNK) f((uint64_t)p * K + k, std::min(RAY_CHUNK, K - k));
	}
}

// the generator for rays [r0, r0 + m) of the request into o, d, t (the chunk's points are uploaded from the host arrays first)
void generate_irradiance_rays(ngp_ctx* ctx, const ngp_irradiance_trace_desc* d, uint32_t K, const float* positions, const float* normals, uint64_t r0, uint32_t m,
                              DevArray<float>& pts, float* o, float* dir, float2* t) {
	const uint64_t p0 = r0 / K, p1 = (r0 + m - 1) / K + 1;
	upload(ctx, pts.get(), positions + 3 * p0, (size_t)(p1 - p0) * 3 * sizeof(float));
	upload(ctx, pts.get() + pts.size() / 2, normals + 3 * p0, (size_t)(p1 - p0) * 3 * sizeof(float));
	ngp::launch_irradiance_rays(ctx->mesh_scene, d->occlude_by_meshes != 0, d->n_u, d->n_v, d->offset, r0, m, pts.get(), pts.get() + pts.size() / 2, o, dir, t,
	                            ctx->stream);
}

// ---- SH9 irradiance volumes (contract: include/ngp_hip.h)
constexpr uint32_t SH_FLOAT4 = 7; // a record: 28 floats

// the descriptor's checks shared by the SH entries, for n probes; returns K
uint32_t check_sh_desc(uint64_t n, const ngp_irradiance_sh_desc* d) {
	if (!d) throw std::runtime_error("null argument");
	if (d->n_u == 0 || d->n_v == 0) throw std::runtime_error("invalid irradiance descriptor: n_u and n_v must be at least 1");
	const uint64_t K = (uint64_t)d->n_u * d->n_v;
	if (K > RAY_CHUNK) throw std::runtime_error("irradiance request too large: n_u * n_v > 2^21 rays per probe");
	if (n > MAX_TRACED_RAYS || K * n > MAX_TRACED_RAYS) throw std::runtime_error("irradiance request too large: probes * n_u * n_v > 2^28 rays");
	return (uint32_t)K;
}
void check_positions(uint32_t n, const float* positions) {
	if (n && !positions) throw std::runtime_error("null argument");
	for (uint32_t i = 0; i < n; ++i)
		if (!finite3(positions + 3 * (size_t)i)) throw std::runtime_error("position " + std::to_string(i) + " is not finite");
}

// resolution and box of a volume; returns the number of probes (at most 2^28)
uint64_t check_volume_lattice(const ngp_irradiance_volume_desc* d) {
	if (!d) throw std::runtime_error("null argument");
	uint64_t probes = 1;
	for (int a = 0; a < 3; ++a) {
		if (d->res[a] == 0) throw std::runtime_error("invalid irradiance volume descriptor: the resolution must be at least 1 on every axis");
		if (!std::isfinite(d->aabb_min[a]) || !std::isfinite(d->aabb_max[a])) throw std::runtime_error("invalid irradiance volume descriptor: the box is not finite");
		if (!std::isfinite(d->aabb_max[a] - d->aabb_min[a])) throw std::runtime_error("invalid irradiance volume descriptor: the box's extent is not finite");
		if (d->res[a] > 1 && !(d->aabb_min[a] < d->aabb_max[a])) throw std::runtime_error("invalid irradiance volume descriptor: the box needs min < max on every axis with more than one probe");
		probes *= d->res[a]; // (each factor below 2^32 and the product checked after every step: no overflow)
		if (probes > MAX_TRACED_RAYS) throw std::runtime_error("irradiance volume too large: more than 2^28 probes");
	}
	return probes;
}

// probe g = i + rx (j + ry k) at min + fraction (max - min), in double from the descriptor's floats, rounded to float
std::vector<float> volume_positions(const ngp_irradiance_volume_desc* d, uint64_t probes) {
	std::vector<float> p(3 * (size_t)probes);
	size_t g = 0;
	for (uint32_t k = 0; k < d->res[2]; ++k)
		for (uint32_t j = 0; j < d->res[1]; ++j)
			for (uint32_t i = 0; i < d->res[0]; ++i, ++g) {
				const uint32_t ijk[3] = {i, j, k};
				for (int a = 0; a < 3; ++a) {
					const double lo = d->aabb_min[a], hi = d->aabb_max[a];
					const double frac = d->res[a] > 1 ? (double)ijk[a] / (double)(d->res[a] - 1) : 0.5;
					p[3 * g + a] = (float)(lo + frac * (hi - lo));
				}
			}
	return p;
}

// the records of n probes at host positions: sphere rays -> the ray-list tracer -> the projection, in chunks of whole probes. Each chunk's
// records go to h_sh (host, n x 28) and / or d_sh (device, 7 n float4), its rays' radiance to h_rays (host, n K x 4) and their alpha to
// d_alpha (device, n K floats: what the bounce passes attenuate by); all nullable.
void trace_sh_probes(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* d, uint32_t K, float* h_sh, float4* d_sh, float* h_rays,
                     float* d_alpha = nullptr) {
	const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)n * K, RAY_CHUNK);
	const uint32_t cap_pts = (uint32_t)std::min<uint64_t>(n, cap);
	DevArray<float> pts(3 * (size_t)cap_pts), o(3 * (size_t)cap), dir(3 * (size_t)cap);
	DevArray<float2> t(cap);
	DevArray<float4> rgba(cap), rec(SH_FLOAT4 * (size_t)cap_pts);
	RayListTrace tr(ctx, (uint64_t)n * K, d->min_transmittance);
	for_each_irradiance_chunk(n, K, [&](uint64_t r0, uint32_t m) { // (K <= RAY_CHUNK: whole probes)
		const uint64_t p0 = r0 / K;
		const uint32_t np = m / K;
		upload(ctx, pts.get(), positions + 3 * p0, (size_t)np * 3 * sizeof(float));
		ngp::launch_irradiance_sphere_rays(ctx->mesh_scene, d->occlude_by_meshes != 0, d->n_u, d->n_v, m, pts.get(), o.get(), dir.get(), t.get(), ctx->stream);
		ngp::launch_ray_list_prep(tr.model(), m, o.get(), dir.get(), t.get(), false, ctx->stream);
		ngp::ProbeParams P{};
		P.ray_o = o.get();
		P.ray_d = dir.get();
		P.ray_t = t.get();
		P.ray_rgba = rgba.get();
		tr.trace(P, m);
		ngp::launch_irradiance_sh_reduce(d->n_u, d->n_v, np, rgba.get(), t.get(), rec.get(), ctx->stream);
		if (d_sh) NGP_HIP_CHECK(hipMemcpyAsync(d_sh + SH_FLOAT4 * p0, rec.get(), (size_t)np * SH_FLOAT4 * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
		if (d_alpha) ngp::launch_ray_alpha(m, rgba.get(), d_alpha + r0, ctx->stream);
		if (h_rays) download(ctx, h_rays + 4 * r0, rgba.get(), (size_t)m * sizeof(float4));
		if (h_sh) download(ctx, h_sh + 4 * SH_FLOAT4 * p0, rec.get(), (size_t)np * SH_FLOAT4 * sizeof(float4));
	});
	tr.finish(); // (synchronises the stream: the chunk buffers may go)
}

// ---- probe visibility (contract: include/ngp_hip.h)
void drop_visibility(ngp_ctx* ctx) {
	ctx->d_sh_visibility.reset();
	ctx->sh_visibility_desc = ngp_irradiance_visibility_desc{};
}
void require_volume(const ngp_ctx* ctx) {
	if (!ctx->d_sh_volume) throw std::runtime_error("no irradiance volume: call ngp_compute_irradiance_volume or ngp_set_irradiance_volume first");
}
void require_visibility(const ngp_ctx* ctx) {
	if (!ctx->d_sh_visibility)
		throw std::runtime_error("no irradiance visibility: call ngp_compute_irradiance_volume_visibility or ngp_set_irradiance_volume_visibility first");
}
// the descriptor's checks shared by the visibility entries, for n probes (rays: the entry traces); returns K, 0 without rays
uint32_t check_visibility_desc(uint64_t n, const ngp_irradiance_visibility_desc* d, bool rays) {
	if (!d) throw std::runtime_error("null argument");
	if (d->sharpness_log2 > 6) throw std::runtime_error("invalid irradiance visibility descriptor: sharpness_log2 must be at most 6");
	if (!std::isfinite(d->max_distance)) throw std::runtime_error("invalid irradiance visibility descriptor: max_distance is not finite");
	if (!std::isfinite(d->normal_bias) || d->normal_bias < 0.0f) throw std::runtime_error("invalid irradiance visibility descriptor: normal_bias must be finite and >= 0");
	if (!rays) return 0;
	ngp_irradiance_sh_desc sh{};
	sh.n_u = d->n_u;
	sh.n_v = d->n_v;
	return check_sh_desc(n, &sh);
}
// D of a volume whose descriptor asks for the default: 1.5 x the diagonal of one lattice cell, an axis of one probe counting with extent
// 0; 1.5 x the box diagonal when every axis has one probe
float default_max_distance(const ngp_irradiance_volume_desc& v) {
	double cell = 0.0, box = 0.0;
	for (int a = 0; a < 3; ++a) {
		const double ext = (double)v.aabb_max[a] - (double)v.aabb_min[a];
		box += ext * ext;
		if (v.res[a] > 1) cell += (ext / (double)(v.res[a] - 1)) * (ext / (double)(v.res[a] - 1));
	}
	return (float)(1.5 * std::sqrt(v.res[0] > 1 || v.res[1] > 1 || v.res[2] > 1 ? cell : box));
}
// D of a visibility descriptor for the lattice v: its own max_distance, or the default; refused when that is no positive finite number
float visibility_distance(const ngp_irradiance_visibility_desc* d, const ngp_irradiance_volume_desc& v) {
	const float D = d->max_distance > 0.0f ? d->max_distance : default_max_distance(v);
	if (!(D > 0.0f) || !std::isfinite(D)) throw std::runtime_error("invalid irradiance visibility descriptor: the default max_distance of this volume is not a positive finite number");
	return D;
}
// the maps of n probes at host positions: sphere rays against the meshes -> the moments, in chunks of whole probes (no tracer: the maps
// need the BVHs alone). Each chunk's maps go to h_maps (host, n x 128 floats) and / or d_maps (device, 64 n float2); both nullable.
void distance_maps(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_visibility_desc* d, uint32_t K, float D, float* h_maps, float2* d_maps) {
	const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)n * K, RAY_CHUNK);
	const uint32_t cap_pts = (uint32_t)std::min<uint64_t>(n, cap);
	DevArray<float> pts(3 * (size_t)cap_pts), o(3 * (size_t)cap), dir(3 * (size_t)cap);
	DevArray<float2> t(cap), maps(ngp::DISTANCE_MAP_TEXELS * (size_t)cap_pts);
	for_each_irradiance_chunk(n, K, [&](uint64_t r0, uint32_t m) { // (K <= RAY_CHUNK: whole probes)
		const uint64_t p0 = r0 / K;
		const uint32_t np = m / K;
		upload(ctx, pts.get(), positions + 3 * p0, (size_t)np * 3 * sizeof(float));
		ngp::launch_irradiance_sphere_rays(ctx->mesh_scene, true, d->n_u, d->n_v, m, pts.get(), o.get(), dir.get(), t.get(), ctx->stream);
		ngp::launch_irradiance_distance_reduce(d->n_u, d->n_v, np, d->sharpness_log2, D, t.get(), maps.get(), ctx->stream);
		const size_t bytes = (size_t)np * ngp::DISTANCE_MAP_TEXELS * sizeof(float2);
		if (d_maps) NGP_HIP_CHECK(hipMemcpyAsync(d_maps + ngp::DISTANCE_MAP_TEXELS * p0, maps.get(), bytes, hipMemcpyDeviceToDevice, ctx->stream));
		if (h_maps) download(ctx, h_maps + 2 * ngp::DISTANCE_MAP_TEXELS * p0, maps.get(), bytes);
	});
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (the chunk buffers may go)
	NGP_HIP_CHECK(hipGetLastError());
}
void check_normals(uint32_t n, const float* normals) {
	for (uint32_t i = 0; i < n; ++i)
		if (!finite3(normals + 3 * (size_t)i) || !nonzero3(normals + 3 * (size_t)i)) throw std::runtime_error("normal " + std::to_string(i) + " is zero or not finite");
}

// ---- diffuse interreflection (contract: include/ngp_hip.h)
constexpr uint32_t MAX_BOUNCES = 16;
void check_albedo(const float* albedo) {
	if (!albedo) throw std::runtime_error("null argument");
	for (int c = 0; c < 3; ++c)
		if (!std::isfinite(albedo[c]) || albedo[c] < 0.0f || albedo[c] > 1.0f)
			throw std::runtime_error("invalid irradiance bounce descriptor: albedo must be finite and in [0, 1] on every channel");
}
// one bounce pass at n probes (host positions) from the source volume V (VV non-null: through its visible lookup): sphere rays against the
// meshes, the lookup at the hits, the projection, in chunks of whole probes (no tracer: a pass needs the BVHs and the records alone).
// d_alpha: the rays' NeRF alpha, n K floats on the device (nullable: 0). Each chunk's records R go to h_sh (host, n x 28), its rays to h_rays
// (host, n K x 4) and d_v0 + R to d_next (device, 7 n float4 each); all nullable.
void bounce_pass(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* d, uint32_t K, const float* albedo, const ngp::IrradianceVolume& V,
                 const ngp::IrradianceVolumeVisible* VV, const float* d_alpha, float* h_sh, float* h_rays, const float4* d_v0, float4* d_next) {
	const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)n * K, RAY_CHUNK);
	const uint32_t cap_pts = (uint32_t)std::min<uint64_t>(n, cap);
	DevArray<float> pts(3 * (size_t)cap_pts);
	DevArray<float2> t(cap);
	DevArray<float4> rgba(cap), rec(SH_FLOAT4 * (size_t)cap_pts);
	const ngp::Event ev0 = ngp::new_event(), ev1 = ngp::new_event();
	NGP_HIP_CHECK(hipEventRecord(ev0, ctx->stream));
	for_each_irradiance_chunk(n, K, [&](uint64_t r0, uint32_t m) { // (K <= RAY_CHUNK: whole probes)
		const uint64_t p0 = r0 / K;
		const uint32_t np = m / K;
		upload(ctx, pts.get(), positions + 3 * p0, (size_t)np * 3 * sizeof(float));
		ngp::launch_irradiance_bounce_rays(ctx->mesh_scene, V, VV, d->occlude_by_meshes != 0, d->n_u, d->n_v, m, pts.get(), albedo, d_alpha ? d_alpha + r0 : nullptr, rgba.get(),
		                                   t.get(), ctx->stream);
		ngp::launch_irradiance_sh_reduce(d->n_u, d->n_v, np, rgba.get(), t.get(), rec.get(), ctx->stream);
		if (d_next) ngp::launch_irradiance_volume_add(SH_FLOAT4 * np, d_v0 + SH_FLOAT4 * p0, rec.get(), d_next + SH_FLOAT4 * p0, ctx->stream);
		if (h_rays) download(ctx, h_rays + 4 * r0, rgba.get(), (size_t)m * sizeof(float4));
		if (h_sh) download(ctx, h_sh + 4 * SH_FLOAT4 * p0, rec.get(), (size_t)np * SH_FLOAT4 * sizeof(float4));
	});
	NGP_HIP_CHECK(hipEventRecord(ev1, ctx->stream));
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (the chunk buffers may go)
	NGP_HIP_CHECK(hipGetLastError());
	NGP_HIP_CHECK(hipEventElapsedTime(&ctx->sh_bounce_ms, ev0, ev1));
}

} // namespace

extern "C" {

int ngp_trace_nerf_rays(ngp_ctx* ctx, uint32_t n, const float* origins, const float* directions, const float* t_range, float min_transmittance, float* rgba_out,
                        float* depth_out) {
	return guarded(ctx, [&] {
		require_probe_model(ctx, "traced rays");
		if (n == 0) return;
		if (!origins || !directions || !rgba_out) throw std::runtime_error("null argument");
		for (uint32_t i = 0; i < n; ++i) {
			if (!finite3(origins + 3 * (size_t)i)) throw std::runtime_error("origin " + std::to_string(i) + " is not finite");
			if (!finite3(directions + 3 * (size_t)i) || !nonzero3(directions + 3 * (size_t)i)) throw std::runtime_error("direction " + std::to_string(i) + " is zero or not finite");
			if (t_range && (std::isnan(t_range[2 * (size_t)i]) || std::isnan(t_range[2 * (size_t)i + 1]))) throw std::runtime_error("t_range " + std::to_string(i) + " is NaN");
		}
		const uint32_t cap = std::min(n, RAY_CHUNK);
		DevArray<float> o(3 * (size_t)cap), dir(3 * (size_t)cap), depth(depth_out ? cap : 0);
		DevArray<float2> t(cap);
		DevArray<float4> rgba(cap);
		std::vector<float2> t_host(cap);
		RayListTrace tr(ctx, n, min_transmittance);
		for (uint32_t r0 = 0; r0 < n; r0 += cap) {
			const uint32_t m = std::min(cap, n - r0);
			upload(ctx, o.get(), origins + 3 * (size_t)r0, (size_t)m * 3 * sizeof(float));
			upload(ctx, dir.get(), directions + 3 * (size_t)r0, (size_t)m * 3 * sizeof(float));
			for (uint32_t i = 0; i < m; ++i)
				t_host[i] = t_range ? make_float2(t_range[2 * (size_t)(r0 + i)], t_range[2 * (size_t)(r0 + i) + 1]) : make_float2(0.0f, std::numeric_limits<float>::infinity());
			upload(ctx, t.get(), t_host.data(), (size_t)m * sizeof(float2));
			ngp::launch_ray_list_prep(tr.model(), m, o.get(), dir.get(), t.get(), true, ctx->stream);
			ngp::ProbeParams P{};
			P.ray_o = o.get();
			P.ray_d = dir.get();
			P.ray_t = t.get();
			P.ray_rgba = rgba.get();
			P.ray_depth = depth.get();
			tr.trace(P, m);
			download(ctx, rgba_out + 4 * (size_t)r0, rgba.get(), (size_t)m * sizeof(float4)); // (the stream stays in order: the next chunk's uploads wait here)
			if (depth_out) download(ctx, depth_out + r0, depth.get(), (size_t)m * sizeof(float));
		}
		tr.finish();
	});
}

int ngp_irradiance_rays(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, const ngp_irradiance_trace_desc* desc, float* origins_out,
                        float* directions_out, float* t_max_out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		const uint32_t K = check_irradiance_request(n, positions, normals, desc);
		if (n == 0) return;
		if (!origins_out || !directions_out || !t_max_out) throw std::runtime_error("null argument");
		const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)n * K, RAY_CHUNK);
		DevArray<float> pts(6 * (size_t)std::min<uint64_t>(n, cap)), o(3 * (size_t)cap), dir(3 * (size_t)cap);
		DevArray<float2> t(cap);
		std::vector<float2> t_host(cap);
		for_each_irradiance_chunk(n, K, [&](uint64_t r0, uint32_t m) {
			generate_irradiance_rays(ctx, desc, K, positions, normals, r0, m, pts, o.get(), dir.get(), t.get());
			download(ctx, origins_out + 3 * r0, o.get(), (size_t)m * 3 * sizeof(float));
			download(ctx, directions_out + 3 * r0, dir.get(), (size_t)m * 3 * sizeof(float));
			download(ctx, t_host.data(), t.get(), (size_t)m * sizeof(float2));
			for (uint32_t i = 0; i < m; ++i) t_max_out[r0 + i] = t_host[i].y;
		});
		NGP_HIP_CHECK(hipGetLastError());
	});
}

int ngp_irradiance_traced(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, const ngp_irradiance_trace_desc* desc, float* out) {
	return guarded(ctx, [&] {
		require_probe_model(ctx, "traced irradiance estimates");
		const uint32_t K = check_irradiance_request(n, positions, normals, desc);
		if (n == 0) return;
		if (!out) throw std::runtime_error("null argument");
		const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)n * K, RAY_CHUNK);
		const uint32_t cap_pts = (uint32_t)std::min<uint64_t>(n, cap);
		DevArray<float> pts(6 * (size_t)cap_pts), o(3 * (size_t)cap), dir(3 * (size_t)cap);
		DevArray<float2> t(cap);
		DevArray<float4> rgba(cap), part(1), E(cap_pts);
		RayListTrace tr(ctx, (uint64_t)n * K, desc->min_transmittance);
		for_each_irradiance_chunk(n, K, [&](uint64_t r0, uint32_t m) {
			generate_irradiance_rays(ctx, desc, K, positions, normals, r0, m, pts, o.get(), dir.get(), t.get());
			ngp::launch_ray_list_prep(tr.model(), m, o.get(), dir.get(), t.get(), false, ctx->stream);
			ngp::ProbeParams P{};
			P.ray_o = o.get();
			P.ray_d = dir.get();
			P.ray_t = t.get();
			P.ray_rgba = rgba.get();
			tr.trace(P, m);
			ngp::launch_irradiance_reduce(K, r0, m, rgba.get(), t.get(), part.get(), E.get(), ctx->stream);
			if ((r0 + m) % K == 0) { // the chunk ends a point: its points [r0 / K, (r0 + m) / K) are complete
				const uint64_t p0 = r0 / K, p1 = (r0 + m) / K;
				download(ctx, out + 4 * p0, E.get(), (size_t)(p1 - p0) * sizeof(float4));
			}
		});
		tr.finish();
	});
}

int ngp_irradiance_sphere_rays(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* desc, float* origins_out, float* directions_out,
                               float* t_max_out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		const uint32_t K = check_sh_desc(n, desc);
		check_positions(n, positions);
		if (n == 0) return;
		if (!origins_out || !directions_out || !t_max_out) throw std::runtime_error("null argument");
		const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)n * K, RAY_CHUNK);
		DevArray<float> pts(3 * (size_t)std::min<uint64_t>(n, cap)), o(3 * (size_t)cap), dir(3 * (size_t)cap);
		DevArray<float2> t(cap);
		std::vector<float2> t_host(cap);
		for_each_irradiance_chunk(n, K, [&](uint64_t r0, uint32_t m) {
			upload(ctx, pts.get(), positions + 3 * (r0 / K), (size_t)(m / K) * 3 * sizeof(float));
			ngp::launch_irradiance_sphere_rays(ctx->mesh_scene, desc->occlude_by_meshes != 0, desc->n_u, desc->n_v, m, pts.get(), o.get(), dir.get(), t.get(), ctx->stream);
			download(ctx, origins_out + 3 * r0, o.get(), (size_t)m * 3 * sizeof(float));
			download(ctx, directions_out + 3 * r0, dir.get(), (size_t)m * 3 * sizeof(float));
			download(ctx, t_host.data(), t.get(), (size_t)m * sizeof(float2));
			for (uint32_t i = 0; i < m; ++i) t_max_out[r0 + i] = t_host[i].y;
		});
		NGP_HIP_CHECK(hipGetLastError());
	});
}

int ngp_irradiance_sh_traced(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* desc, float* sh_out, float* rays_rgba_out) {
	return guarded(ctx, [&] {
		require_probe_model(ctx, "SH irradiance probes");
		const uint32_t K = check_sh_desc(n, desc);
		check_positions(n, positions);
		if (n == 0) return;
		if (!sh_out) throw std::runtime_error("null argument");
		trace_sh_probes(ctx, n, positions, desc, K, sh_out, nullptr, rays_rgba_out);
	});
}

int ngp_compute_irradiance_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc) {
	return guarded(ctx, [&] {
		require_probe_model(ctx, "SH irradiance probes");
		const uint64_t probes = check_volume_lattice(desc);
		const uint32_t K = check_sh_desc(probes, &desc->sh);
		const std::vector<float> positions = volume_positions(desc, probes);
		DevArray<float4> sh(SH_FLOAT4 * (size_t)probes);
		trace_sh_probes(ctx, (uint32_t)probes, positions.data(), &desc->sh, K, nullptr, sh.get(), nullptr);
		ctx->d_sh_volume = std::move(sh); // (the previous volume stays in place when the trace throws)
		ctx->sh_volume_desc = *desc;
		drop_visibility(ctx); // (the lattice may have changed)
		++ctx->sh_volume_generation;
	});
}

int ngp_compute_irradiance_volume_bounced(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const ngp_irradiance_bounce_desc* bounce,
                                          const ngp_irradiance_visibility_desc* visibility) {
	return guarded(ctx, [&] {
		if (!bounce) throw std::runtime_error("null argument");
		if (bounce->n_bounces > MAX_BOUNCES) throw std::runtime_error("invalid irradiance bounce descriptor: n_bounces must be at most 16");
		check_albedo(bounce->albedo);
		require_probe_model(ctx, "SH irradiance probes");
		const uint64_t probes = check_volume_lattice(desc);
		const uint32_t K = check_sh_desc(probes, &desc->sh);
		const uint32_t K_vis = visibility ? check_visibility_desc(probes, visibility, true) : 0;
		const float D = visibility ? visibility_distance(visibility, *desc) : 0.0f;
		const std::vector<float> positions = volume_positions(desc, probes);
		// without a source (no pass asked for, a black albedo, nothing to hit) the records are V_0's own: no pass runs
		const float* al = bounce->albedo;
		const uint32_t n_bounces = (al[0] != 0.0f || al[1] != 0.0f || al[2] != 0.0f) && !ctx->meshes.empty() && desc->sh.occlude_by_meshes != 0 ? bounce->n_bounces : 0;
		DevArray<float4> v0(SH_FLOAT4 * (size_t)probes), even(n_bounces > 1 ? v0.size() : 0), odd(n_bounces > 0 ? v0.size() : 0);
		DevArray<float> alpha(n_bounces ? (size_t)probes * K : 0); // the whole volume's rays: the NeRF is traced once
		trace_sh_probes(ctx, (uint32_t)probes, positions.data(), &desc->sh, K, nullptr, v0.get(), nullptr, n_bounces ? alpha.get() : nullptr);
		DevArray<float2> maps(visibility ? ngp::DISTANCE_MAP_TEXELS * (size_t)probes : 0);
		if (visibility) distance_maps(ctx, (uint32_t)probes, positions.data(), visibility, K_vis, D, nullptr, maps.get());
		ngp::IrradianceVolumeVisible A{};
		for (int a = 0; a < 3; ++a) {
			A.V.res[a] = desc->res[a];
			A.V.lo[a] = desc->aabb_min[a];
			A.V.hi[a] = desc->aabb_max[a];
		}
		A.maps = maps.get();
		A.D = D;
		A.normal_bias = visibility ? visibility->normal_bias : 0.0f;
		const float4* prev = v0.get();
		for (uint32_t b = 1; b <= n_bounces; ++b) { // V_b = V_0 + R(V_{b-1}): every probe of a pass reads the pass before it alone
			float4* next = b % 2u ? odd.get() : even.get();
			A.V.sh = prev;
			bounce_pass(ctx, (uint32_t)probes, positions.data(), &desc->sh, K, al, A.V, visibility ? &A : nullptr, alpha.get(), nullptr, nullptr, v0.get(), next);
			prev = next;
		}
		ctx->d_sh_volume = std::move(n_bounces == 0 ? v0 : n_bounces % 2u ? odd : even); // (the previous volume stays in place when a launch throws)
		ctx->sh_volume_desc = *desc;
		drop_visibility(ctx);
		if (visibility) {
			ctx->d_sh_visibility = std::move(maps);
			ctx->sh_visibility_desc = *visibility;
			ctx->sh_visibility_desc.max_distance = D;
		}
		++ctx->sh_volume_generation;
	});
}

int ngp_irradiance_sh_bounce(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* desc, const float* albedo, const float* alpha, int use_visible,
                             float* sh_out, float* rays_out) {
	return guarded(ctx, [&] {
		check_albedo(albedo);
		require_device(ctx);
		require_volume(ctx);
		if (use_visible) require_visibility(ctx);
		const uint32_t K = check_sh_desc(n, desc);
		check_positions(n, positions);
		if (n == 0) return;
		if (!sh_out) throw std::runtime_error("null argument");
		const size_t rays = (size_t)n * K;
		if (alpha)
			for (size_t i = 0; i < rays; ++i)
				if (!std::isfinite(alpha[i])) throw std::runtime_error("alpha " + std::to_string(i) + " is not finite");
		DevArray<float> d_alpha(alpha ? rays : 0);
		if (alpha) upload(ctx, d_alpha.get(), alpha, rays * sizeof(float));
		const ngp::IrradianceVolumeVisible A = use_visible ? ngp::sh_volume_visible_of(ctx) : ngp::IrradianceVolumeVisible{};
		bounce_pass(ctx, n, positions, desc, K, albedo, ngp::sh_volume_of(ctx), use_visible ? &A : nullptr, alpha ? d_alpha.get() : nullptr, sh_out, rays_out, nullptr, nullptr);
	});
}

int ngp_get_irradiance_bounce_ms(ngp_ctx* ctx, float* ms) {
	return guarded(ctx, [&] {
		require_device(ctx);
		if (!ms) throw std::runtime_error("null argument");
		*ms = ctx->sh_bounce_ms;
	});
}

int ngp_set_irradiance_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const float* sh) {
	return guarded(ctx, [&] {
		require_device(ctx);
		const uint64_t probes = check_volume_lattice(desc);
		if (!sh) throw std::runtime_error("null argument");
		for (size_t i = 0; i < 4 * SH_FLOAT4 * (size_t)probes; ++i)
			if (!std::isfinite(sh[i])) throw std::runtime_error("irradiance volume: value " + std::to_string(i % 28) + " of probe " + std::to_string(i / 28) + " is not finite");
		DevArray<float4> d;
		d.upload(reinterpret_cast<const float4*>(sh), SH_FLOAT4 * (size_t)probes);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (a lookup still in flight reads the old records)
		ctx->d_sh_volume = std::move(d);
		ctx->sh_volume_desc = *desc;
		drop_visibility(ctx);
		++ctx->sh_volume_generation;
	});
}

int ngp_get_irradiance_volume(ngp_ctx* ctx, ngp_irradiance_volume_desc* desc_out, float* sh_out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		if (!ctx->d_sh_volume) throw std::runtime_error("no irradiance volume: call ngp_compute_irradiance_volume or ngp_set_irradiance_volume first");
		if (desc_out) *desc_out = ctx->sh_volume_desc;
		if (sh_out) download(ctx, sh_out, ctx->d_sh_volume.get(), ctx->d_sh_volume.size() * sizeof(float4));
	});
}

int ngp_clear_irradiance_volume(ngp_ctx* ctx) {
	return guarded(ctx, [&] {
		require_device(ctx);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		ctx->d_sh_volume.reset();
		ctx->sh_volume_desc = ngp_irradiance_volume_desc{};
		drop_visibility(ctx);
		++ctx->sh_volume_generation;
		for (ngp_ctx* p : ctx->peers) { // the replicas go too: a multi-device frame refuses like a single-device one
			ngp::DeviceGuard g(p->device);
			NGP_HIP_CHECK(hipStreamSynchronize(p->stream));
			p->d_sh_volume.reset();
			p->sh_volume_desc = ngp_irradiance_volume_desc{};
			drop_visibility(p);
			p->synced_sh_volume_generation = ctx->sh_volume_generation;
		}
	});
}

int ngp_irradiance_volume_at(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, float* out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		if (!ctx->d_sh_volume) throw std::runtime_error("no irradiance volume: call ngp_compute_irradiance_volume or ngp_set_irradiance_volume first");
		if (n == 0) return;
		if (!positions || !normals || !out) throw std::runtime_error("null argument");
		check_positions(n, positions);
		for (uint32_t i = 0; i < n; ++i)
			if (!finite3(normals + 3 * (size_t)i) || !nonzero3(normals + 3 * (size_t)i)) throw std::runtime_error("normal " + std::to_string(i) + " is zero or not finite");
		DevArray<float> d_p(3 * (size_t)n), d_n(3 * (size_t)n);
		DevArray<float4> d_o(n);
		upload(ctx, d_p.get(), positions, (size_t)n * 3 * sizeof(float));
		upload(ctx, d_n.get(), normals, (size_t)n * 3 * sizeof(float));
		ngp::launch_irradiance_volume_lookup(ngp::sh_volume_of(ctx), n, d_p.get(), d_n.get(), d_o.get(), ctx->stream);
		download(ctx, out, d_o.get(), (size_t)n * sizeof(float4));
		NGP_HIP_CHECK(hipGetLastError());
	});
}

int ngp_irradiance_distance_maps(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_visibility_desc* desc, float* maps_out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		const uint32_t K = check_visibility_desc(n, desc, true);
		if (!(desc->max_distance > 0.0f)) throw std::runtime_error("invalid irradiance visibility descriptor: max_distance must be > 0 here");
		check_positions(n, positions);
		if (n == 0) return;
		if (!maps_out) throw std::runtime_error("null argument");
		distance_maps(ctx, n, positions, desc, K, desc->max_distance, maps_out, nullptr);
	});
}

int ngp_compute_irradiance_volume_visibility(ngp_ctx* ctx, const ngp_irradiance_visibility_desc* desc) {
	return guarded(ctx, [&] {
		require_device(ctx);
		require_volume(ctx);
		const uint64_t probes = ctx->d_sh_volume.size() / SH_FLOAT4;
		const uint32_t K = check_visibility_desc(probes, desc, true);
		const float D = visibility_distance(desc, ctx->sh_volume_desc);
		const std::vector<float> positions = volume_positions(&ctx->sh_volume_desc, probes);
		DevArray<float2> maps(ngp::DISTANCE_MAP_TEXELS * (size_t)probes);
		distance_maps(ctx, (uint32_t)probes, positions.data(), desc, K, D, nullptr, maps.get());
		ctx->d_sh_visibility = std::move(maps); // (the previous maps stay in place when a launch throws)
		ctx->sh_visibility_desc = *desc;
		ctx->sh_visibility_desc.max_distance = D;
		++ctx->sh_volume_generation;
	});
}

int ngp_get_irradiance_volume_visibility(ngp_ctx* ctx, ngp_irradiance_visibility_desc* desc_out, float* maps_out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		require_volume(ctx);
		require_visibility(ctx);
		if (desc_out) *desc_out = ctx->sh_visibility_desc;
		if (maps_out) download(ctx, maps_out, ctx->d_sh_visibility.get(), ctx->d_sh_visibility.size() * sizeof(float2));
	});
}

int ngp_set_irradiance_volume_visibility(ngp_ctx* ctx, const ngp_irradiance_visibility_desc* desc, const float* maps) {
	return guarded(ctx, [&] {
		require_device(ctx);
		require_volume(ctx);
		check_visibility_desc(0, desc, false);
		if (!(desc->max_distance > 0.0f)) throw std::runtime_error("invalid irradiance visibility descriptor: max_distance must be > 0 for maps that are set");
		if (!maps) throw std::runtime_error("null argument");
		const size_t probes = ctx->d_sh_volume.size() / SH_FLOAT4, texels = ngp::DISTANCE_MAP_TEXELS * probes;
		for (size_t i = 0; i < 2 * texels; ++i)
			if (!std::isfinite(maps[i]) || maps[i] < 0.0f)
				throw std::runtime_error("irradiance visibility: m" + std::to_string(i % 2 + 1) + " of texel " + std::to_string(i / 2 % 64) + " of probe " + std::to_string(i / 128) +
				                         (std::isfinite(maps[i]) ? " is negative" : " is not finite"));
		DevArray<float2> d;
		d.upload(reinterpret_cast<const float2*>(maps), texels);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (a lookup still in flight reads the old maps)
		ctx->d_sh_visibility = std::move(d);
		ctx->sh_visibility_desc = *desc;
		++ctx->sh_volume_generation;
	});
}

int ngp_clear_irradiance_volume_visibility(ngp_ctx* ctx) {
	return guarded(ctx, [&] {
		require_device(ctx);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
		drop_visibility(ctx);
		++ctx->sh_volume_generation;
	});
}

int ngp_irradiance_volume_at_visible(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, float* out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		require_volume(ctx);
		require_visibility(ctx);
		if (n == 0) return;
		if (!positions || !normals || !out) throw std::runtime_error("null argument");
		check_positions(n, positions);
		check_normals(n, normals);
		DevArray<float> d_p(3 * (size_t)n), d_n(3 * (size_t)n);
		DevArray<float4> d_o(n);
		upload(ctx, d_p.get(), positions, (size_t)n * 3 * sizeof(float));
		upload(ctx, d_n.get(), normals, (size_t)n * 3 * sizeof(float));
		ngp::launch_irradiance_volume_lookup_visible(ngp::sh_volume_visible_of(ctx), n, d_p.get(), d_n.get(), d_o.get(), ctx->stream);
		download(ctx, out, d_o.get(), (size_t)n * sizeof(float4));
		NGP_HIP_CHECK(hipGetLastError());
	});
}

int ngp_irradiance_sh_eval(uint32_t n, const float* sh, const float* normals, float* rgb_out) {
	if (n == 0) return 0;
	if (!sh || !normals || !rgb_out) return -2;
	for (uint32_t i = 0; i < n; ++i) {
		const float* nr = normals + 3 * (size_t)i;
		if (!finite3(nr) || !nonzero3(nr)) return -1;
		const double x = nr[0], y = nr[1], z = nr[2], len = std::sqrt(x * x + y * y + z * z);
		double E[3];
		ngp::sh9_irradiance(sh + 28 * (size_t)i, x / len, y / len, z / len, E);
		for (int c = 0; c < 3; ++c) rgb_out[3 * (size_t)i + c] = (float)E[c];
	}
	return 0;
}

} // extern "C"

// Geometry mode on a multi-device context (the reference's render_frame serves every mode on every device, src/testbed.cu:4833-4889,
// 5575-5616): an auxiliary device gets the primary's meshes exactly as built (same triangle order, same BVH4 nodes -- rebuilt nowhere),
// the BRDF / sun parameters and, when they were computed, the tabulated irradiance E(n) and the SH9 irradiance volume. Generation counters: only what changed moves.
namespace ngp {
void sync_peer_geometry(ngp_ctx* primary, ngp_ctx* peer) {
	peer->shade = primary->shade;
	if (peer->synced_mesh_generation != primary->mesh_generation) {
		DeviceGuard g(peer->device);
		NGP_HIP_CHECK(hipStreamSynchronize(peer->stream)); // (a rare event: frames on the peer still trace the old BVHs)
		peer->meshes.clear();
		for (const HostMesh& m : primary->meshes) { // uploaded from the primary's host copies; the replica keeps none
			HostMesh c;
			memcpy(c.bmin, m.bmin, sizeof(c.bmin));
			memcpy(c.bmax, m.bmax, sizeof(c.bmax));
			memcpy(c.center, m.center, sizeof(c.center));
			c.d_tris.upload(m.tris.data(), m.tris.size());
			c.d_nodes.upload(m.nodes.data(), m.nodes.size());
			peer->meshes.push_back(std::move(c));
		}
		rebuild_scene(peer);
		peer->synced_mesh_generation = primary->mesh_generation;
	}
	if (peer->synced_probe_generation != primary->probe_generation && primary->d_irradiance) {
		const size_t texels = (size_t)primary->env_n_theta * primary->env_n_phi * (primary->env_probe.mode == 3 ? (size_t)primary->env_probe.grid_x * primary->env_probe.grid_y : 1u);
		{
			DeviceGuard g(peer->device);
			NGP_HIP_CHECK(hipStreamSynchronize(peer->stream));
			peer->d_envmap.reset(), peer->d_irradiance.reset();
			peer->d_envmap.reset(texels);
			peer->d_irradiance.reset(texels);
		}
		NGP_HIP_CHECK(hipStreamSynchronize(primary->stream)); // compute_probes ends synchronised; a no-op in practice
		NGP_HIP_CHECK(hipMemcpyPeer(peer->d_envmap.get(), peer->device, primary->d_envmap.get(), primary->device, texels * sizeof(float4)));
		NGP_HIP_CHECK(hipMemcpyPeer(peer->d_irradiance.get(), peer->device, primary->d_irradiance.get(), primary->device, texels * sizeof(float4)));
		peer->env_probe = primary->env_probe;
		peer->env_n_theta = primary->env_n_theta;
		peer->env_n_phi = primary->env_n_phi;
		peer->synced_probe_generation = primary->probe_generation;
	}
	if (peer->synced_sh_volume_generation != primary->sh_volume_generation) { // (a cleared volume: the replica is dropped, the peer's frame refuses)
		const size_t n = primary->d_sh_volume.size();
		{
			DeviceGuard g(peer->device);
			NGP_HIP_CHECK(hipStreamSynchronize(peer->stream)); // frames on the peer still read the old records
			peer->d_sh_volume.reset();
			if (n) peer->d_sh_volume.reset(n);
		}
		if (n) {
			NGP_HIP_CHECK(hipStreamSynchronize(primary->stream)); // the trace / upload that wrote the records ends synchronised; a no-op in practice
			DeviceGuard g(peer->device);
			NGP_HIP_CHECK(hipMemcpyPeer(peer->d_sh_volume.get(), peer->device, primary->d_sh_volume.get(), primary->device, n * sizeof(float4)));
		}
		const size_t nv = primary->d_sh_visibility.size(); // the distance maps follow the records (a volume without visibility: the replica's are dropped)
		{
			DeviceGuard g(peer->device);
			peer->d_sh_visibility.reset();
			if (nv) {
				peer->d_sh_visibility.reset(nv);
				NGP_HIP_CHECK(hipMemcpyPeer(peer->d_sh_visibility.get(), peer->device, primary->d_sh_visibility.get(), primary->device, nv * sizeof(float2)));
			}
		}
		peer->sh_visibility_desc = primary->sh_visibility_desc;
		peer->sh_volume_desc = primary->sh_volume_desc;
		peer->synced_sh_volume_generation = primary->sh_volume_generation;
	}
}
} // namespace ngp
