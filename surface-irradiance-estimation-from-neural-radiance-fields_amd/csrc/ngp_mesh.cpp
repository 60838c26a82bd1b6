// Geometry mode, host side of the C ABI: Testbed::load_scene / load_mesh (reference
// src/testbed_geometry_training.cu:2751-2866, 3101-3210), the BVH4 build (src/triangle_bvh.cu:425-508) and the
// .obj reader that replaces the vendored tinyobjloader wrapper (src/tinyobj_loader_wrapper.cu).
#include "ngp_host.h"
#include "bvh4_build.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>

using namespace ngp;

namespace {

using namespace ngp::bvh4; // V3 and its helpers, bounds, build_bvh4

// the device table of the meshes' materials (ngp_kernels.h MeshMaterial), whole, from the host's copies; dropped while no mesh owns one, which is
// what sends a frame to the kernels without materials. Frames in flight may read the old table: the device is waited for first (a rare event,
// as the mesh list's own upload is).
void upload_mesh_materials(ngp_ctx* ctx) {
	++ctx->material_generation;
	ctx->n_own_materials = 0;
	for (const HostMesh& m : ctx->meshes) ctx->n_own_materials += m.own_material ? 1u : 0u;
	if (ctx->device < 0) return;
	DeviceGuard g(ctx->device);
	if (ctx->d_mesh_materials) {
		NGP_HIP_CHECK(hipDeviceSynchronize());
		ctx->d_mesh_materials.reset();
	}
	if (!ctx->n_own_materials) return;
	std::vector<MeshMaterial> table(ctx->meshes.size());
	for (size_t i = 0; i < table.size(); ++i) {
		static_assert(sizeof(ngp_mesh_material) == 13 * sizeof(float) && offsetof(MeshMaterial, own) == sizeof(ngp_mesh_material), "material record layout");
		memset(&table[i], 0, sizeof(MeshMaterial));
		memcpy(&table[i], &ctx->meshes[i].material, sizeof(ngp_mesh_material));
		table[i].own = ctx->meshes[i].own_material ? 1u : 0u;
	}
	ctx->d_mesh_materials.upload(table.data(), table.size());
}

// the fields of a material in the header's order, for refusals and the scene file's keys; a colour is three floats
struct MaterialField {
	const char* name;
	size_t offset;
	int n;
};
const MaterialField MATERIAL_FIELDS[] = {
	{"metallic", offsetof(ngp_mesh_material, metallic), 1},   {"subsurface", offsetof(ngp_mesh_material, subsurface), 1},
	{"specular", offsetof(ngp_mesh_material, specular), 1},   {"roughness", offsetof(ngp_mesh_material, roughness), 1},
	{"sheen", offsetof(ngp_mesh_material, sheen), 1},         {"clearcoat", offsetof(ngp_mesh_material, clearcoat), 1},
	{"clearcoat_gloss", offsetof(ngp_mesh_material, clearcoat_gloss), 1},
	{"basecolor", offsetof(ngp_mesh_material, basecolor), 3}, {"ambientcolor", offsetof(ngp_mesh_material, ambientcolor), 3},
};
const float* material_field(const ngp_mesh_material& m, const MaterialField& f) { return (const float*)((const char*)&m + f.offset); }
ngp_mesh_material default_material() {
	ngp_mesh_material m{};
	m.specular = 1.0f;
	m.roughness = 0.5f;
	m.basecolor[0] = m.basecolor[1] = m.basecolor[2] = 0.8f;
	return m;
}
void check_material(const ngp_mesh_material& m, const std::string& where) {
	for (const MaterialField& f : MATERIAL_FIELDS)
		for (int i = 0; i < f.n; ++i)
			if (!std::isfinite(material_field(m, f)[i])) throw std::runtime_error(where + "material field '" + f.name + "' is not finite");
}
// the "material" object of a scene file's "Mesh" entry: missing keys take the header's defaults
ngp_mesh_material parse_material(const mj::Value& v, const std::string& where) {
	if (!v.is_object()) throw std::runtime_error(where + "'material' must be an object");
	ngp_mesh_material m = default_material();
	for (const auto& kv : v.obj) {
		const MaterialField* field = nullptr;
		for (const MaterialField& f : MATERIAL_FIELDS)
			if (kv.first == f.name) field = &f;
		if (!field) throw std::runtime_error(where + "unknown material key '" + kv.first + "'");
		float* dst = const_cast<float*>(material_field(m, *field));
		if (field->n == 1) {
			if (!kv.second.is_number()) throw std::runtime_error(where + "material key '" + kv.first + "' must be a number");
			dst[0] = (float)kv.second.num();
		} else {
			if (!kv.second.is_array() || kv.second.size() != 3) throw std::runtime_error(where + "material key '" + kv.first + "' must be an array of 3 numbers");
			for (size_t i = 0; i < 3; ++i) {
				if (!kv.second.at(i).is_number()) throw std::runtime_error(where + "material key '" + kv.first + "' must be an array of 3 numbers");
				dst[i] = (float)kv.second.at(i).num();
			}
		}
	}
	check_material(m, where);
	return m;
}
// three channels of a mesh's albedo: each finite and in [0, 1]
void check_mesh_albedo(const float* a, const std::string& where) {
	for (int c = 0; c < 3; ++c)
		if (!std::isfinite(a[c]) || a[c] < 0.0f || a[c] > 1.0f) throw std::runtime_error(where + "mesh albedo must be finite and in [0, 1] on every channel");
}
// what a scene file's "Mesh" entry carries beside its path: its material and its albedo, where it has them
struct SceneEntryExtras {
	bool own_material = false, own_albedo = false;
	ngp_mesh_material material{};
	float albedo[3] = {0.f, 0.f, 0.f};
};
// the "albedo" array of a scene file's "Mesh" entry
void parse_albedo(const mj::Value& v, const std::string& where, float* out) {
	if (!v.is_array() || v.size() != 3) throw std::runtime_error(where + "'albedo' must be an array of 3 numbers");
	for (size_t i = 0; i < 3; ++i) {
		if (!v.at(i).is_number()) throw std::runtime_error(where + "'albedo' must be an array of 3 numbers");
		out[i] = (float)v.at(i).num();
	}
	check_mesh_albedo(out, where);
}
HostMesh& mesh_slot(ngp_ctx* ctx, int mesh) {
	if (mesh < 0 || mesh >= (int)ctx->meshes.size())
		throw std::runtime_error("mesh: index " + std::to_string(mesh) + " outside [0, " + std::to_string(ctx->meshes.size()) + ") (ngp_n_meshes)");
	return ctx->meshes[(size_t)mesh];
}

// after any change of the mesh list: scene AABB (load_scene :3183-3189) and the device-side MeshRef table
void rebuild_scene(ngp_ctx* ctx) {
	++ctx->mesh_generation;
	ctx->d_meshrefs.reset();
	ctx->mesh_scene = MeshSceneParams{};
	upload_mesh_materials(ctx); // (the table follows the list: a slot's material goes with its mesh)
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
		// the entries' materials and albedos are read and refused before the scene is touched
		std::vector<SceneEntryExtras> extras;
		for (const mj::Value& g : geometries.arr) {
			const mj::Value* mat = g.is_object() ? g.find("material") : nullptr;
			const mj::Value* alb = g.is_object() ? g.find("albedo") : nullptr;
			const std::string where = "geometry[" + std::to_string(extras.size()) + "]: ";
			const bool nerf = g.contains("type") && g.at("type").is_string() && g.at("type").str() == "Nerf";
			if (mat && nerf) throw std::runtime_error(where + "'material' applies to a 'Mesh' entry, not to 'Nerf'");
			if (alb && nerf) throw std::runtime_error(where + "'albedo' applies to a 'Mesh' entry, not to 'Nerf'");
			SceneEntryExtras e;
			e.own_material = mat != nullptr;
			if (mat) e.material = parse_material(*mat, where);
			e.own_albedo = alb != nullptr;
			if (alb) parse_albedo(*alb, where, e.albedo);
			extras.push_back(e);
		}
		ctx->meshes.clear();
		size_t entry = 0;
		for (const mj::Value& g : geometries.arr) {
			const SceneEntryExtras& e = extras[entry++];
			std::string path = g.at("path").str();
			if (!path.empty() && path[0] != '/') path = base + "/" + path;
			const std::string& type = g.at("type").str();
			float center[3];
			for (int i = 0; i < 3; ++i) center[i] = (float)g.at("center").at((size_t)i).num();
			if (type == "Mesh") {
				load_mesh_file_impl(ctx, path, center);
				ctx->meshes.back().own_material = e.own_material;
				ctx->meshes.back().material = e.material;
				ctx->meshes.back().own_albedo = e.own_albedo;
				memcpy(ctx->meshes.back().albedo, e.albedo, sizeof(e.albedo));
			} else if (type == "Nerf") load_snapshot_path(ctx, path);
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

int ngp_set_mesh_material(ngp_ctx* ctx, int mesh, const ngp_mesh_material* m) {
	return guarded(ctx, [&] {
		HostMesh& slot = mesh_slot(ctx, mesh);
		if (m) check_material(*m, "");
		slot.own_material = m != nullptr;
		slot.material = m ? *m : ngp_mesh_material{};
		upload_mesh_materials(ctx);
	});
}

int ngp_get_mesh_material(ngp_ctx* ctx, int mesh, ngp_mesh_material* out, int* own) {
	return guarded(ctx, [&] {
		const HostMesh& slot = mesh_slot(ctx, mesh);
		if (own) *own = slot.own_material ? 1 : 0;
		if (!out) return;
		if (slot.own_material) *out = slot.material;
		else memcpy(out, &ctx->shade.metallic, sizeof(ngp_mesh_material)); // (the BRDF part of ngp_geometry_opts has the material's layout)
	});
}

// (no device state: the passes of the SH9 volume resolve a table per call, ngp_irradiance.cpp)
int ngp_set_mesh_albedo(ngp_ctx* ctx, int mesh, const float* albedo) {
	return guarded(ctx, [&] {
		HostMesh& slot = mesh_slot(ctx, mesh);
		if (albedo) check_mesh_albedo(albedo, "");
		slot.own_albedo = albedo != nullptr;
		for (int c = 0; c < 3; ++c) slot.albedo[c] = albedo ? albedo[c] : 0.0f;
	});
}

int ngp_get_mesh_albedo(ngp_ctx* ctx, int mesh, float* out, int* own) {
	return guarded(ctx, [&] {
		const HostMesh& slot = mesh_slot(ctx, mesh);
		if (own) *own = slot.own_albedo ? 1 : 0;
		if (out) memcpy(out, slot.albedo, sizeof(slot.albedo)); // (zeros without one)
	});
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
} // extern "C"

// Geometry mode on a multi-device context (the reference's render_frame serves every mode on every device, src/testbed.cu:4833-4889,
// 5575-5616): an auxiliary device gets the primary's meshes exactly as built (same triangle order, same BVH4 nodes -- rebuilt nowhere),
// the BRDF / sun parameters and, when they were computed, the tabulated irradiance E(n) and the SH9 irradiance volume. Generation counters: only what changed moves.
namespace ngp {
void sync_peer_geometry(ngp_ctx* primary, ngp_ctx* peer) {
	peer->shade = primary->shade;
	peer->options = primary->options;
	const bool meshes_changed = peer->synced_mesh_generation != primary->mesh_generation;
	if (!meshes_changed && peer->synced_material_generation != primary->material_generation) { // the materials alone: the slots' copies and the table
		for (size_t i = 0; i < peer->meshes.size(); ++i) {
			peer->meshes[i].material = primary->meshes[i].material;
			peer->meshes[i].own_material = primary->meshes[i].own_material;
		}
		upload_mesh_materials(peer);
	}
	peer->synced_material_generation = primary->material_generation; // (a new mesh list brings its materials below: rebuild_scene uploads them)
	if (meshes_changed) {
		DeviceGuard g(peer->device);
		NGP_HIP_CHECK(hipStreamSynchronize(peer->stream)); // (a rare event: frames on the peer still trace the old BVHs)
		peer->meshes.clear();
		for (const HostMesh& m : primary->meshes) { // uploaded from the primary's host copies; the replica keeps none
			HostMesh c;
			memcpy(c.bmin, m.bmin, sizeof(c.bmin));
			memcpy(c.bmax, m.bmax, sizeof(c.bmax));
			memcpy(c.center, m.center, sizeof(c.center));
			c.material = m.material;
			c.own_material = m.own_material;
			memcpy(c.albedo, m.albedo, sizeof(c.albedo)); // (nothing on a peer reads it: the volume is computed on the primary)
			c.own_albedo = m.own_albedo;
			c.d_tris.upload(m.tris.data(), m.tris.size());
			c.d_nodes.upload(m.nodes.data(), m.nodes.size());
			peer->meshes.push_back(std::move(c));
		}
		rebuild_scene(peer);
		peer->synced_mesh_generation = primary->mesh_generation;
	}
	if (peer->synced_probe_generation != primary->probe_generation && primary->d_irradiance) {
		const size_t texels = env_texels(primary);
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
	if (peer->synced_sh_reference_generation != primary->sh_reference_generation) { // the reference volume, as the volume above (it has no maps)
		const size_t n = primary->d_sh_reference.size();
		{
			DeviceGuard g(peer->device);
			NGP_HIP_CHECK(hipStreamSynchronize(peer->stream)); // frames on the peer still read the old records
			peer->d_sh_reference.reset();
			if (n) peer->d_sh_reference.reset(n);
		}
		if (n) {
			NGP_HIP_CHECK(hipStreamSynchronize(primary->stream));
			DeviceGuard g(peer->device);
			NGP_HIP_CHECK(hipMemcpyPeer(peer->d_sh_reference.get(), peer->device, primary->d_sh_reference.get(), primary->device, n * sizeof(float4)));
		}
		peer->sh_reference_desc = primary->sh_reference_desc;
		peer->synced_sh_reference_generation = primary->sh_reference_generation;
	}
}
} // namespace ngp
