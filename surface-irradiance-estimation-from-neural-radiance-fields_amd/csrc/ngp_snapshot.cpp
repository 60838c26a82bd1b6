// Snapshots (.msgpack / .ingp, the reference's format): a file is parsed and checked as a whole, then committed to the
// context; the writer; the session state and camera a snapshot carries.
#include "ngp_host.h"

#include <zlib.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>

using namespace ngp;

namespace ngp {
uint16_t float_to_half(float f) { // round to nearest even, for "params_type": "float" snapshots
	uint32_t x;
	memcpy(&x, &f, 4);
	uint32_t sign = (x >> 16) & 0x8000u;
	int32_t exp = (int32_t)((x >> 23) & 0xff) - 127 + 15;
	uint32_t man = x & 0x7fffffu;
	if (((x >> 23) & 0xff) == 0xff) return (uint16_t)(sign | 0x7c00u | (man ? 0x200u : 0));
	if (exp >= 31) return (uint16_t)(sign | 0x7c00u);
	if (exp <= 0) {
		if (exp < -10) return (uint16_t)sign;
		man |= 0x800000u;
		uint32_t shift = (uint32_t)(14 - exp);
		uint32_t half_man = man >> shift;
		uint32_t rem = man & ((1u << shift) - 1u);
		uint32_t halfway = 1u << (shift - 1);
		if (rem > halfway || (rem == halfway && (half_man & 1u))) ++half_man;
		return (uint16_t)(sign | half_man);
	}
	uint32_t half = (uint32_t)(exp << 10) | (man >> 13);
	uint32_t rem = man & 0x1fffu;
	if (rem > 0x1000u || (rem == 0x1000u && (half & 1u))) ++half;
	return (uint16_t)(sign | half);
}

void read_vec(const mj::Value& v, float* out, size_t n) {
	if (!v.is_array() || v.size() != n) throw std::runtime_error("snapshot: vector of unexpected size");
	for (size_t i = 0; i < n; ++i) out[i] = (float)v.at(i).num();
}
} // namespace ngp

namespace {

std::string inflate_all(const void* data, size_t n) { // zlib or gzip container (zstr, src/testbed.cu:262-266)
	z_stream zs;
	memset(&zs, 0, sizeof(zs));
	if (inflateInit2(&zs, 15 + 32) != Z_OK) throw std::runtime_error("inflateInit2 failed");
	zs.next_in = (Bytef*)data;
	zs.avail_in = (uInt)n;
	std::string out;
	std::vector<char> buf(1 << 20);
	int rc;
	do {
		zs.next_out = (Bytef*)buf.data();
		zs.avail_out = (uInt)buf.size();
		rc = inflate(&zs, Z_NO_FLUSH);
		if (rc != Z_OK && rc != Z_STREAM_END) {
			inflateEnd(&zs);
			throw std::runtime_error("inflate failed: corrupt .ingp stream");
		}
		out.append(buf.data(), buf.size() - zs.avail_out);
	} while (rc != Z_STREAM_END);
	inflateEnd(&zs);
	return out;
}

std::string deflate_gzip(const std::string& in, int level) {
	z_stream zs;
	memset(&zs, 0, sizeof(zs));
	if (deflateInit2(&zs, level, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("deflateInit2 failed");
	zs.next_in = (Bytef*)in.data();
	zs.avail_in = (uInt)in.size();
	std::string out;
	std::vector<char> buf(1 << 20);
	int rc;
	do {
		zs.next_out = (Bytef*)buf.data();
		zs.avail_out = (uInt)buf.size();
		rc = deflate(&zs, Z_FINISH);
		out.append(buf.data(), buf.size() - zs.avail_out);
	} while (rc != Z_STREAM_END);
	deflateEnd(&zs);
	return out;
}

// tcnn vec_json.h: a tmat<T,N,M> is an array of M rows with N entries each; storage is column-major
void read_mat(const mj::Value& v, float* out, int n_cols, int n_rows) {
	if (!v.is_array() || (int)v.size() != n_rows) throw std::runtime_error("snapshot: matrix of unexpected size");
	for (int r = 0; r < n_rows; ++r) {
		const mj::Value& row = v.at((size_t)r);
		if (!row.is_array() || (int)row.size() != n_cols) throw std::runtime_error("snapshot: matrix of unexpected size");
		for (int c = 0; c < n_cols; ++c) out[c * n_rows + r] = (float)row.at((size_t)c).num();
	}
}
mj::Value write_vec(const float* v, size_t n) {
	mj::Value a = mj::Value::make_array();
	for (size_t i = 0; i < n; ++i) a.push(mj::Value::make_float(v[i]));
	return a;
}
mj::Value write_mat(const float* m, int n_cols, int n_rows) {
	mj::Value a = mj::Value::make_array();
	for (int r = 0; r < n_rows; ++r) {
		mj::Value row = mj::Value::make_array();
		for (int c = 0; c < n_cols; ++c) row.push(mj::Value::make_float(m[c * n_rows + r]));
		a.push(std::move(row));
	}
	return a;
}

// Lens <-> json, json_binding.h:37-93
void lens_from_json(const mj::Value& j, TrainingView& v) {
	auto num = [&](const char* k) { return (float)j.at(k).num(); };
	if (j.contains("k1")) {
		if (j.value("is_fisheye", false)) {
			v.lens_mode = NGP_LENS_OPENCV_FISHEYE;
			v.lens_params[0] = num("k1"); v.lens_params[1] = num("k2"); v.lens_params[2] = num("k3"); v.lens_params[3] = num("k4");
		} else {
			v.lens_mode = NGP_LENS_OPENCV;
			v.lens_params[0] = num("k1"); v.lens_params[1] = num("k2"); v.lens_params[2] = num("p1"); v.lens_params[3] = num("p2");
		}
	} else if (j.contains("ftheta_p0")) {
		v.lens_mode = NGP_LENS_FTHETA;
		const char* keys[7] = {"ftheta_p0", "ftheta_p1", "ftheta_p2", "ftheta_p3", "ftheta_p4", "w", "h"};
		for (int i = 0; i < 7; ++i) v.lens_params[i] = num(keys[i]);
	} else if (j.contains("latlong")) {
		v.lens_mode = NGP_LENS_LATLONG;
	} else if (j.contains("equirectangular")) {
		v.lens_mode = NGP_LENS_EQUIRECTANGULAR;
	} else {
		v.lens_mode = NGP_LENS_PERSPECTIVE;
	}
}
mj::Value lens_to_json(const TrainingView& v) {
	mj::Value j = mj::Value::make_object();
	auto put = [&](const char* k, float x) { j[k] = mj::Value::make_float(x); };
	if (v.lens_mode == NGP_LENS_OPENCV) {
		j["is_fisheye"] = mj::Value::make_bool(false);
		put("k1", v.lens_params[0]); put("k2", v.lens_params[1]); put("p1", v.lens_params[2]); put("p2", v.lens_params[3]);
	} else if (v.lens_mode == NGP_LENS_OPENCV_FISHEYE) {
		j["is_fisheye"] = mj::Value::make_bool(true);
		put("k1", v.lens_params[0]); put("k2", v.lens_params[1]); put("k3", v.lens_params[2]); put("k4", v.lens_params[3]);
	} else if (v.lens_mode == NGP_LENS_FTHETA) {
		const char* keys[7] = {"ftheta_p0", "ftheta_p1", "ftheta_p2", "ftheta_p3", "ftheta_p4", "w", "h"};
		for (int i = 0; i < 7; ++i) put(keys[i], v.lens_params[i]);
	} else if (v.lens_mode == NGP_LENS_LATLONG) {
		j["latlong"] = mj::Value::make_bool(true);
	} else if (v.lens_mode == NGP_LENS_EQUIRECTANGULAR) {
		j["equirectangular"] = mj::Value::make_bool(true);
	}
	return j;
}

void dataset_from_json(const mj::Value& j, Dataset& ds) { // json_binding.h:121-183
	const int64_t n_images = j.at("n_images").integer();
	if (n_images < 0 || !j.at("xforms").is_array() || (uint64_t)n_images != j.at("xforms").size()) throw std::runtime_error("snapshot dataset: n_images does not match the list of camera transforms");
	size_t n = (size_t)n_images;
	ds.views = std::vector<TrainingView>(n); // (value-initialised: TrainingView{} each)
	for (size_t i = 0; i < n; ++i) {
		TrainingView& v = ds.views[i];
		v.principal_point[0] = v.principal_point[1] = 0.5f;
		v.focal_length[0] = v.focal_length[1] = 1000.f;
		v.resolution[0] = v.resolution[1] = 0;
		if (j.contains("principal_point")) read_vec(j.at("principal_point"), v.principal_point, 2);
		if (j.contains("focal_length")) read_vec(j.at("focal_length"), v.focal_length, 2);
		if (j.contains("image_resolution")) { float r[2]; read_vec(j.at("image_resolution"), r, 2); v.resolution[0] = to_int(r[0]); v.resolution[1] = to_int(r[1]); }
		read_mat(j.at("xforms").at(i).at("start"), v.xform.data(), 4, 3);
		if (j.contains("metadata")) {
			const mj::Value& ji = j.at("metadata").at(i);
			float r[2];
			read_vec(ji.at("resolution"), r, 2);
			v.resolution[0] = to_int(r[0]);
			v.resolution[1] = to_int(r[1]);
			read_vec(ji.at("focal_length"), v.focal_length, 2);
			read_vec(ji.at("principal_point"), v.principal_point, 2);
			if (ji.contains("lens")) lens_from_json(ji.at("lens"), v);
		}
		if (j.contains("paths") && i < j.at("paths").size()) v.path = j.at("paths").at(i).str();
	}
	const mj::Value& ra = j.at("render_aabb");
	read_vec(ra.at("min"), ds.render_aabb_min, 3);
	read_vec(ra.at("max"), ds.render_aabb_max, 3);
	ds.has_render_aabb = true;
	if (j.contains("render_aabb_to_local")) read_mat(j.at("render_aabb_to_local"), ds.render_aabb_to_local, 3, 3);
	read_vec(j.at("up"), ds.up, 3);
	read_vec(j.at("offset"), ds.offset, 3);
	ds.scale = (float)j.at("scale").num();
	ds.aabb_scale = (int)j.at("aabb_scale").integer();
	ds.from_mitsuba = j.at("from_mitsuba").boolean();
	ds.is_hdr = j.value("is_hdr", false);
	ds.n_extra_learnable_dims = to_int(j.value("n_extra_learnable_dims", 0.0));
}

// the dataset as the snapshot describes it: with the model's aabb_scale and, unless the dataset sets one, the model's render box
mj::Value dataset_to_json(const Dataset& ds, int32_t aabb_scale, const float* render_aabb_min, const float* render_aabb_max) { // json_binding.h:94-119
	mj::Value j = mj::Value::make_object();
	j["n_images"] = mj::Value::make_uint(ds.views.size());
	mj::Value paths = mj::Value::make_array(), metadata = mj::Value::make_array(), xforms = mj::Value::make_array();
	for (auto& v : ds.views) {
		paths.push(mj::Value::make_string(v.path));
		mj::Value m = mj::Value::make_object();
		m["focal_length"] = write_vec(v.focal_length, 2);
		m["lens"] = lens_to_json(v);
		m["principal_point"] = write_vec(v.principal_point, 2);
		float rs[4] = {0, 0, 0, 0};
		m["rolling_shutter"] = write_vec(rs, 4);
		mj::Value res = mj::Value::make_array();
		res.push(mj::Value::make_int(v.resolution[0]));
		res.push(mj::Value::make_int(v.resolution[1]));
		m["resolution"] = res;
		metadata.push(std::move(m));
		mj::Value x = mj::Value::make_object();
		x["start"] = write_mat(v.xform.data(), 4, 3);
		x["end"] = write_mat(v.xform.data(), 4, 3);
		xforms.push(std::move(x));
	}
	j["paths"] = paths;
	j["metadata"] = metadata;
	j["xforms"] = xforms;
	mj::Value ra = mj::Value::make_object();
	ra["min"] = write_vec(render_aabb_min, 3);
	ra["max"] = write_vec(render_aabb_max, 3);
	j["render_aabb"] = ra;
	j["render_aabb_to_local"] = write_mat(ds.render_aabb_to_local, 3, 3);
	j["up"] = write_vec(ds.up, 3);
	j["offset"] = write_vec(ds.offset, 3);
	mj::Value er = mj::Value::make_array();
	er.push(mj::Value::make_int(0));
	er.push(mj::Value::make_int(0));
	j["envmap_resolution"] = er;
	j["scale"] = mj::Value::make_float(ds.scale);
	j["aabb_scale"] = mj::Value::make_int(aabb_scale);
	j["from_mitsuba"] = mj::Value::make_bool(ds.from_mitsuba);
	j["is_hdr"] = mj::Value::make_bool(ds.is_hdr);
	j["wants_importance_sampling"] = mj::Value::make_bool(true);
	j["n_extra_learnable_dims"] = mj::Value::make_int(ds.n_extra_learnable_dims);
	return j;
}

std::string lower(std::string t) {
	for (auto& ch : t) ch = (char)tolower(ch);
	return t;
}

// everything a snapshot file says, read and checked without a context
struct ParsedSnapshot {
	ngp_model_desc desc{}; // (params_fp16 / density_grid_fp16 stay null: commit_snapshot points them at the two vectors below)
	std::vector<uint16_t> params;
	std::vector<uint16_t> density_grid; // density_grid_binary, fp16 as stored
	Dataset dataset;
	ngp_session_state session{};
	// the "camera" block; what it leaves out keeps the context's value
	bool has_camera = false, has_matrix = false, has_relative_focal_length = false, has_screen_center = false;
	float camera[12], relative_focal_length[2], screen_center[2], zoom = 1.f;
	int32_t fov_axis = 1;
	mj::Value config; // the file without "snapshot"
};

// the position encoding's kind and, for the grids, its level parameters
void parse_encoding(const mj::Value& enc, ngp_model_desc& d) {
	const std::string otype = lower(enc.value("otype", "OneBlob"));
	// tcnn GridEncoding: HashGrid, or DenseGrid (every level x + y*res + z*res^2, never hashed, not capped by a hash-map size) --
	// the latter is the former with a hash map that no level ever fills, which is how it is carried here (log2 = 31).
	// TiledGrid wraps coordinates per axis and drops axes whose stride exceeds the tile: not implemented.
	bool dense_grid = false;
	if (otype == "densegrid") dense_grid = true;
	else if (otype == "grid") {
		const std::string gt = lower(enc.value("type", "Hash"));
		if (gt == "dense") dense_grid = true;
		else if (gt != "hash") throw std::runtime_error("unsupported grid type '" + gt + "' (Hash and Dense are implemented)");
	} else if (otype == "frequency") { // configs/nerf/frequency.json
		d.pos_encoding = 1;
		d.pos_n_frequencies = to_u32(enc.value("n_frequencies", 12.0));
	} else if (otype == "identity") { // configs/nerf/none.json: the position itself (tcnn Identity: in * scale + offset, padded with ones)
		if (enc.value("scale", 1.0) != 1.0 || enc.value("offset", 0.0) != 0.0) throw std::runtime_error("unsupported Identity encoding (scale 1, offset 0 are implemented)");
		d.pos_encoding = 2;
	} else if (otype != "hashgrid") {
		throw std::runtime_error("unsupported encoding '" + otype + "' (HashGrid, DenseGrid, Frequency and Identity are implemented)");
	}
	d.n_features_per_level = to_u32(enc.value("n_features_per_level", 2.0));
	d.n_levels = enc.contains("n_features") && enc.at("n_features").is_number() && enc.at("n_features").num() > 0 && d.n_features_per_level ? to_u32(enc.at("n_features").num()) / d.n_features_per_level
	                                                                                                                                       : to_u32(enc.value("n_levels", 16.0));
	d.log2_hashmap_size = dense_grid ? 31u : to_u32(enc.value("log2_hashmap_size", 15.0));
	d.base_resolution = to_u32(enc.value("base_resolution", 0.0));
	if (!d.base_resolution) d.base_resolution = d.log2_hashmap_size < 96u ? 1u << (d.log2_hashmap_size / 3) : 0u; // testbed.cu:3945-3949 (a larger value fails the validation below)
}

// the two MLPs' kind and the direction encoding: what the kernels hard-wire is checked, the rest goes into the descriptor
void parse_networks(const mj::Value& root, const mj::Value& net, const mj::Value& rgb, ngp_model_desc& d) {
	auto fully_fused = [](const mj::Value& n) {
		const std::string t = lower(n.value("otype", "FullyFusedMLP"));
		return t == "fullyfusedmlp" || t == "megakernelmlp" || t == "cutlassmlp";
	};
	auto is_cutlass = [](const mj::Value& n) { return lower(n.value("otype", "FullyFusedMLP")) == "cutlassmlp"; };
	if (!fully_fused(net) || !fully_fused(rgb)) throw std::runtime_error("unsupported network otype");
	// encodings and the rgb network's input / output are padded to the networks' alignment: 16 for FullyFusedMLP, 8 for CutlassMLP
	// (nerf_network.h:81-100; the rgb network's own for its output). The implemented architectures use one kind for both networks.
	if (is_cutlass(net) != is_cutlass(rgb) && d.pos_encoding >= 1) throw std::runtime_error("unsupported network otype: density and rgb networks of different kinds");
	d.mlp_alignment = is_cutlass(rgb) ? 8u : 16u; // grid models (base_0layer.json mixes the kinds): the rgb network's, nerf_network.h:83
	// what the kernels hard-wire beyond the shapes: ReLU hidden layers without an output activation, and a direction encoding of
	// SphericalHarmonics degree 4 (bare, or first in a Composite whose remainder is Identity: configs/nerf/base.json). A snapshot
	// with another choice has the same parameter count and would render silently wrong.
	for (const mj::Value* n : {&net, &rgb}) {
		if (lower(n->value("activation", "ReLU")) != "relu") throw std::runtime_error("unsupported network activation '" + n->value("activation", "ReLU") + "' (ReLU is implemented)");
		if (lower(n->value("output_activation", "None")) != "none") throw std::runtime_error("unsupported network output_activation '" + n->value("output_activation", "None") + "' (None is implemented)");
	}
	if (root.contains("dir_encoding")) {
		const mj::Value& de = root.at("dir_encoding");
		auto is_sh4 = [&](const mj::Value& e) { return lower(e.value("otype", "")) == "sphericalharmonics" && to_int(e.value("degree", 4.0)) == 4; };
		auto is_freq = [&](const mj::Value& e) { return d.pos_encoding >= 1 && lower(e.value("otype", "")) == "frequency"; };
		auto is_ident = [&](const mj::Value& e) { return d.pos_encoding >= 1 && lower(e.value("otype", "")) == "identity" && e.value("scale", 1.0) == 1.0 && e.value("offset", 0.0) == 0.0; };
		const mj::Value* first = &de;
		bool ok = is_sh4(de) || is_freq(de) || is_ident(de);
		if (!ok && lower(de.value("otype", "")) == "composite" && de.contains("nested") && de.at("nested").is_array() && de.at("nested").size() >= 1) {
			const mj::Value& nested = de.at("nested");
			first = &nested.at(0);
			ok = (is_sh4(*first) || is_freq(*first)) && (!first->contains("n_dims_to_encode") || first->at("n_dims_to_encode").integer() == 3);
			for (size_t i = 1; ok && i < nested.size(); ++i) ok = lower(nested.at(i).value("otype", "")) == "identity";
		}
		if (!ok) throw std::runtime_error("unsupported dir_encoding (SphericalHarmonics of degree 4 -- or Frequency beside a Frequency position encoding --, bare or first in a Composite with Identity for the extra dimensions, is implemented)");
		if (is_freq(*first)) {
			d.dir_encoding = 1;
			d.dir_n_frequencies = to_u32(first->value("n_frequencies", 12.0));
		} else if (first == &de && is_ident(de)) {
			d.dir_encoding = 2;
		}
	}
	d.n_neurons = (uint32_t)net.at("n_neurons").integer();
	if ((uint32_t)rgb.at("n_neurons").integer() != d.n_neurons) throw std::runtime_error("density and rgb networks must have the same width");
	d.n_hidden_density = (uint32_t)net.at("n_hidden_layers").integer();
	d.n_hidden_rgb = (uint32_t)rgb.at("n_hidden_layers").integer();
	d.density_out_dims = to_u32(net.value("n_output_dims", 16.0));
}

// Trainer::deserialize: params_binary (__half or float), then the occupancy grid's values
void parse_binaries(const mj::Value& snap, ParsedSnapshot& p) {
	const mj::Value& pb = snap.at("params_binary");
	if (pb.type != mj::Value::Binary) throw std::runtime_error("snapshot: params_binary is not binary");
	std::string ptype = snap.value("params_type", "__half");
	std::vector<uint16_t>& params = p.params;
	if (ptype == "float") {
		size_t n = pb.s.size() / 4;
		params.resize(n);
		const float* src = (const float*)pb.s.data();
		for (size_t i = 0; i < n; ++i) params[i] = float_to_half(src[i]);
	} else {
		params.resize(pb.s.size() / 2);
		memcpy(params.data(), pb.s.data(), params.size() * 2);
	}
	if (snap.contains("n_params") && (uint64_t)snap.at("n_params").integer() != params.size()) throw std::runtime_error("snapshot: n_params does not match params_binary");
	p.desc.n_params = params.size();
	const mj::Value& gb = snap.at("density_grid_binary");
	if (gb.type != mj::Value::Binary) throw std::runtime_error("snapshot: density_grid_binary is not binary");
	p.density_grid.resize(gb.s.size() / 2);
	memcpy(p.density_grid.data(), gb.s.data(), p.density_grid.size() * 2);
	p.desc.n_density_grid = p.density_grid.size();
}

// src/testbed.cu:5395-5418: the session and the camera the snapshot was saved with
void parse_session(const mj::Value& snap, ParsedSnapshot& p) {
	ngp_session_state& st = p.session;
	st.valid = 1;
	st.background_color[3] = 1.f;
	st.sun_dir[0] = st.sun_dir[1] = st.sun_dir[2] = 0.57735026f;
	st.up_dir[1] = 1.f;
	st.camera_scale = 1.5f;
	memcpy(st.up_dir, p.dataset.up, sizeof(st.up_dir));
	if (snap.contains("background_color")) read_vec(snap.at("background_color"), st.background_color, 4);
	st.exposure = (float)snap.value("exposure", 0.0);
	if (snap.contains("sun_dir")) read_vec(snap.at("sun_dir"), st.sun_dir, 3);
	if (snap.contains("up_dir")) read_vec(snap.at("up_dir"), st.up_dir, 3);
	if (!snap.contains("camera")) return;
	const mj::Value& cam = snap.at("camera");
	st.camera_scale = (float)cam.value("scale", 1.5);
	st.aperture_size = (float)cam.value("aperture_size", 0.0);
	st.autofocus_depth = (float)cam.value("autofocus_depth", 0.0);
	p.has_camera = true;
	if ((p.has_matrix = cam.contains("matrix"))) read_mat(cam.at("matrix"), p.camera, 4, 3);
	p.fov_axis = (int32_t)cam.value("fov_axis", 1.0);
	if ((p.has_relative_focal_length = cam.contains("relative_focal_length"))) read_vec(cam.at("relative_focal_length"), p.relative_focal_length, 2);
	if ((p.has_screen_center = cam.contains("screen_center"))) read_vec(cam.at("screen_center"), p.screen_center, 2);
	p.zoom = (float)cam.value("zoom", 1.0);
}

// Testbed::load_snapshot(nlohmann::json) (src/testbed.cu:5285-5463), Nerf mode, inference-relevant state
ParsedSnapshot parse_snapshot(const mj::Value& root) {
	if (!root.contains("snapshot")) throw std::runtime_error("File does not contain a snapshot.");
	const mj::Value& snap = root.at("snapshot");
	if (snap.value("version", 0.0) < 1.0) throw std::runtime_error("Snapshot uses an old format and can not be loaded.");
	const std::string mode = lower(snap.value("mode", snap.contains("nerf") ? "nerf" : "none"));
	if (mode != "nerf") throw std::runtime_error("Only NeRF snapshots are supported by this renderer (snapshot mode: " + mode + ").");
	if (snap.at("density_grid_size").integer() != (int64_t)NERF_GRIDSIZE) throw std::runtime_error("Incompatible grid size.");

	ParsedSnapshot p;
	ngp_model_desc& d = p.desc;
	Dataset& ds = p.dataset;
	const mj::Value& enc = root.at("encoding");
	const mj::Value& net = root.at("network");
	const mj::Value& rgb = root.at("rgb_network");
	parse_encoding(enc, d);

	const mj::Value& nerf = snap.at("nerf");
	if (nerf.contains("dataset")) dataset_from_json(nerf.at("dataset"), ds);
	if (nerf.contains("aabb_scale")) ds.aabb_scale = (int)nerf.at("aabb_scale").integer();
	d.aabb_scale = (uint32_t)ds.aabb_scale;

	d.per_level_scale = (float)enc.value("per_level_scale", 0.0);
	if (d.pos_encoding >= 1) {
		d.n_levels = d.n_features_per_level = d.log2_hashmap_size = d.base_resolution = 0;
		d.per_level_scale = 0.0f;
	} else if (!(d.per_level_scale > 0.0f) && d.n_levels > 1) {
		// The fork derives it from m_geometry.nerf...aabb_scale, which is 1 in Nerf mode (testbed.cu:3959-3966).
		d.per_level_scale = std::exp(std::log(2048.0f * 1.0f / (float)d.base_resolution) / (float)(d.n_levels - 1));
	}
	parse_networks(root, net, rgb, d);
	d.rgb_activation = ds.is_hdr ? NGP_ACT_EXPONENTIAL : NGP_ACT_LOGISTIC; // testbed_nerf.cu:2653
	d.density_activation = NGP_ACT_EXPONENTIAL;                           // nerf.h:151-152

	// m_aabb / m_render_aabb: load_nerf_post (testbed_nerf.cu:2720-2727), then the snapshot's own values (testbed.cu:5309,5422-5423)
	float half = 0.5f * (float)std::min<int>(1 << (NERF_CASCADES - 1), ds.aabb_scale);
	for (int i = 0; i < 3; ++i) {
		d.aabb_min[i] = 0.5f - half;
		d.aabb_max[i] = 0.5f + half;
		d.render_aabb_min[i] = d.aabb_min[i];
		d.render_aabb_max[i] = d.aabb_max[i];
	}
	for (int i = 0; i < 9; ++i) d.render_aabb_to_local[i] = ds.render_aabb_to_local[i];
	if (snap.contains("aabb")) {
		read_vec(snap.at("aabb").at("min"), d.aabb_min, 3);
		read_vec(snap.at("aabb").at("max"), d.aabb_max, 3);
	}
	if (snap.contains("render_aabb")) {
		read_vec(snap.at("render_aabb").at("min"), d.render_aabb_min, 3);
		read_vec(snap.at("render_aabb").at("max"), d.render_aabb_max, 3);
	}
	if (snap.contains("render_aabb_to_local")) read_mat(snap.at("render_aabb_to_local"), d.render_aabb_to_local, 3, 3);
	d.cone_angle_constant = ds.aabb_scale <= 1 ? 0.0f : (1.0f / 256.0f); // testbed_nerf.cu:2736
	d.linear_colors = 0;

	parse_binaries(snap, p);
	parse_session(snap, p);
	// keep the network config (without the heavy binaries) for save_snapshot
	p.config = mj::Value::make_object();
	for (auto& kv : root.obj)
		if (kv.first != "snapshot") p.config.set(kv.first, kv.second);
	return p;
}

// The model's own validation (set_model_impl) is the one step that can still refuse the file; it changes nothing when it does,
// and nothing after it throws: a refused snapshot leaves the context as it was.
void commit_snapshot(ngp_ctx* ctx, ParsedSnapshot&& p) {
	p.desc.params_fp16 = p.params.data();
	p.desc.density_grid_fp16 = p.density_grid.data();
	set_model_impl(ctx, p.desc);

	if (ctx->train) ctx->train->images_dirty = true;
	ctx->dataset = std::move(p.dataset); // (frees the training images of the dataset being replaced)
	ctx->session = p.session;
	ctx->has_snapshot_camera = p.has_matrix;
	if (p.has_matrix) memcpy(ctx->snap_camera, p.camera, sizeof(p.camera));
	if (p.has_camera) {
		ctx->snap_fov_axis = p.fov_axis;
		ctx->snap_zoom = p.zoom;
	}
	if (p.has_relative_focal_length) memcpy(ctx->snap_relative_focal_length, p.relative_focal_length, sizeof(p.relative_focal_length));
	if (p.has_screen_center) memcpy(ctx->snap_screen_center, p.screen_center, sizeof(p.screen_center));
	ctx->config = std::move(p.config);
}

void load_snapshot_bytes(ngp_ctx* ctx, const void* bytes, size_t n_bytes) { commit_snapshot(ctx, parse_snapshot(mj::MsgpackReader((const uint8_t*)bytes, n_bytes).parse())); }

// the network description of a model that came without one (ngp_set_model): the configs/nerf file of its architecture
void describe_network(const ngp_model_desc& d, mj::Value& root) {
	const bool wide = d.pos_encoding >= 1; // configs/nerf/frequency.json, none.json
	mj::Value e = mj::Value::make_object();
	if (wide) {
		e["otype"] = mj::Value::make_string(d.pos_encoding == 2 ? "Identity" : "Frequency");
		if (d.pos_encoding == 1) e["n_frequencies"] = mj::Value::make_uint(d.pos_n_frequencies);
	} else {
		e["otype"] = mj::Value::make_string(d.log2_hashmap_size == 31 ? "DenseGrid" : "HashGrid");
		e["n_levels"] = mj::Value::make_uint(d.n_levels);
		e["n_features_per_level"] = mj::Value::make_uint(d.n_features_per_level);
		if (d.log2_hashmap_size != 31) e["log2_hashmap_size"] = mj::Value::make_uint(d.log2_hashmap_size);
		e["base_resolution"] = mj::Value::make_uint(d.base_resolution);
	}
	root["encoding"] = e;
	auto mlp = [&](uint32_t hidden, bool cutlass) {
		mj::Value n = mj::Value::make_object();
		n["otype"] = mj::Value::make_string(cutlass ? "CutlassMLP" : "FullyFusedMLP");
		n["activation"] = mj::Value::make_string("ReLU");
		n["output_activation"] = mj::Value::make_string("None");
		n["n_neurons"] = mj::Value::make_uint(d.n_neurons);
		n["n_hidden_layers"] = mj::Value::make_uint(hidden);
		return n;
	};
	root["network"] = mlp(d.n_hidden_density, wide ? d.mlp_alignment == 8 : d.n_hidden_density == 0);
	root["rgb_network"] = mlp(d.n_hidden_rgb, d.mlp_alignment == 8);
	mj::Value de = mj::Value::make_object();
	if (d.dir_encoding == 1) {
		de["otype"] = mj::Value::make_string("Frequency");
		de["n_frequencies"] = mj::Value::make_uint(d.dir_n_frequencies);
	} else if (d.dir_encoding == 2) {
		de["otype"] = mj::Value::make_string("Identity");
	} else if (wide) {
		de["otype"] = mj::Value::make_string("SphericalHarmonics");
		de["degree"] = mj::Value::make_uint(4);
	} else {
		de["otype"] = mj::Value::make_string("Composite");
		mj::Value nested = mj::Value::make_array();
		mj::Value sh = mj::Value::make_object();
		sh["n_dims_to_encode"] = mj::Value::make_uint(3);
		sh["otype"] = mj::Value::make_string("SphericalHarmonics");
		sh["degree"] = mj::Value::make_uint(4);
		nested.push(sh);
		mj::Value id = mj::Value::make_object();
		id["otype"] = mj::Value::make_string("Identity");
		nested.push(id);
		de["nested"] = nested;
	}
	root["dir_encoding"] = de;
}

// what ngp_save_snapshot_file writes: the network config the model was loaded with (or its description) and "snapshot"
mj::Value build_snapshot_value(const ngp_ctx* ctx) {
	const ngp_model_desc& d = ctx->desc;
	mj::Value root = ctx->config.is_object() ? ctx->config : mj::Value::make_object();
	if (!root.contains("encoding")) describe_network(d, root);
	if (d.pos_encoding == 0) root["encoding"]["per_level_scale"] = mj::Value::make_float(d.per_level_scale);
	mj::Value snap = mj::Value::make_object();
	snap["n_params"] = mj::Value::make_uint(ctx->params.size());
	snap["params_type"] = mj::Value::make_string("__half");
	snap["params_binary"] = mj::Value::make_binary(ctx->params.data(), ctx->params.size() * 2);
	snap["version"] = mj::Value::make_uint(1);
	snap["mode"] = mj::Value::make_string("nerf");
	snap["density_grid_size"] = mj::Value::make_uint(NERF_GRIDSIZE);
	snap["density_grid_binary"] = mj::Value::make_binary(ctx->density_grid.data(), ctx->density_grid.size() * 2);
	mj::Value nerf = mj::Value::make_object();
	nerf["aabb_scale"] = mj::Value::make_uint(d.aabb_scale);
	mj::Value rgbc = mj::Value::make_object();
	rgbc["rays_per_batch"] = mj::Value::make_uint(4096);
	rgbc["measured_batch_size"] = mj::Value::make_uint(0);
	rgbc["measured_batch_size_before_compaction"] = mj::Value::make_uint(0);
	nerf["rgb"] = rgbc;
	const Dataset& ds = ctx->dataset;
	nerf["dataset"] = dataset_to_json(ds, (int)d.aabb_scale, ds.has_render_aabb ? ds.render_aabb_min : d.render_aabb_min, ds.has_render_aabb ? ds.render_aabb_max : d.render_aabb_max);
	snap["nerf"] = nerf;
	snap["training_step"] = mj::Value::make_uint(0);
	snap["loss"] = mj::Value::make_float(0.0);
	mj::Value aabb = mj::Value::make_object();
	aabb["min"] = write_vec(d.aabb_min, 3);
	aabb["max"] = write_vec(d.aabb_max, 3);
	snap["aabb"] = aabb;
	mj::Value raabb = mj::Value::make_object();
	raabb["min"] = write_vec(d.render_aabb_min, 3);
	raabb["max"] = write_vec(d.render_aabb_max, 3);
	snap["render_aabb"] = raabb;
	snap["render_aabb_to_local"] = write_mat(d.render_aabb_to_local, 3, 3);
	snap["up_dir"] = write_vec(ctx->session.valid ? ctx->session.up_dir : ctx->dataset.up, 3);
	if (ctx->session.valid) { // src/testbed.cu:5249-5251
		snap["sun_dir"] = write_vec(ctx->session.sun_dir, 3);
		snap["exposure"] = mj::Value::make_float(ctx->session.exposure);
		snap["background_color"] = write_vec(ctx->session.background_color, 4);
	}
	if (ctx->has_snapshot_camera) {
		mj::Value cam = mj::Value::make_object();
		if (ctx->session.valid) {
			cam["scale"] = mj::Value::make_float(ctx->session.camera_scale);
			cam["aperture_size"] = mj::Value::make_float(ctx->session.aperture_size);
			cam["autofocus_depth"] = mj::Value::make_float(ctx->session.autofocus_depth);
		}
		cam["matrix"] = write_mat(ctx->snap_camera, 4, 3);
		cam["fov_axis"] = mj::Value::make_int(ctx->snap_fov_axis);
		cam["relative_focal_length"] = write_vec(ctx->snap_relative_focal_length, 2);
		cam["screen_center"] = write_vec(ctx->snap_screen_center, 2);
		cam["zoom"] = mj::Value::make_float(ctx->snap_zoom);
		snap["camera"] = cam;
	}
	root["snapshot"] = snap;
	return root;
}

} // namespace

namespace ngp {
void load_snapshot_path(ngp_ctx* ctx, const std::string& p) {
	std::string data = read_file(p);
	bool compressed = ends_with_ci(p, ".ingp"); // testbed.cu:262-266
	if (!compressed && !ends_with_ci(p, ".msgpack")) throw std::runtime_error("snapshot must be a .msgpack or .ingp file");
	if (compressed) data = inflate_all(data.data(), data.size());
	load_snapshot_bytes(ctx, data.data(), data.size());
}
} // namespace ngp

// ================================================================================================== C ABI
extern "C" {

int ngp_load_snapshot(ngp_ctx* ctx, const void* bytes, size_t n_bytes, int is_compressed) {
	return guarded(ctx, [&] {
		if (!bytes || !n_bytes) throw std::runtime_error("empty snapshot");
		if (is_compressed) {
			std::string raw = inflate_all(bytes, n_bytes);
			load_snapshot_bytes(ctx, raw.data(), raw.size());
		} else {
			load_snapshot_bytes(ctx, bytes, n_bytes);
		}
	});
}

int ngp_load_snapshot_file(ngp_ctx* ctx, const char* path) {
	return guarded(ctx, [&] {
		if (!path) throw std::runtime_error("null path");
		ngp::load_snapshot_path(ctx, path);
	});
}

int ngp_save_snapshot_file(ngp_ctx* ctx, const char* path, int compress) {
	return guarded(ctx, [&] {
		if (!ctx->have_desc) throw std::runtime_error("no model to save");
		if (!path) throw std::runtime_error("null path");
		ngp::sync_host_params(ctx);
		ngp::refresh_density_grid_host(ctx);
		mj::MsgpackWriter w;
		w.write(build_snapshot_value(ctx));
		std::string p = path;
		std::ofstream f(p, std::ios::out | std::ios::binary);
		if (!f) throw std::runtime_error("cannot write '" + p + "'");
		if (ends_with_ci(p, ".ingp")) {
			std::string z = deflate_gzip(w.out, compress ? Z_DEFAULT_COMPRESSION : Z_NO_COMPRESSION);
			f.write(z.data(), (std::streamsize)z.size());
		} else {
			f.write(w.out.data(), (std::streamsize)w.out.size());
		}
	});
}

int ngp_get_session_state(const ngp_ctx* ctx, ngp_session_state* out) {
	if (!ctx || !out) return -1;
	*out = ctx->session;
	return 0;
}

int ngp_set_session_state(ngp_ctx* ctx, const ngp_session_state* state, const float* matrix12, const float* rfl2, int32_t fov_axis, const float* sc2, float zoom) {
	if (!ctx || !state) return -1;
	ctx->session = *state;
	ctx->session.valid = 1;
	if (matrix12) {
		memcpy(ctx->snap_camera, matrix12, sizeof(float) * 12);
		if (rfl2) memcpy(ctx->snap_relative_focal_length, rfl2, sizeof(float) * 2);
		if (sc2) memcpy(ctx->snap_screen_center, sc2, sizeof(float) * 2);
		ctx->snap_fov_axis = fov_axis;
		ctx->snap_zoom = zoom;
		ctx->has_snapshot_camera = true;
	}
	return 0;
}

int ngp_get_snapshot_camera(const ngp_ctx* ctx, float* matrix12, float* rfl2, int32_t* fov_axis, float* sc2, float* zoom) {
	if (!ctx || !ctx->has_snapshot_camera) return -1;
	if (matrix12) memcpy(matrix12, ctx->snap_camera, sizeof(float) * 12);
	if (rfl2) memcpy(rfl2, ctx->snap_relative_focal_length, sizeof(float) * 2);
	if (fov_axis) *fov_axis = ctx->snap_fov_axis;
	if (sc2) memcpy(sc2, ctx->snap_screen_center, sizeof(float) * 2);
	if (zoom) *zoom = ctx->snap_zoom;
	return 0;
}

} // extern "C"
