// transforms.json datasets (camera metadata; ngp_train.cpp decodes the images) and what the ABI reports about them.
#include "ngp_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <dirent.h>

using namespace ngp;

namespace {

// ------------------------------------------------------------------------------------------------ transforms.json
// SI::natural::compare (dependencies/NaturalSort): digit runs compare by value
bool natural_less(const std::string& a, const std::string& b) {
	size_t i = 0, j = 0;
	while (i < a.size() && j < b.size()) {
		if (isdigit((unsigned char)a[i]) && isdigit((unsigned char)b[j])) {
			size_t i0 = i, j0 = j;
			while (i0 < a.size() && a[i0] == '0') ++i0;
			while (j0 < b.size() && b[j0] == '0') ++j0;
			size_t i1 = i0, j1 = j0;
			while (i1 < a.size() && isdigit((unsigned char)a[i1])) ++i1;
			while (j1 < b.size() && isdigit((unsigned char)b[j1])) ++j1;
			if (i1 - i0 != j1 - j0) return (i1 - i0) < (j1 - j0);
			int c = a.compare(i0, i1 - i0, b, j0, j1 - j0);
			if (c != 0) return c < 0;
			i = i1;
			j = j1;
		} else {
			if (a[i] != b[j]) return a[i] < b[j];
			++i;
			++j;
		}
	}
	return a.size() - i < b.size() - j;
}

float fov_to_focal_length(int resolution, float degrees) { return 0.5f * (float)resolution / tanf(0.5f * degrees * 3.14159265358979323846f / 180.0f); }

bool read_focal_length(const mj::Value& json, float* fl, const int* res) { // nerf_loader.cu:243-271
	auto read = [&](int resolution, const std::string& axis) -> float {
		if (json.contains(axis + "_fov")) return fov_to_focal_length(resolution, (float)json.at(axis + "_fov").num());
		if (json.contains("fl_" + axis)) return (float)json.at("fl_" + axis).num();
		if (json.contains("camera_angle_" + axis)) return fov_to_focal_length(resolution, (float)json.at("camera_angle_" + axis).num() * 180 / 3.14159265358979323846f);
		return 0.0f;
	};
	float x_fl = read(res[0], "x"), y_fl = read(res[1], "y");
	if (x_fl != 0) {
		fl[0] = fl[1] = x_fl;
		if (y_fl != 0) fl[1] = y_fl;
	} else if (y_fl != 0) {
		fl[0] = fl[1] = y_fl;
	} else {
		return false;
	}
	return true;
}

// NerfDataset::nerf_matrix_to_ngp (nerf_loader.h:101-120); m column-major 4x3 in place
void nerf_matrix_to_ngp(const Dataset& ds, float* m) {
	for (int r = 0; r < 3; ++r) {
		m[3 + r] *= -1.f;
		m[6 + r] *= -1.f;
		m[9 + r] = m[9 + r] * ds.scale + ds.offset[r];
	}
	if (ds.from_mitsuba) {
		for (int r = 0; r < 3; ++r) { m[0 + r] *= -1.f; m[6 + r] *= -1.f; }
	} else {
		for (int c = 0; c < 4; ++c) { // cycle rows xyz <- yzx
			float t = m[c * 3 + 0];
			m[c * 3 + 0] = m[c * 3 + 1];
			m[c * 3 + 1] = m[c * 3 + 2];
			m[c * 3 + 2] = t;
		}
	}
}

// ngp::load_nerf (src/nerf_loader.cu:273-743), camera metadata only: images are not decoded on the inference path,
// so per-view resolution comes from the json's "w"/"h".
void load_training_data_impl(ngp_ctx* ctx, const std::string& path) {
	std::vector<std::string> json_paths;
	if (is_directory(path)) {
		DIR* dir = opendir(path.c_str());
		if (!dir) throw std::runtime_error("cannot open directory '" + path + "'");
		while (dirent* e = readdir(dir)) {
			std::string name = e->d_name;
			if (ends_with_ci(name, ".json")) json_paths.push_back(path + "/" + name);
		}
		closedir(dir);
		std::sort(json_paths.begin(), json_paths.end());
	} else if (ends_with_ci(path, ".json")) {
		json_paths.push_back(path);
	} else {
		throw std::runtime_error("NeRF data path must either be a json file or a directory containing json files.");
	}
	if (json_paths.empty()) throw std::runtime_error("Cannot load NeRF data from an empty set of paths.");

	Dataset ds;
	ds.scale = 0.33f; // NERF_SCALE, nerf_loader.h:29
	ds.offset[0] = ds.offset[1] = ds.offset[2] = 0.5f;
	for (const std::string& jp : json_paths) {
		mj::Value json = mj::parse_json(read_file(jp));
		if (!json.contains("frames") || !json.at("frames").is_array()) continue;
		const std::string base = parent_dir(jp);
		std::vector<mj::Value> frames = json.at("frames").arr;
		std::stable_sort(frames.begin(), frames.end(), [](const mj::Value& a, const mj::Value& b) { return natural_less(a.at("file_path").str(), b.at("file_path").str()); });
		if (json.contains("n_frames")) frames.resize(std::min(frames.size(), (size_t)json.at("n_frames").integer()));
		auto resolve = [&](const std::string& local) {
			std::string p = (!local.empty() && local[0] == '/') ? local : base + "/" + local;
			if (p.find_last_of('.') == std::string::npos || p.find_last_of('.') < p.find_last_of('/')) {
				for (const char* ext : {"png", "jpg", "jpeg", "bmp", "gif", "tga", "pic", "pnm", "psd", "exr"})
					if (file_exists(p + "." + ext)) return p + "." + ext;
			}
			return p;
		};
		if (!frames.empty() && frames[0].contains("sharpness")) { // blurry / missing frames are dropped, nerf_loader.cu:364-388
			float thresh = (float)json.value("sharpness_discard_threshold", 0.0);
			std::vector<mj::Value> kept;
			for (int i = 0; i < (int)frames.size(); ++i) {
				float mean = 0.f;
				int s = std::max(0, i - 3), e = std::min(i + 3, (int)frames.size() - 1);
				for (int j = s; j < e; ++j) mean += (float)frames[j].value("sharpness", 1.0);
				mean /= (float)(e - s);
				if (file_exists(resolve(frames[i].at("file_path").str())) && (float)frames[i].value("sharpness", 1.0) > thresh * mean) kept.push_back(frames[i]);
			}
			frames.swap(kept);
		}
		if (json.contains("normal_mts_args")) ds.from_mitsuba = true;
		if (ds.from_mitsuba) { ds.scale = 0.66f; ds.offset[0] = ds.offset[1] = ds.offset[2] = 0.25f * ds.scale; }
		if (json.contains("render_aabb")) {
			read_vec(json.at("render_aabb").at(0), ds.render_aabb_min, 3);
			read_vec(json.at("render_aabb").at(1), ds.render_aabb_max, 3);
			ds.has_render_aabb = true;
		}
		if (json.contains("scale")) ds.scale = (float)json.at("scale").num();
		if (json.contains("n_extra_learnable_dims")) ds.n_extra_learnable_dims = (int)json.at("n_extra_learnable_dims").integer();
		if (json.contains("aabb_scale")) ds.aabb_scale = (int)json.at("aabb_scale").integer();
		if (json.contains("offset")) {
			const mj::Value& o = json.at("offset");
			if (o.is_array()) read_vec(o, ds.offset, 3);
			else ds.offset[0] = ds.offset[1] = ds.offset[2] = (float)o.num();
		}
		if (json.contains("aabb")) { // nerf_loader.cu:503-509
			const mj::Value& a = json.at("aabb");
			float lo[3], hi[3];
			read_vec(a.at(0), lo, 3);
			read_vec(a.at(1), hi, 3);
			float len = std::max(0.000001f, std::max(std::max(std::abs(hi[0] - lo[0]), std::abs(hi[1] - lo[1])), std::abs(hi[2] - lo[2])));
			ds.scale = 1.f / len;
			for (int i = 0; i < 3; ++i) ds.offset[i] = ((hi[i] + lo[i]) * 0.5f) * -ds.scale + 0.5f;
		}
		if (json.contains("up")) {
			ds.up[0] = (float)json.at("up").at(1).num();
			ds.up[1] = (float)json.at("up").at(2).num();
			ds.up[2] = (float)json.at("up").at(0).num();
		}
		float pp[2] = {0.5f, 0.5f};
		auto read_pp = [](const mj::Value& j, float* pp) {
			if (j.contains("cx")) pp[0] = (float)j.at("cx").num() / (float)j.at("w").num();
			if (j.contains("cy")) pp[1] = (float)j.at("cy").num() / (float)j.at("h").num();
		};
		read_pp(json, pp);
		// read_lens (src/nerf_loader.cu:175-240): OpenCV parameters switch the mode on when one of them is non-zero; an
		// outer (file-level) lens is kept unless the frame names its own
		auto read_lens = [](const mj::Value& j, TrainingView& v) {
			int mode = NGP_LENS_PERSPECTIVE;
			const int opencv_mode = j.value("is_fisheye", false) ? NGP_LENS_OPENCV_FISHEYE : NGP_LENS_OPENCV;
			auto rd = [&](const char* name, int idx) {
				if (j.contains(name)) {
					v.lens_params[idx] = (float)j.at(name).num();
					if (v.lens_params[idx] != 0.f) mode = opencv_mode;
				}
			};
			rd("k1", 0); rd("k2", 1); rd("k3", 2); rd("k4", 3);
			rd("p1", 2); rd("p2", 3);
			if (j.contains("ftheta_p0")) {
				const char* keys[7] = {"ftheta_p0", "ftheta_p1", "ftheta_p2", "ftheta_p3", "ftheta_p4", "w", "h"};
				for (int i = 0; i < 7; ++i) v.lens_params[i] = (float)j.at(keys[i]).num();
				mode = NGP_LENS_FTHETA;
			}
			if (j.contains("latlong")) mode = NGP_LENS_LATLONG;
			if (j.contains("equirectangular")) mode = NGP_LENS_EQUIRECTANGULAR;
			if (mode != NGP_LENS_PERSPECTIVE) v.lens_mode = mode;
		};
		TrainingView file_lens;
		read_lens(json, file_lens);
		for (const mj::Value& frame : frames) {
			TrainingView v;
			v.lens_mode = file_lens.lens_mode;
			memcpy(v.lens_params, file_lens.lens_params, sizeof(v.lens_params));
			read_lens(frame, v);
			v.path = frame.at("file_path").str();
			std::replace(v.path.begin(), v.path.end(), '\\', '/');
			v.abs_path = resolve(v.path);
			v.white_transparent = json.value("white_transparent", false);
			v.black_transparent = json.value("black_transparent", false);
			v.resolution[0] = to_int(frame.contains("w") ? frame.at("w").num() : json.value("w", 0.0));
			v.resolution[1] = to_int(frame.contains("h") ? frame.at("h").num() : json.value("h", 0.0));
			if ((v.resolution[0] <= 0 || v.resolution[1] <= 0) && !probe_image_size(v.abs_path, v.resolution[0], v.resolution[1]))
				throw std::runtime_error("transforms.json gives no 'w' / 'h' and the resolution of '" + v.abs_path + "' cannot be read (PNG or JPEG expected)");
			v.focal_length[0] = v.focal_length[1] = 1000.f;
			bool got = read_focal_length(json, v.focal_length, v.resolution);
			got |= read_focal_length(frame, v.focal_length, v.resolution);
			if (!got) throw std::runtime_error("Couldn't read fov.");
			const mj::Value& mat = frame.contains("transform_matrix_start") ? frame.at("transform_matrix_start") : frame.at("transform_matrix");
			for (int m = 0; m < 3; ++m)
				for (int n = 0; n < 4; ++n) v.xform[(size_t)n * 3 + m] = (float)mat.at((size_t)m).at((size_t)n).num();
			v.principal_point[0] = pp[0];
			v.principal_point[1] = pp[1];
			read_pp(frame, v.principal_point);
			nerf_matrix_to_ngp(ds, v.xform.data());
			ds.views.push_back(std::move(v));
		}
	}
	if (ctx->train) ctx->train->images_dirty = true;
	ctx->dataset = std::move(ds); // (frees the training images of the dataset being replaced)
	ctx->data_path = path;
}

} // namespace

// ================================================================================================== C ABI
extern "C" {

int ngp_load_training_data(ngp_ctx* ctx, const char* path) {
	if (!ctx) return -1;
	try { // needs no device
		if (!path) throw std::runtime_error("null path");
		load_training_data_impl(ctx, path);
		ctx->error.clear();
		return 0;
	} catch (const std::exception& e) {
		ctx->error = e.what();
		return -1;
	}
}

int ngp_get_training_view_lens(const ngp_ctx* ctx, int view, int32_t* lens_mode, float* lens_params7) {
	if (!ctx || view < 0 || (size_t)view >= ctx->dataset.views.size()) return 1;
	const TrainingView& v = ctx->dataset.views[(size_t)view];
	if (lens_mode) *lens_mode = v.lens_mode;
	if (lens_params7) memcpy(lens_params7, v.lens_params, sizeof(v.lens_params));
	return 0;
}

int ngp_n_training_views(const ngp_ctx* ctx) { return ctx ? (int)ctx->dataset.views.size() : -1; }

int ngp_get_training_view(const ngp_ctx* ctx, int view, float* matrix12, int32_t* res2, float* fl2, float* pp2) {
	if (!ctx || view < 0 || view >= (int)ctx->dataset.views.size()) return -1;
	const TrainingView& v = ctx->dataset.views[(size_t)view];
	if (matrix12) memcpy(matrix12, v.xform.data(), sizeof(float) * 12);
	if (res2) { res2[0] = v.resolution[0]; res2[1] = v.resolution[1]; }
	if (fl2) { fl2[0] = v.focal_length[0]; fl2[1] = v.focal_length[1]; }
	if (pp2) { pp2[0] = v.principal_point[0]; pp2[1] = v.principal_point[1]; }
	return 0;
}

int ngp_get_dataset_info(const ngp_ctx* ctx, int32_t* aabb_scale, float* scale, float* offset3, int32_t* is_hdr) {
	if (!ctx) return -1;
	if (aabb_scale) *aabb_scale = ctx->dataset.aabb_scale;
	if (scale) *scale = ctx->dataset.scale;
	if (offset3) memcpy(offset3, ctx->dataset.offset, sizeof(float) * 3);
	if (is_hdr) *is_hdr = ctx->dataset.is_hdr ? 1 : 0;
	return 0;
}

} // extern "C"
