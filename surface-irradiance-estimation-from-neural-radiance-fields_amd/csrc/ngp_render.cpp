// Frames: the per-frame constants, the scheduling knobs, the context's frame buffers and the issue of a frame's work on a
// stream; page-locked host images; render statistics.
#include "ngp_host.h"

#include <map>
#include <mutex>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

using namespace ngp;

namespace {

// ------------------------------------------------------------------------------------------------ sampling (host)
// ld_random_pixel_offset (random_val.cuh:365-370) is a per-frame constant, so it is evaluated once on the host.
// Sobol dimensions 0 and 1 need no table: dim 0 is a bit reversal, dim 1's direction numbers obey v[i] = v[i-1] ^ (v[i-1] >> 1).
uint32_t reverse_bits32(uint32_t x) {
	x = ((x & 0xaaaaaaaau) >> 1) | ((x & 0x55555555u) << 1);
	x = ((x & 0xccccccccu) >> 2) | ((x & 0x33333333u) << 2);
	x = ((x & 0xf0f0f0f0u) >> 4) | ((x & 0x0f0f0f0fu) << 4);
	x = ((x & 0xff00ff00u) >> 8) | ((x & 0x00ff00ffu) << 8);
	return (x >> 16) | (x << 16);
}
uint32_t lk_perm(uint32_t x, uint32_t seed) {
	x += seed;
	x ^= x * 0x6c50b47cu;
	x ^= x * 0xb82f1e52u;
	x ^= x * 0xc7afe638u;
	x ^= x * 0x8d22f6e6u;
	return x;
}
uint32_t nus2(uint32_t x, uint32_t seed) { return reverse_bits32(lk_perm(reverse_bits32(x), seed)); }
uint32_t hash_combine(uint32_t seed, uint32_t v) { return seed ^ (v + (seed << 6) + (seed >> 2)); }
uint32_t sobol_dim(uint32_t index, int dim) {
	if (dim == 0) return reverse_bits32(index);
	uint32_t v = 0x80000000u, X = 0;
	for (int bit = 0; bit < 32; ++bit) {
		if ((index >> bit) & 1u) X ^= v;
		v ^= v >> 1;
	}
	return X;
}
void ld_random_val_2d(uint32_t index, uint32_t seed, float* out) {
	index = nus2(index, seed);
	for (int i = 0; i < 2; ++i) out[i] = (float)nus2(sobol_dim(index, i), hash_combine(seed, (uint32_t)i)) * 2.3283064365386963e-10f;
}
void ld_random_pixel_offset(uint32_t spp, float* out) {
	float a[2], b[2];
	ld_random_val_2d(0, 0xdeadbeefu, a);
	ld_random_val_2d(spp, 0xdeadbeefu, b);
	for (int i = 0; i < 2; ++i) {
		float v = (0.5f - a[i]) + b[i];
		out[i] = v - floorf(v);
	}
}

// ------------------------------------------------------------------------------------------------ frame
// The scheduling knobs of the persistent render kernel (FrameParams::tune). They never change results except
// block_jumps (0 = the reference's voxel-by-voxel walk through empty space), but values outside these ranges would
// leave a wave spinning in fused_body's loop (a refill threshold above 64 never refills, zero march steps never
// advance a ray): a GPU hang, not an error. Hence one gate for every way of setting them.
void validate_schedule(const int32_t* t, int n) {
	static const struct { const char* name; int lo, hi; } range[8] = {{"refill_min", 16, 64}, {"skip_steps", 1, 64},  {"go_min", 1, 64},      {"max_stall", 0, 64},
	                                                                  {"k_busy", 1, 8},       {"k_drain", 1, 8},      {"block_jumps", 0, 1}, {"share", 0, 1}};
	if (n < 0 || n > 8) throw std::runtime_error("schedule: at most 8 knobs");
	for (int i = 0; i < n; ++i)
		if (t[i] < range[i].lo || t[i] > range[i].hi)
			throw std::runtime_error(std::string("schedule knob ") + range[i].name + " = " + std::to_string(t[i]) + " outside [" + std::to_string(range[i].lo) + ", " + std::to_string(range[i].hi) + "]");
}

uint32_t shard_count_of(const ngp_render_opts& opts) { return opts.shard_count ? opts.shard_count : 1u; }

// What a frame of the render kernel needs beyond the camera (FrameParams), and the call's copy of the model (M arrives as ctx->M;
// a Geometry-mode frame marches the NeRF inside the meshes' box). Enqueues the clears of the diagnostic buffers on `stream`.
void make_frame_params(ngp_ctx* ctx, const ngp_camera& cam, const ngp_render_opts& opts, float* d_depth_out, int slot, int spp, hipStream_t stream, FrameParams& F, ModelParams& M) {
	const uint32_t shard_count = shard_count_of(opts);
	F.frame_buffer = ctx->d_frame.get();
	F.depth_buffer = d_depth_out ? d_depth_out : ctx->d_depth.get();
	ctx->bind_slot(F, slot); // every call has its own queue word and counters: frames on different streams may overlap
	if (shard_count > 1) F.xqueue = nullptr; // per-XCD bands pay for a whole frame (+1.4 %); a rank's interleaved share is too small for them (N = 4: -3 %, N = 8: -6 %)
	F.tiles_x = (uint32_t)(cam.width + 7) / 8;
	F.tiles_y = (uint32_t)(cam.height + 7) / 8;
	F.shard_index = opts.shard_index;
	F.shard_count = shard_count;
	F.n_local_tiles = tile_share(cam.width, cam.height, opts.shard_index, shard_count);
	F.min_transmittance = opts.min_transmittance;
	F.linear_colors = ctx->desc.linear_colors;
	F.packed = opts.packed_output ? 1 : 0;
	F.prof = nullptr;
	memcpy(F.tune, ctx->tune, sizeof(F.tune));
	if (getenv("NGP_PROFILE_SECTIONS")) { // diagnostic: per-section cycle sums of the fused kernel, printed by ngp_get_render_stats
		if (!ctx->d_prof) ctx->d_prof.reset(128);
		NGP_HIP_CHECK(hipMemsetAsync(ctx->d_prof.get(), 0, 1024, stream));
		F.prof = ctx->d_prof.get();
		F.prof_level = atoi(getenv("NGP_PROFILE_SECTIONS"));
		if (const char* e = getenv("NGP_PROFILE_TRACE")) { // timelines of every stride-th working wave (tools/wave_trace.py)
			const int stride = atoi(e);
			if (stride > 0) {
				const size_t words = 16 + (size_t)ngp_ctx::TRACE_WAVES * 16 + (size_t)ngp_ctx::TRACE_WAVES * ngp_ctx::TRACE_ITERS * 16;
				if (!ctx->d_trace) ctx->d_trace.reset(words);
				NGP_HIP_CHECK(hipMemsetAsync(ctx->d_trace.get(), 0, words * sizeof(uint32_t), stream));
				F.trace = ctx->d_trace.get();
				F.trace_stride = (uint32_t)stride;
				F.trace_cap_waves = ngp_ctx::TRACE_WAVES;
				F.trace_cap_iters = ngp_ctx::TRACE_ITERS;
			}
		}
	}
#ifdef NGP_EXPERIMENT_CELL_CACHE_STATS // counting experiment (tools/cell_cache_stats.py): the shipped kernels add their lookups and hits to prof[64 ..], over all frames
	if (!F.prof) {
		if (!ctx->d_prof) {
			ctx->d_prof.reset(128);
			NGP_HIP_CHECK(hipMemsetAsync(ctx->d_prof.get(), 0, 1024, stream));
		}
		F.prof = ctx->d_prof.get();
	}
#endif
	const bool geometry = opts.testbed_mode == NGP_MODE_GEOMETRY;
	const bool have_meshes = geometry && !ctx->meshes.empty();
	if (have_meshes && cam.has_matrix1 && memcmp(cam.matrix, cam.matrix1, sizeof(cam.matrix)) != 0) throw std::runtime_error("a moving camera (matrix1 / rolling shutter) renders NeRF mode");
	F.depth_test = geometry ? 1 : 0; // shade_kernel_nerf_geometry
	if (have_meshes) { // load_scene sets m_render_aabb to the inflated mesh bb (testbed_geometry_training.cu:3185-3189)
		for (int i = 0; i < 3; ++i) { M.raabb_min[i] = ctx->mesh_scene.scene_min[i]; M.raabb_max[i] = ctx->mesh_scene.scene_max[i]; }
		const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
		memcpy(M.r2l, ident, sizeof(ident));
		M.r2l_identity = 1u;
	}

	// 1 spp and no mesh pass: the fused kernel writes finished pixels (clear + accumulate + tonemap folded in) straight
	// into the caller's image -- one 32-byte memset and one launch per frame
	// (a rank's share in image layout keeps the general path: the other ranks' pixels must read as an empty frame)
	F.direct = (spp == 1 && !have_meshes && !geometry && (shard_count == 1 || opts.packed_output)) ? 1 : 0;
	F.to_srgb = opts.to_srgb;
	// the NeRF pass knows the grid mode as ShadeEnvMap (shaded like Shade, without its sRGB -> linear step) and ShadeIrradianceVolume, this project's own, as Shade itself
	F.render_mode = opts.render_mode == NGP_RENDER_SHADE_GRID_ENVMAP ? NGP_RENDER_SHADE_ENVMAP : opts.render_mode == NGP_RENDER_SHADE_IRRADIANCE_VOLUME ? NGP_RENDER_SHADE : opts.render_mode;
	F.color_space = opts.color_space;
	if (opts.color_space != 0 && opts.color_space != 1) throw std::runtime_error("color_space: 0 (Linear) or 1 (SRGB)");
	F.depth_scale = opts.depth_scale != 0.f ? opts.depth_scale : 1.0f / 0.33f;
	memcpy(F.background, opts.background, sizeof(F.background));
	F.exposure_scale = powf(2.0f, opts.exposure);
	if (ctx->d_bg_envmap) {
		if (geometry) throw std::runtime_error("an environment map applies to NeRF mode (in the reference the Geometry-mode NeRF pass would paint it over the meshes, src/testbed_geometry_training.cu:1993-1995): clear it with ngp_set_envmap(ctx, 0, 0, NULL)");
		F.envmap = ctx->d_bg_envmap.get();
		F.env_w = ctx->bg_env_w;
		F.env_h = ctx->bg_env_h;
	}
	{ // a render box inside the outermost cascade's cube never puts a ray outside the occupancy grid (kernel selection)
		const float h = 0.5f * (float)(1u << M.max_cascade);
		bool inside = M.r2l_identity != 0;
		for (int i = 0; i < 3; ++i) inside = inside && M.raabb_min[i] >= 0.5f - h && M.raabb_max[i] <= 0.5f + h;
		F.outside_possible = inside ? 0 : 1;
	}
}

// the shadow directions of the sample of spp index s over the sun's disk (contract: include/ngp_hip.h, "sun: the sun's disk"): formed in
// double in this order and rounded to float once. 3 n_rays floats.
void sun_disk_table(const ngp_sun_disk_desc& desc, const float* sun_dir, uint32_t s, float* out) {
	const double PI = 3.14159265358979323846;
	const double x = sun_dir[0], y = sun_dir[1], z = sun_dir[2];
	const double len = std::sqrt(x * x + y * y + z * z);
	if (!std::isfinite(len) || !(len > 0.0)) throw std::runtime_error("sun disk: the sun direction must be finite and have a length");
	const double sh[3] = {x / len, y / len, z / len};
	int a = 0;
	for (int j = 1; j < 3; ++j)
		if (std::fabs(sh[j]) < std::fabs(sh[a])) a = j;
	const double e[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
	const double c[3] = {e[1] * sh[2] - e[2] * sh[1], e[2] * sh[0] - e[0] * sh[2], e[0] * sh[1] - e[1] * sh[0]};
	const double cl = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
	const double u[3] = {c[0] / cl, c[1] / cl, c[2] / cl};
	const double v[3] = {sh[1] * u[2] - sh[2] * u[1], sh[2] * u[0] - sh[0] * u[2], sh[0] * u[1] - sh[1] * u[0]};
	const double tr = std::tan((double)desc.angular_radius);
	const double golden = PI * (3.0 - std::sqrt(5.0));
	const double turn = (double)s * 0.6180339887498949;
	const double rot = 2.0 * PI * (turn - std::floor(turn));
	const uint32_t K = desc.n_rays;
	for (uint32_t k = 0; k < K; ++k) {
		const double r = K > 1 ? std::sqrt(((double)k + 0.5) / (double)K) : 0.0;
		const double phi = (double)k * golden + rot;
		const double cp = std::cos(phi), sp = std::sin(phi), m = tr * r;
		double w[3];
		for (int j = 0; j < 3; ++j) w[j] = sh[j] + m * (cp * u[j] + sp * v[j]);
		const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
		for (int j = 0; j < 3; ++j) out[3 * k + j] = (float)(w[j] / wl);
	}
}
SunDisk sun_disk_of(const ngp_ctx* ctx, uint32_t spp_index) {
	SunDisk D{};
	D.n_rays = ctx->options.sun_disk.desc.n_rays;
	sun_disk_table(ctx->options.sun_disk.desc, ctx->shade.sun_dir, spp_index, D.d);
	return D;
}
// NGP_SUN_DISK_LAYOUT=thread: one thread a pixel loops over its rays instead of the wave dealing them over its lanes (A/B runs,
// tools/mesh_shade_rate.py --sun-disk; the same integers). Read a frame, so one process can alternate.
bool sun_disk_wave_layout() {
	const char* e = getenv("NGP_SUN_DISK_LAYOUT");
	return !e || strcmp(e, "thread") != 0;
}

// what can be refused before anything is allocated or enqueued
void validate_render_request(const ngp_ctx* ctx, const ngp_camera& cam, const ngp_render_opts& opts) {
	if (cam.width <= 0 || cam.height <= 0 || cam.width > 65536 || cam.height > 65536) throw std::runtime_error("invalid render resolution"); // (tile counts stay inside 32 bits)
	if (opts.render_mode < NGP_RENDER_SHADE || opts.render_mode > NGP_RENDER_SHADE_IRRADIANCE_VOLUME) throw std::runtime_error("render modes implemented: Shade, ShadeEnvMap, ShadeGridEnvMap, ShadeIrradianceVolume, AO, Normals, Positions, Depth, Cost");
	const bool gbuffer_mode = (opts.render_mode >= NGP_RENDER_AO && opts.render_mode <= NGP_RENDER_COST) || opts.render_mode == NGP_RENDER_NORMALS;
	if (gbuffer_mode && opts.testbed_mode == NGP_MODE_GEOMETRY) throw std::runtime_error("the G-buffer render modes (AO, Normals, Positions, Depth, Cost) apply to NeRF mode");
	if (opts.render_mode == NGP_RENDER_NORMALS && ctx->model_loaded && ctx->M.wide.width && (!ctx->M.wide.layers_t[0].n_mtiles || ctx->M.wide.enc_dims > ctx->M.wide.width))
		throw std::runtime_error("render_mode Normals on a Frequency / Identity-encoding model: implemented for up to 8 hidden density layers and an encoding no wider than the network");
	if (opts.shard_index >= shard_count_of(opts)) throw std::runtime_error("shard_index out of range");
}

} // namespace

namespace ngp {
// NGP_TUNE="refill_min,skip_steps,..." (experiments: tools/sweep_tune.sh): read ONCE, at context creation
void schedule_from_env(ngp_ctx* ctx) {
	const char* t = getenv("NGP_TUNE");
	if (!t || !*t) return;
	int32_t v[8];
	memcpy(v, ctx->tune, sizeof(v));
	int n = sscanf(t, "%d,%d,%d,%d,%d,%d,%d,%d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7]);
	if (n <= 0) throw std::runtime_error("NGP_TUNE: expected a comma-separated list of integers");
	validate_schedule(v, n);
	memcpy(ctx->tune, v, sizeof(v));
}

CameraParams make_camera_params(const ngp_camera& cam, uint32_t spp_index) {
	CameraParams C{};
	memcpy(C.m, cam.matrix, sizeof(C.m));
	C.width = cam.width;
	C.height = cam.height;
	C.focal[0] = cam.focal_length[0];
	C.focal[1] = cam.focal_length[1];
	C.screen_center[0] = cam.screen_center[0];
	C.screen_center[1] = cam.screen_center[1];
	C.spp = spp_index;
	C.near_distance = cam.near_distance;
	if (cam.lens_mode < 0 || cam.lens_mode > NGP_LENS_EQUIRECTANGULAR) throw std::runtime_error("unknown lens mode (Perspective, OpenCV, FTheta, LatLong, OpenCVFisheye, Equirectangular)");
	C.lens_mode = cam.lens_mode;
	C.aperture_size = cam.focus_z < 0.f ? 0.f : cam.aperture_size; // plane_z < 0 switches the aperture off (src/testbed_nerf.cu:1462-1464)
	C.focus_z = cam.focus_z;
	if (C.aperture_size != 0.f && !(C.focus_z > 0.f)) throw std::runtime_error("depth of field needs a positive focus distance");
	memcpy(C.lens_params, cam.lens_params, sizeof(C.lens_params));
	// camera_matrix1 + rolling shutter: a frame is "moving" only when camera1 differs from camera0 or the per-pixel time is not the
	// whole-frame constant the quaternion round trip would leave unchanged anyway
	C.moving = cam.has_matrix1 && memcmp(cam.matrix, cam.matrix1, sizeof(cam.matrix)) != 0 ? 1 : 0;
	memcpy(C.m1, cam.has_matrix1 ? cam.matrix1 : cam.matrix, sizeof(C.m1));
	memcpy(C.rolling_shutter, cam.rolling_shutter, sizeof(C.rolling_shutter));
	if (!cam.has_matrix1) { C.rolling_shutter[0] = C.rolling_shutter[1] = C.rolling_shutter[2] = 0.f; C.rolling_shutter[3] = 1.f; }
	ld_random_pixel_offset(cam.snap_to_pixel_centers ? 0u : spp_index, C.pixel_offset);
	return C;
}

void ensure_frame_buffers(ngp_ctx* ctx, size_t n_pixels) {
	if (!ctx->d_sync) {
		ctx->d_sync.reset(ngp_ctx::SLOT_BYTES * ngp_ctx::HISTORY);
		NGP_HIP_CHECK(hipMemset(ctx->d_sync.get(), 0, ngp_ctx::SLOT_BYTES * ngp_ctx::HISTORY));
		for (int i = 0; i < ngp_ctx::HISTORY; ++i) {
			ctx->ev_frame0[i] = new_event();
			ctx->ev_frame1[i] = new_event();
			ctx->ev_kern0[i] = new_event();
			ctx->ev_kern1[i] = new_event();
			ctx->ev_mesh0[i] = new_event();
			ctx->ev_mesh1[i] = new_event();
		}
	}
	if (n_pixels <= ctx->d_rgba.size()) return;
	ctx->d_frame.reset(), ctx->d_depth.reset(), ctx->d_accum.reset(), ctx->d_rgba.reset(); // all four go before the new ones come
	ctx->d_frame.reset(n_pixels);
	ctx->d_depth.reset(n_pixels);
	ctx->d_accum.reset(n_pixels);
	ctx->d_rgba.reset(n_pixels);
}

// Which passes a frame runs. The options apply to a hybrid frame -- Geometry mode, meshes and a model (always the general path) -- and all
// but the sun shadow to the four shade modes alone; the sun's disk and the materials need the meshes alone. Resolved once a call, with the
// options' refusals and buffers, before anything is enqueued; all of a frame's work then goes onto its stream and nothing waits.
struct FramePlan {
	bool have_meshes = false; // a Geometry frame with meshes: it has a mesh pass
	bool runs[N_FRAME_PASSES] = {};
	bool operator[](FramePassId pass) const { return runs[pass]; }
	// the mesh pass is split around its ray lists: G-buffer -> per list: prep -> trace -> deferred shade (the disk alone fills the shadow list without tracing it)
	bool split() const { return runs[PASS_SUN_SHADOW] || runs[PASS_REFLECTION] || runs[PASS_SUN_DISK]; }
	// the NeRF launch composites into the NeRF scratch and a kernel behind it closes the frame
	bool scratch() const { return runs[PASS_MESH_SHADOW] || runs[PASS_AMBIENT_CHANGE]; }
};

// The one rule of the passes' buffers: nothing is allocated until a frame first needs it; a group grows when a frame has more pixels than it
// holds; all of its buffers go before any new one comes (releasing device memory waits for the device: nothing goes under a frame in
// flight); and its capacity is 0 from before the release until the last allocation has succeeded, so the next frame rebuilds a group
// that an allocation failed in.
template <typename Group>
static void grow_scratch(Group& g, size_t n_pixels) {
	if (n_pixels <= g.capacity) return;
	g.capacity = 0;
	g.release();
	g.allocate(n_pixels);
	g.capacity = n_pixels;
}
static void ensure_pass_buffers(ngp_ctx* ctx, const FramePlan& plan, size_t n_pixels) {
	if (plan.split()) grow_scratch(ctx->gbuffer_scratch, n_pixels);
	if (plan[PASS_REFLECTION]) grow_scratch(ctx->reflection_scratch, n_pixels);
	if (plan[PASS_REFLECTION_HITS]) grow_scratch(ctx->reflection_hit_scratch, n_pixels);
	if (plan.scratch()) grow_scratch(ctx->nerf_scratch, n_pixels);
	for (int i = 0; i < N_FRAME_PASSES; ++i)
		if (plan.runs[i]) grow_scratch(ctx->passes[i], n_pixels);
}

static FramePlan plan_frame(ngp_ctx* ctx, const ngp_render_opts& opts, size_t n_pixels) {
	const FrameOptions& o = ctx->options;
	FramePlan p;
	p.have_meshes = opts.testbed_mode == NGP_MODE_GEOMETRY && !ctx->meshes.empty();
	const bool hybrid = p.have_meshes && ctx->model_loaded;
	const bool shade_mode = opts.render_mode == NGP_RENDER_SHADE || opts.render_mode == NGP_RENDER_SHADE_ENVMAP || opts.render_mode == NGP_RENDER_SHADE_GRID_ENVMAP ||
	                        opts.render_mode == NGP_RENDER_SHADE_IRRADIANCE_VOLUME;
	p.runs[PASS_SUN_SHADOW] = o.sun_nerf_shadow.on && hybrid;
	// (strength 0 adds nothing: no trace is run and the frame takes the path it would take with the option off)
	p.runs[PASS_REFLECTION] = o.mesh_reflection.on && o.mesh_reflection.desc.strength > 0.0f && hybrid && shade_mode;
	p.runs[PASS_REFLECTION_HITS] = p[PASS_REFLECTION] && o.mesh_reflection_meshes;
	p.runs[PASS_MESH_SHADOW] = o.mesh_shadow_on_nerf.on && hybrid && shade_mode;
	p.runs[PASS_AMBIENT_CHANGE] = o.ambient_change_on_nerf.on && hybrid && shade_mode;
	p.runs[PASS_SUN_DISK] = o.sun_disk.on && p.have_meshes;
	p.runs[PASS_MESH_IDS] = p.have_meshes && ctx->n_own_materials > 0; // some mesh owns a material: the mesh pass's material instantiations run and leave the id plane

	if (p[PASS_SUN_SHADOW]) require_probe_model(ctx, "sun_nerf_shadow frames (ngp_set_sun_nerf_shadow)");
	if (p[PASS_REFLECTION]) require_probe_model(ctx, "mesh_reflection frames (ngp_set_mesh_reflection)");
	if (p[PASS_AMBIENT_CHANGE]) {
		if (!ctx->d_sh_volume) throw std::runtime_error("ambient_change_on_nerf frames need the irradiance volume: call ngp_compute_irradiance_volume or ngp_set_irradiance_volume first");
		if (!ctx->d_sh_reference)
			throw std::runtime_error("ambient_change_on_nerf frames need the reference irradiance volume: call ngp_compute_reference_irradiance_volume or ngp_set_reference_irradiance_volume first");
		if (ctx->M.wide.width) throw std::runtime_error("ambient_change_on_nerf frames need a grid-encoded model (ngp_set_ambient_change_on_nerf)");
	}
	if (p[PASS_SUN_DISK]) (void)sun_disk_of(ctx, 0); // (a sun direction without a length is refused here, ahead of the frame's work)

	ensure_pass_buffers(ctx, p, n_pixels);
	return p;
}

// what the steps of one sample share
struct FrameCall {
	ngp_ctx* ctx;
	FramePlan plan;
	FrameLayout L;
	int slot;
	hipStream_t stream;
};

// one ray list of a sample's split mesh pass: clear, `fill` (the kernel that writes the pixels' entries), and with `trace` `before_prep`
// (what reads the list as `fill` left it: the prep step normalises d in place and moves t.x) -> prep -> trace, between the pass's events.
// The trace borrows the slot's queue ahead of the NeRF launch and reports into the list's own results.
template <typename Fill, typename BeforePrep>
static void trace_pixel_rays(const FrameCall& f, const ModelParams& M, const RayList& rays, const FramePass& pass, bool trace, float min_transmittance, bool last, Fill&& fill,
                             BeforePrep&& before_prep) {
	const uint32_t n = f.L.n_pixels;
	NGP_HIP_CHECK(hipMemsetAsync(rays.t.get(), 0, (size_t)n * sizeof(float2), f.stream)); // entries no pixel owns stay dead
	if (trace) pass.clear(n, f.stream);
	fill();
	if (!trace) return;
	pass.begin(f.slot, f.stream, last);
	before_prep();
	launch_ray_list_prep(M, n, rays.o.get(), rays.d.get(), rays.t.get(), true, f.stream);
	FrameParams FT{};
	tracer_frame_params(f.ctx, f.slot, min_transmittance, FT);
	FT.results = rays.results.get();
	if (n) launch_probe_trace(f.ctx, M, FT, ray_list_params(n, rays.o.get(), rays.d.get(), rays.t.get(), rays.traced.get(), nullptr), false, f.stream); // (a shard without tiles traces nothing)
	pass.end(f.slot, f.stream, last);
}

// the mesh pass of a sample into d_frame and the depth buffer: fused, or G-buffer -> per list: prep -> trace -> deferred shade
static void mesh_pass(const FrameCall& f, const ngp_render_opts& opts, const ModelParams& M, const CameraParams& C, const FrameParams& F, bool last) {
	ngp_ctx* ctx = f.ctx;
	IrradianceMap I{};
	if (opts.render_mode == NGP_RENDER_SHADE_ENVMAP) {
		if (!ctx->d_irradiance || ctx->env_probe.mode == 3) throw std::runtime_error("render_mode ShadeEnvMap needs ngp_compute_envmap first");
		I = irradiance_map_of(ctx);
	} else if (opts.render_mode == NGP_RENDER_SHADE_GRID_ENVMAP) {
		if (!ctx->d_irradiance || ctx->env_probe.mode != 3) throw std::runtime_error("render_mode ShadeGridEnvMap needs ngp_compute_envmap_grid first");
		I = irradiance_map_of(ctx);
	}
	IrradianceVolume V{};
	const bool volume = opts.render_mode == NGP_RENDER_SHADE_IRRADIANCE_VOLUME;
	if (volume) {
		if (!ctx->d_sh_volume) throw std::runtime_error("render_mode ShadeIrradianceVolume needs ngp_compute_irradiance_volume or ngp_set_irradiance_volume first");
		V = sh_volume_of(ctx);
	}
	const bool visible = volume && ctx->d_sh_visibility; // the held distance maps weight the probes
	const IrradianceVolumeVisible VV = visible ? sh_volume_visible_of(ctx) : IrradianceVolumeVisible{};
	// with materials the kernels select own ? table[mesh] : ctx->shade per thread and write the id plane (entries no pixel owns stay -1)
	const MeshMaterial* materials = f.plan[PASS_MESH_IDS] ? ctx->d_mesh_materials.get() : nullptr;
	int32_t* ids = f.plan[PASS_MESH_IDS] ? (int32_t*)ctx->passes[PASS_MESH_IDS].record.get() : nullptr;
	if (last) NGP_HIP_CHECK(hipEventRecord(ctx->ev_mesh0[f.slot], f.stream)); // (ngp_get_mesh_pass_ms)
	if (ids) ctx->passes[PASS_MESH_IDS].clear(f.L.n_pixels, f.stream);
	if (f.plan.split()) {
		const FrameOptions& o = ctx->options;
		const RayList& ss = ctx->gbuffer_scratch.rays;
		float4* gbuf = ctx->gbuffer_scratch.gbuf.get();
		trace_pixel_rays(f, M, ss, ctx->passes[PASS_SUN_SHADOW], f.plan[PASS_SUN_SHADOW], o.sun_nerf_shadow.desc.min_transmittance, last, [&] {
			launch_mesh_gbuffer(ctx->mesh_scene, ctx->shade, C, f.L, F.depth_buffer, o.sun_nerf_shadow.desc.t_min, gbuf, ss.o.get(), ss.d.get(), ss.t.get(), ids, f.stream);
			if (!f.plan[PASS_SUN_DISK]) return;
			const FramePass& disk = ctx->passes[PASS_SUN_DISK]; // (the kernel writes its owners' records; the clear covers the others)
			disk.clear(f.L.n_pixels, f.stream);
			disk.begin(f.slot, f.stream, last);
			launch_mesh_sun_disk(ctx->mesh_scene, C, f.L, sun_disk_of(ctx, C.spp), sun_disk_wave_layout(), o.sun_nerf_shadow.desc.t_min, gbuf, ss.o.get(), ss.t.get(), disk.f4(), f.stream);
			disk.end(f.slot, f.stream, last);
		}, [] {});
		MeshReflectionList R{};
		if (f.plan[PASS_REFLECTION]) { // the mirror rays: a list and a trace of their own behind the shadow rays', every ray traced on its own
			const RayList& mr = ctx->reflection_scratch.rays;
			const FramePass& hits = ctx->passes[PASS_REFLECTION_HITS];
			int2* hit_ids = f.plan[PASS_REFLECTION_HITS] ? ctx->reflection_hit_scratch.ids.get() : nullptr;
			trace_pixel_rays(f, M, mr, ctx->passes[PASS_REFLECTION], true, o.mesh_reflection.desc.min_transmittance, last, [&] {
				launch_mesh_reflection_rays(ctx->mesh_scene, C, f.L, o.mesh_reflection.desc.t_min, gbuf, mr.o.get(), mr.d.get(), mr.t.get(), hit_ids, f.stream);
			}, [&] {
				if (!hit_ids) return;
				hits.clear(f.L.n_pixels, f.stream); // (the kernel writes every pixel it owns; the clear covers the others)
				hits.begin(f.slot, f.stream, last);
				launch_mesh_reflection_hit_shade(ctx->mesh_scene, ctx->shade, I, volume ? &V : nullptr, visible ? &VV : nullptr, C, f.L, mr.o.get(), mr.d.get(), mr.t.get(), hit_ids,
				                                 hits.f4(), materials, f.stream);
				hits.end(f.slot, f.stream, last);
			});
			R = MeshReflectionList{mr.o.get(), mr.t.get(), mr.traced.get(), ctx->passes[PASS_REFLECTION].f4(), o.mesh_reflection.desc.strength, hit_ids ? hits.f4() : nullptr};
		}
		launch_mesh_shade_deferred(ctx->shade, I, volume ? &V : nullptr, visible ? &VV : nullptr, C, f.L, ctx->d_frame.get(), gbuf, ss.o.get(), ss.t.get(),
		                           f.plan[PASS_SUN_SHADOW] ? ss.traced.get() : nullptr, ctx->passes[PASS_SUN_SHADOW].f4(), R, materials, ids, f.stream);
	} else {
		launch_render_mesh(ctx->mesh_scene, ctx->shade, I, volume ? &V : nullptr, visible ? &VV : nullptr, C, f.L, ctx->d_frame.get(), F.depth_buffer, materials, ids, f.stream);
	}
	if (last) NGP_HIP_CHECK(hipEventRecord(ctx->ev_mesh1[f.slot], f.stream));
}

// the NeRF launch of sample s: into the frame, or with plan.scratch() over zeros into the NeRF scratch, apart from the mesh pass's pixels (its depth
// test and depth writes are every frame's)
static void nerf_pass(const FrameCall& f, const ModelParams& M, const CameraParams& C, FrameParams& F, int s, bool last) {
	ngp_ctx* ctx = f.ctx;
	if (f.plan.scratch()) {
		NGP_HIP_CHECK(hipMemsetAsync(ctx->nerf_scratch.nerf.get(), 0, (size_t)f.L.n_pixels * sizeof(float4), f.stream));
		if (f.plan[PASS_MESH_SHADOW]) ctx->passes[PASS_MESH_SHADOW].clear(f.L.n_pixels, f.stream);
		if (f.plan[PASS_AMBIENT_CHANGE]) ctx->passes[PASS_AMBIENT_CHANGE].clear(f.L.n_pixels, f.stream);
		F.frame_buffer = ctx->nerf_scratch.nerf.get();
	}
	if (last) NGP_HIP_CHECK(hipEventRecord(ctx->ev_kern0[f.slot], f.stream));
	if (ctx->model_loaded) ctx->last_render_kernel = launch_render_nerf(M, C, F, ctx->n_cus, f.stream); // persistent grid sized by the launcher
	else if (s == 0) NGP_HIP_CHECK(hipMemsetAsync(F.results, 0, 24, f.stream)); // meshes only: no NeRF launch reports counters
	if (last) NGP_HIP_CHECK(hipEventRecord(ctx->ev_kern1[f.slot], f.stream));
}

// what closes a sample whose NeRF launch went into the scratch: the scratch's colour follows the ambient light, then its composite over the
// mesh pass's pixels, scaled where a mesh stands in front of the sun (or plain: f = 1, no traversal)
static void closing_passes(const FrameCall& f, const ModelParams& M, const CameraParams& C, const FrameParams& F, bool last) {
	ngp_ctx* ctx = f.ctx;
	float4* nerf = ctx->nerf_scratch.nerf.get();
	if (f.plan[PASS_AMBIENT_CHANGE]) {
		const FramePass& pass = ctx->passes[PASS_AMBIENT_CHANGE];
		const ngp_ambient_change_desc& d = ctx->options.ambient_change_on_nerf.desc;
		pass.begin(f.slot, f.stream, last);
		launch_nerf_surface_normals(M, C, f.L, F.depth_buffer, nerf, pass.f4(), f.stream);
		launch_nerf_ambient_ratio(sh_volume_of(ctx), sh_reference_of(ctx), f.L.n_pixels, nerf, pass.f4(), d.min_irradiance, d.max_gain, f.stream);
		pass.end(f.slot, f.stream, last);
		if (!f.plan[PASS_MESH_SHADOW]) launch_nerf_composite(C, ctx->d_frame.get(), nerf, f.L, f.stream);
	}
	if (f.plan[PASS_MESH_SHADOW]) {
		const FramePass& pass = ctx->passes[PASS_MESH_SHADOW];
		const ngp_mesh_shadow_on_nerf_desc& d = ctx->options.mesh_shadow_on_nerf.desc;
		pass.begin(f.slot, f.stream, last);
		if (f.plan[PASS_SUN_DISK])
			launch_nerf_mesh_soft_shadow(ctx->mesh_scene, ctx->shade, M, C, ctx->d_frame.get(), F.depth_buffer, nerf, pass.f4(), f.L, sun_disk_of(ctx, C.spp), sun_disk_wave_layout(),
			                             d.strength, d.bias, f.stream);
		else
			launch_nerf_mesh_shadow(ctx->mesh_scene, ctx->shade, M, C, ctx->d_frame.get(), F.depth_buffer, nerf, pass.f4(), f.L, d.strength, d.bias, f.stream);
		pass.end(f.slot, f.stream, last);
	}
}

// Testbed::render_frame (src/testbed.cu:4694-4721) for opts->spp samples; the final image lands in d_rgba_out.
void render_frames(ngp_ctx* ctx, const ngp_camera& cam, const ngp_render_opts& opts, float4* d_rgba_out, float* d_depth_out, hipStream_t stream) {
	require_device(ctx, "rendering needs an MI355X");
	if (!ctx->model_loaded && !(opts.testbed_mode == NGP_MODE_GEOMETRY && !ctx->meshes.empty())) throw std::runtime_error("No network available."); // testbed.cu:4735-4738
	sync_inference_model(ctx);
	validate_render_request(ctx, cam, opts);
	// frame-buffer extent: the whole image, or only this shard's tiles in tile-packed order
	const size_t n_pixels = opts.packed_output ? (size_t)tile_share(cam.width, cam.height, opts.shard_index, shard_count_of(opts)) * 64 : (size_t)cam.width * cam.height;
	ensure_frame_buffers(ctx, n_pixels ? n_pixels : 1);
	const FramePlan plan = plan_frame(ctx, opts, n_pixels ? n_pixels : 1);
	const int spp = opts.spp > 0 ? opts.spp : 1;
	const int slot = (int)(ctx->n_calls % ngp_ctx::HISTORY);
	// Call k reuses the queue word, exit counter and accumulators of call k - HISTORY, which may have been issued on another stream and,
	// in an unsynchronised loop of short frames, may still be running: two live launches on one slot would deal tiles twice and zero
	// the slot under each other. Order this call's stream behind that frame's end (a device-side wait, no host stall; free when the
	// old frame is long done, which is the usual case).
	if (ctx->n_calls >= (uint64_t)ngp_ctx::HISTORY) NGP_HIP_CHECK(hipStreamWaitEvent(stream, ctx->ev_frame1[slot], 0));
	FrameParams F{};
	ModelParams M = ctx->M;
	make_frame_params(ctx, cam, opts, d_depth_out, slot, spp, stream, F, M);
	const FrameCall f{ctx, plan, FrameLayout{F.shard_index, F.shard_count, (uint32_t)n_pixels, F.packed}, slot, stream};

	order_after_model(ctx, stream); // a training step / grid refresh / peer copy that updated what this frame reads (a device-side wait)
	NGP_HIP_CHECK(hipEventRecord(ctx->ev_frame0[slot], stream));
	ctx->last_render_kernel = "";
	if (F.direct) {
		F.frame_buffer = d_rgba_out;
		CameraParams C = make_camera_params(cam, cam.spp_index);
		NGP_HIP_CHECK(hipEventRecord(ctx->ev_kern0[slot], stream));
		ctx->last_render_kernel = launch_render_nerf(M, C, F, ctx->n_cus, stream);
		NGP_HIP_CHECK(hipEventRecord(ctx->ev_kern1[slot], stream));
	}
	if (!F.direct && ctx->n_calls > 0 && (ctx->streams_mixed || (ctx->last_stream && ctx->last_stream != stream))) {
		// the general path goes through the context's own frame / accumulate buffers: frames on other streams must have
		// left them (only direct-output frames may overlap each other). Several may still be in flight, one event would
		// not cover them all: wait for the device.
		NGP_HIP_CHECK(hipDeviceSynchronize());
		ctx->streams_mixed = false;
	}
	if (ctx->last_stream && ctx->last_stream != stream) ctx->streams_mixed = true;
	for (int s = 0; s < spp && !F.direct; ++s) {
		CameraParams C = make_camera_params(cam, cam.spp_index + (uint32_t)s);
		// CudaRenderBufferView::clear (src/render_buffer.cu:603-607)
		NGP_HIP_CHECK(hipMemsetAsync(ctx->d_frame.get(), 0, n_pixels * sizeof(float4), stream));
		NGP_HIP_CHECK(hipMemsetAsync(F.depth_buffer, 0, n_pixels * sizeof(float), stream));
		F.add_results = s > 0 ? 1 : 0; // the call's counters are the sums over its samples per pixel
		const bool last = s == spp - 1;
		if (plan.have_meshes) mesh_pass(f, opts, M, C, F, last);
		nerf_pass(f, M, C, F, s, last);
		closing_passes(f, M, C, F, last);
		launch_accumulate_tonemap((uint32_t)n_pixels, ctx->d_frame.get(), ctx->d_accum.get(), (float)s, opts.background, opts.exposure, opts.to_srgb, opts.color_space, last ? d_rgba_out : nullptr, stream);
	}
	NGP_HIP_CHECK(hipEventRecord(ctx->ev_frame1[slot], stream));
	NGP_HIP_CHECK(hipGetLastError());
	ctx->last_stream = stream;
	ctx->hist_n_rays[slot] = (uint64_t)F.n_local_tiles * 64u * (uint64_t)spp;
	ctx->hist_mesh_pass[slot] = plan.have_meshes && !F.direct;
	for (int i = 0; i < N_FRAME_PASSES; ++i) ctx->passes[i].ran(slot, plan.runs[i], n_pixels); // (a frame with a pass has meshes: never the direct path)
	ctx->last_was_multi = false;
	++ctx->n_calls;
}
} // namespace ngp

// ================================================================================================== C ABI
namespace {
// ---- the bodies the frame options' entries share. An option's setter validates first: a refused call leaves the option as it was.
template <typename Desc>
int set_option(ngp_ctx* ctx, FrameOption<Desc> FrameOptions::*option, const Desc* desc) {
	return guarded(ctx, [&] {
		if (desc) check_desc(*desc);
		ctx->options.*option = FrameOption<Desc>{desc != nullptr, desc ? *desc : Desc{}};
	});
}
template <typename Desc>
int get_option(ngp_ctx* ctx, FrameOption<Desc> FrameOptions::*option, Desc* out, int* enabled) {
	return guarded(ctx, [&] {
		if (!out || !enabled) throw std::runtime_error("null argument");
		*out = (ctx->options.*option).desc;
		*enabled = (ctx->options.*option).on ? 1 : 0;
	});
}
// whether the context's last call was a frame that ran the pass
bool ran_last(const ngp_ctx* ctx, FramePassId pass) { return ctx->n_calls && ctx->passes[pass].hist[(ctx->n_calls - 1) % FRAME_HISTORY]; }
// the record the pass left in the last frame, n pixels of FRAME_PASSES[pass].bytes each
int read_record(ngp_ctx* ctx, FramePassId pass, void* out, size_t n) {
	return guarded(ctx, [&] {
		const FramePass& p = ctx->passes[pass];
		require_device(ctx);
		if (!out) throw std::runtime_error("null argument");
		if (!ran_last(ctx, pass)) throw std::runtime_error(p.info->none);
		if (n != p.n_pixels) throw std::runtime_error("n_pixels: the last frame had " + std::to_string(p.n_pixels) + " pixels on this device");
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		NGP_HIP_CHECK(hipMemcpy(out, p.record.get(), p.info->bytes * n, hipMemcpyDeviceToHost));
	});
}
// the pass's device time in the last frame's last sample; after a frame without the pass 0, or the record's refusal (FRAME_PASSES)
int read_ms(ngp_ctx* ctx, FramePassId pass, float* ms) {
	return guarded(ctx, [&] {
		const FramePass& p = ctx->passes[pass];
		require_device(ctx);
		const bool ran = ran_last(ctx, pass);
		if (!ran && p.info->ms == PassMs::refuses) throw std::runtime_error(p.info->none);
		if (!ms) throw std::runtime_error("null argument");
		*ms = 0.f;
		if (!ran) return;
		const int slot = (int)((ctx->n_calls - 1) % FRAME_HISTORY);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		NGP_HIP_CHECK(hipEventElapsedTime(ms, p.ev0[slot], p.ev1[slot]));
	});
}
} // namespace

extern "C" {

// ---- page-locked host images. Testbed::render_to_cpu returns a fresh numpy array per call (src/python_api.cu:124-202); a
// pageable destination makes the runtime stage the 33 MB of a 1080p frame through its own bounce buffers (1.7 ms, against
// 2.1 ms of rendering). Buffers from this pool are pinned once and recycled by size, so a binding can hand out "fresh"
// arrays that the copy engine writes directly.
namespace {
struct HostPool {
	std::mutex mu;
	std::multimap<size_t, void*> free_list;
	std::map<void*, size_t> live;
	~HostPool() { // (process exit: the runtime may already be gone; leave the pages to the OS)
	}
} g_host_pool;
constexpr size_t HOST_POOL_KEEP = 8; // buffers kept for reuse per process

// the device-side address of [host, host + bytes) if that range lies inside a live page-locked buffer of the pool, else nullptr
void* pinned_device_alias(const void* host, size_t bytes) {
	std::lock_guard<std::mutex> lock(g_host_pool.mu);
	auto it = g_host_pool.live.upper_bound(const_cast<void*>(host));
	if (it == g_host_pool.live.begin()) return nullptr;
	--it;
	const char* base = (const char*)it->first;
	if (it->second == 0 || (const char*)host < base || (const char*)host + bytes > base + it->second) return nullptr;
	void* dev = nullptr;
	if (hipHostGetDevicePointer(&dev, it->first, 0) != hipSuccess || !dev) {
		(void)hipGetLastError();
		return nullptr;
	}
	return (char*)dev + ((const char*)host - base);
}
} // namespace

void* ngp_host_alloc(size_t bytes) {
	if (bytes == 0) return nullptr;
	const size_t rounded = (bytes + 4095) & ~(size_t)4095;
	{
		std::lock_guard<std::mutex> lock(g_host_pool.mu);
		auto it = g_host_pool.free_list.find(rounded);
		if (it != g_host_pool.free_list.end()) {
			void* p = it->second;
			g_host_pool.free_list.erase(it);
			g_host_pool.live[p] = rounded;
			return p;
		}
	}
	void* p = nullptr;
	if (hipHostMalloc(&p, rounded, hipHostMallocDefault) != hipSuccess) { // no device / no pinned memory left: plain memory still works, only slower
		(void)hipGetLastError();
		p = aligned_alloc(4096, rounded);
		if (!p) return nullptr;
		std::lock_guard<std::mutex> lock(g_host_pool.mu);
		g_host_pool.live[p] = 0; // 0: malloc'ed, never pooled
		return p;
	}
	std::lock_guard<std::mutex> lock(g_host_pool.mu);
	g_host_pool.live[p] = rounded;
	return p;
}

void ngp_host_free(void* p) {
	if (!p) return;
	size_t size = 0;
	bool release = false;
	{
		std::lock_guard<std::mutex> lock(g_host_pool.mu);
		auto it = g_host_pool.live.find(p);
		if (it == g_host_pool.live.end()) return; // not ours
		size = it->second;
		g_host_pool.live.erase(it);
		if (size != 0 && g_host_pool.free_list.size() < HOST_POOL_KEEP) g_host_pool.free_list.emplace(size, p);
		else release = true;
	}
	if (!release) return;
	if (size == 0) free(p);
	else (void)hipHostFree(p);
}

int ngp_render_device(ngp_ctx* ctx, const ngp_camera* cam, const ngp_render_opts* opts, void* d_rgba, void* d_depth, void* stream) {
	return guarded(ctx, [&] {
		if (!cam || !opts || !d_rgba) throw std::runtime_error("null argument");
		if (!ctx->peers.empty() && opts->shard_count <= 1) { // a multi-device context: every device renders its tiles, device 0 assembles
			ngp::render_frames_multi(ctx, *cam, *opts, (float4*)d_rgba, (float*)d_depth, stream ? (hipStream_t)stream : ctx->stream);
			return;
		}
		render_frames(ctx, *cam, *opts, (float4*)d_rgba, (float*)d_depth, stream ? (hipStream_t)stream : ctx->stream);
	});
}

uint32_t ngp_packed_tiles(int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count) {
	if (width <= 0 || height <= 0 || shard_count == 0 || shard_index >= shard_count) return 0;
	return tile_share(width, height, shard_index, shard_count);
}

int ngp_render(ngp_ctx* ctx, const ngp_camera* cam, const ngp_render_opts* opts, float* rgba_out, float* depth_out) {
	return guarded(ctx, [&] {
		if (!cam || !opts) throw std::runtime_error("null argument");
		if (cam->width <= 0 || cam->height <= 0 || cam->width > 65536 || cam->height > 65536) throw std::runtime_error("invalid render resolution");
		if (!rgba_out) throw std::runtime_error("null argument");
		if (opts->packed_output) throw std::runtime_error("packed_output is for ngp_render_device (GPU-resident tiles); ngp_render returns images");
		require_device(ctx, "rendering needs an MI355X");
		const size_t n_pixels = (size_t)cam->width * cam->height;
		ensure_frame_buffers(ctx, n_pixels);
		// A destination from ngp_host_alloc is page-locked AND mapped into the device's address space: the image is write-only for
		// every kernel that produces it (the fused kernel's direct output, accumulate + tonemap, the multi-device tile scatter), so
		// they write it over the link while they run and no copy follows the frame -- the 33 MB of a 1080p frame would take the
		// copy engine 0.8 ms after a 2.4 ms render. NGP_HOST_DIRECT=0 restores render-then-copy (A/B measurements).
		static const bool host_direct = []() { const char* e = getenv("NGP_HOST_DIRECT"); return !e || atoi(e) != 0; }();
		float4* d_image = host_direct ? (float4*)pinned_device_alias(rgba_out, n_pixels * sizeof(float4)) : nullptr;
		float4* d_target = d_image ? d_image : ctx->d_rgba.get();
		if (!ctx->peers.empty() && opts->shard_count <= 1) ngp::render_frames_multi(ctx, *cam, *opts, d_target, ctx->d_depth.get(), ctx->stream);
		else render_frames(ctx, *cam, *opts, d_target, nullptr, ctx->stream);
		// (otherwise: one DMA at the link's rate into page-locked memory, a staged copy into ordinary memory)
		if (!d_image) NGP_HIP_CHECK(hipMemcpyAsync(rgba_out, ctx->d_rgba.get(), n_pixels * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
		if (depth_out) NGP_HIP_CHECK(hipMemcpyAsync(depth_out, ctx->d_depth.get(), n_pixels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	});
}

static void read_history_slot(ngp_ctx* ctx, uint64_t call, ngp_render_stats* out) {
	const int slot = (int)(call % ngp_ctx::HISTORY);
	unsigned long long c[4];
	NGP_HIP_CHECK(hipMemcpy(c, ctx->d_sync.get() + ngp_ctx::SLOT_BYTES * (size_t)slot + 32, sizeof(c), hipMemcpyDeviceToHost)); // the slot's results (ngp_ctx::bind_slot)
	out->kernel_device_ms = (float)((double)c[3] * 1e-5); // 100 MHz ticks
	out->n_rays = ctx->hist_n_rays[slot];
	out->n_rays_alive_after_init = c[0];
	out->n_rays_hit = c[1];
	out->n_samples = c[2];
	NGP_HIP_CHECK(hipEventElapsedTime(&out->kernel_ms, ctx->ev_kern0[slot], ctx->ev_kern1[slot]));
	NGP_HIP_CHECK(hipEventElapsedTime(&out->frame_ms, ctx->ev_frame0[slot], ctx->ev_frame1[slot]));
}

int ngp_get_mesh_pass_ms(ngp_ctx* ctx, float* ms_out) {
	return guarded(ctx, [&] {
		if (!ms_out) throw std::runtime_error("null argument");
		if (!ctx->n_calls) throw std::runtime_error("nothing rendered yet");
		const int slot = (int)((ctx->n_calls - 1) % ngp_ctx::HISTORY);
		if (!ctx->hist_mesh_pass[slot]) throw std::runtime_error("the last frame had no mesh pass");
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		NGP_HIP_CHECK(hipEventElapsedTime(ms_out, ctx->ev_mesh0[slot], ctx->ev_mesh1[slot]));
	});
}

// ---- the frame options' settings (FrameOptions, ngp_host.h)
int ngp_set_sun_nerf_shadow(ngp_ctx* ctx, const ngp_irradiance_sun_nerf_desc* nerf) { return set_option(ctx, &FrameOptions::sun_nerf_shadow, nerf); }
int ngp_get_sun_nerf_shadow(ngp_ctx* ctx, ngp_irradiance_sun_nerf_desc* out, int* enabled) { return get_option(ctx, &FrameOptions::sun_nerf_shadow, out, enabled); }
int ngp_set_mesh_reflection(ngp_ctx* ctx, const ngp_mesh_reflection_desc* desc) { return set_option(ctx, &FrameOptions::mesh_reflection, desc); }
int ngp_get_mesh_reflection(ngp_ctx* ctx, ngp_mesh_reflection_desc* out, int* enabled) { return get_option(ctx, &FrameOptions::mesh_reflection, out, enabled); }
int ngp_set_mesh_shadow_on_nerf(ngp_ctx* ctx, const ngp_mesh_shadow_on_nerf_desc* desc) { return set_option(ctx, &FrameOptions::mesh_shadow_on_nerf, desc); }
int ngp_get_mesh_shadow_on_nerf(ngp_ctx* ctx, ngp_mesh_shadow_on_nerf_desc* out, int* enabled) { return get_option(ctx, &FrameOptions::mesh_shadow_on_nerf, out, enabled); }
int ngp_set_ambient_change_on_nerf(ngp_ctx* ctx, const ngp_ambient_change_desc* desc) { return set_option(ctx, &FrameOptions::ambient_change_on_nerf, desc); }
int ngp_get_ambient_change_on_nerf(ngp_ctx* ctx, ngp_ambient_change_desc* out, int* enabled) { return get_option(ctx, &FrameOptions::ambient_change_on_nerf, out, enabled); }
int ngp_set_sun_disk(ngp_ctx* ctx, const ngp_sun_disk_desc* desc) { return set_option(ctx, &FrameOptions::sun_disk, desc); }
int ngp_get_sun_disk(ngp_ctx* ctx, ngp_sun_disk_desc* out, int* enabled) { return get_option(ctx, &FrameOptions::sun_disk, out, enabled); }
int ngp_set_mesh_reflection_meshes(ngp_ctx* ctx, int on) {
	return guarded(ctx, [&] { ctx->options.mesh_reflection_meshes = on != 0; });
}
int ngp_get_mesh_reflection_meshes(ngp_ctx* ctx, int* on) {
	return guarded(ctx, [&] {
		if (!on) throw std::runtime_error("null argument");
		*on = ctx->options.mesh_reflection_meshes ? 1 : 0;
	});
}

int ngp_sun_disk_directions(ngp_ctx* ctx, const float* sun_dir, uint32_t spp_index, float* out) {
	return guarded(ctx, [&] {
		if (!sun_dir || !out) throw std::runtime_error("null argument");
		if (!ctx->options.sun_disk.on) throw std::runtime_error("the sun has no disk: call ngp_set_sun_disk first");
		sun_disk_table(ctx->options.sun_disk.desc, sun_dir, spp_index, out);
	});
}

// ---- what the last frame's optional passes left (FRAME_PASSES, ngp_host.h)
int ngp_get_frame_sun_disk(ngp_ctx* ctx, float* out, size_t n_pixels) { return read_record(ctx, PASS_SUN_DISK, out, n_pixels); }
int ngp_get_frame_sun_disk_ms(ngp_ctx* ctx, float* ms) { return read_ms(ctx, PASS_SUN_DISK, ms); }
int ngp_get_frame_sun_shadow(ngp_ctx* ctx, float* out, size_t n_pixels) { return read_record(ctx, PASS_SUN_SHADOW, out, n_pixels); }
int ngp_get_frame_sun_shadow_ms(ngp_ctx* ctx, float* ms) { return read_ms(ctx, PASS_SUN_SHADOW, ms); }
int ngp_get_frame_mesh_reflection(ngp_ctx* ctx, float* out, size_t n_pixels) { return read_record(ctx, PASS_REFLECTION, out, n_pixels); }
int ngp_get_frame_mesh_reflection_ms(ngp_ctx* ctx, float* ms) { return read_ms(ctx, PASS_REFLECTION, ms); }
int ngp_get_frame_mesh_reflection_hits(ngp_ctx* ctx, float* out, size_t n_pixels) { return read_record(ctx, PASS_REFLECTION_HITS, out, n_pixels); }
int ngp_get_frame_mesh_reflection_hits_ms(ngp_ctx* ctx, float* ms) { return read_ms(ctx, PASS_REFLECTION_HITS, ms); }
int ngp_get_frame_mesh_shadow(ngp_ctx* ctx, float* out, size_t n_pixels) { return read_record(ctx, PASS_MESH_SHADOW, out, n_pixels); }
int ngp_get_frame_mesh_shadow_ms(ngp_ctx* ctx, float* ms) { return read_ms(ctx, PASS_MESH_SHADOW, ms); }
int ngp_get_frame_ambient_change(ngp_ctx* ctx, float* out, size_t n_pixels) { return read_record(ctx, PASS_AMBIENT_CHANGE, out, n_pixels); }
int ngp_get_frame_ambient_change_ms(ngp_ctx* ctx, float* ms) { return read_ms(ctx, PASS_AMBIENT_CHANGE, ms); }
int ngp_get_frame_mesh_ids(ngp_ctx* ctx, int32_t* out, size_t n_pixels) { return read_record(ctx, PASS_MESH_IDS, out, n_pixels); }

int ngp_get_render_stats(ngp_ctx* ctx, ngp_render_stats* out) {
	return guarded(ctx, [&] {
		if (!out) throw std::runtime_error("null argument");
		if (!ctx->n_calls) throw std::runtime_error("nothing rendered yet");
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		read_history_slot(ctx, ctx->n_calls - 1, out);
		if (ctx->last_was_multi) { // a frame over several devices: totals over the devices' shares, the slowest share's times
			for (ngp_ctx* p : ctx->peers) {
				ngp_render_stats s{};
				DeviceGuard g(p->device);
				if (ngp_get_render_stats(p, &s) != 0) throw std::runtime_error(p->error);
				out->n_rays += s.n_rays; out->n_rays_alive_after_init += s.n_rays_alive_after_init; out->n_rays_hit += s.n_rays_hit; out->n_samples += s.n_samples;
				out->kernel_ms = std::max(out->kernel_ms, s.kernel_ms);
				out->frame_ms = std::max(out->frame_ms, s.frame_ms);
				out->kernel_device_ms = std::max(out->kernel_device_ms, s.kernel_device_ms);
			}
		}
#ifdef NGP_EXPERIMENT_CELL_CACHE_STATS
		if (ctx->d_prof) {
			unsigned long long p[128];
			NGP_HIP_CHECK(hipMemcpy(p, ctx->d_prof.get(), sizeof(p), hipMemcpyDeviceToHost));
			for (int l = 0; l < 4; ++l)
				fprintf(stderr, "[ngp cell cache] level %d lookups %llu hits with 4 / 8 / 16 sets %llu %llu %llu\n", l, p[64 + 4 * l], p[65 + 4 * l], p[66 + 4 * l], p[67 + 4 * l]);
		}
#endif
		if (ctx->d_prof && getenv("NGP_PROFILE_SECTIONS")) {
			unsigned long long p[128];
			NGP_HIP_CHECK(hipMemcpy(p, ctx->d_prof.get(), sizeof(p), hipMemcpyDeviceToHost));
			{ // wave timeline on the 100 MHz chip clock: when the tile queue ran dry, when the last wave left
				const double us = 0.01, t_first = (double)(~p[8]);
				fprintf(stderr, "[ngp timeline] kernel %.1f us | queue empty seen first at %.1f us, last at %.1f us | wave exits per 0.1 ms:", ((double)p[9] - t_first) * us,
				        ((double)(~p[10]) - t_first) * us, ((double)p[11] - t_first) * us);
				for (int b = 0; b < 48; ++b) fprintf(stderr, " %llu", p[16 + b]);
				fprintf(stderr, "\n[ngp skips] lane-steps that left an empty cell %llu, an empty 4^3 block %llu, an empty 16^3 block %llu\n", p[12], p[13], p[14]);
			}
			double tot = (double)(p[0] + p[1] + p[2] + p[3]);
			fprintf(stderr, "[ngp profile] refill %.1f%% march %.1f%% network %.1f%% composite %.1f%% | wave-iterations %llu passes %llu | cycles/iter %.0f cycles/pass(network) %.0f | skip rounds %llu lane-steps %llu (%.1f lanes/round) cycles/round %.0f\n",
			        100.0 * p[0] / tot, 100.0 * p[1] / tot, 100.0 * p[2] / tot, 100.0 * p[3] / tot, p[4], p[5], tot / (double)p[4], (double)p[2] / (double)p[5], p[6], p[7], (double)p[7] / (double)p[6], (double)p[1] / (double)p[6]);
			if (ctx->M.wide.width && p[5]) // the wide kernel's finer sections (wide_kernels.hip), cycles per network round of one workgroup
				fprintf(stderr, "[ngp wide profile] per network round: hidden layers %.0f (-) %.0f output layers %.0f | march loop %.0f decision %.0f rows+prefetch %.0f encode %.0f composite %.0f | rounds %llu network rounds %llu\n",
				        (double)p[64] / p[5], (double)p[65] / p[5], (double)p[71] / p[5], (double)p[66] / p[5], (double)p[67] / p[5], (double)p[68] / p[5], (double)p[69] / p[5], (double)p[70] / p[5], p[4], p[5]);
		}
	});
}

// diagnostic (NGP_PROFILE_SECTIONS + NGP_PROFILE_TRACE): the wave timelines of the last frame; layout in csrc/ngp_kernels.h (FrameParams::trace)
int ngp_get_profile_trace(ngp_ctx* ctx, uint32_t* out, uint64_t n_words, uint32_t* cap_waves, uint32_t* cap_iters) {
	return guarded(ctx, [&] {
		if (!ctx->d_trace) throw std::runtime_error("no wave trace: set NGP_PROFILE_SECTIONS=1|2 and NGP_PROFILE_TRACE=<stride> before rendering");
		const size_t words = 16 + (size_t)ngp_ctx::TRACE_WAVES * 16 + (size_t)ngp_ctx::TRACE_WAVES * ngp_ctx::TRACE_ITERS * 16;
		if (cap_waves) *cap_waves = ngp_ctx::TRACE_WAVES;
		if (cap_iters) *cap_iters = ngp_ctx::TRACE_ITERS;
		if (!out) return;
		NGP_HIP_CHECK(hipDeviceSynchronize());
		NGP_HIP_CHECK(hipMemcpy(out, ctx->d_trace.get(), std::min<size_t>(words, (size_t)n_words) * sizeof(uint32_t), hipMemcpyDeviceToHost));
	});
}

int ngp_set_schedule(ngp_ctx* ctx, const int32_t* knobs, int n) {
	return guarded(ctx, [&] {
		if (!knobs) throw std::runtime_error("schedule: null");
		validate_schedule(knobs, n);
		if (ctx->last_stream) NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		for (int i = 0; i < n; ++i) ctx->tune[i] = knobs[i];
	});
}

const char* ngp_last_render_kernel(ngp_ctx* ctx) { return ctx ? ctx->last_render_kernel : ""; }

int ngp_get_culled_tiles(ngp_ctx* ctx, uint64_t* out) {
	return guarded(ctx, [&] {
		if (!out) throw std::runtime_error("null argument");
		if (!ctx->n_calls) throw std::runtime_error("nothing rendered yet");
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		*out = 0;
		// only the unit kernels cull (nerf_kernels.hip tile_cull) and write the word: after any other kernel the slot holds an older frame's
		if (strncmp(ctx->last_render_kernel, "render_nerf_fused_unit", 22) != 0) return;
		const int slot = (int)((ctx->n_calls - 1) % ngp_ctx::HISTORY);
		unsigned long long c = 0;
		NGP_HIP_CHECK(hipMemcpy(&c, ctx->d_sync.get() + ngp_ctx::SLOT_BYTES * (size_t)slot + 32 + 8 * ngp::RESULT_CULLED, sizeof(c), hipMemcpyDeviceToHost));
		*out = c;
	});
}

int ngp_get_render_history(ngp_ctx* ctx, int n, ngp_render_stats* out) {
	return guarded(ctx, [&] {
		if (!out || n <= 0) throw std::runtime_error("invalid argument");
		if ((uint64_t)n > ctx->n_calls || n > ngp_ctx::HISTORY) throw std::runtime_error("history holds fewer render calls than requested");
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		for (int i = 0; i < n; ++i) read_history_slot(ctx, ctx->n_calls - (uint64_t)n + (uint64_t)i, &out[i]);
	});
}

int ngp_set_envmap(ngp_ctx* ctx, int32_t width, int32_t height, const float* rgba) {
	return guarded(ctx, [&] {
		if (ctx->device < 0) throw std::runtime_error("this context has no HIP device (host-only)");
		NGP_HIP_CHECK(hipDeviceSynchronize()); // frames in flight read the map
		ctx->d_bg_envmap.reset();
		ctx->bg_env_w = ctx->bg_env_h = 0;
		if (!rgba || width <= 0 || height <= 0) return;
		if ((int64_t)width * height > (1ll << 28)) throw std::runtime_error("environment map too large");
		ctx->d_bg_envmap.upload((const float4*)rgba, (size_t)width * height);
		ctx->bg_env_w = width;
		ctx->bg_env_h = height;
		for (ngp_ctx* p : ctx->peers) { // the replicas of a multi-device context see the same background
			DeviceGuard g(p->device);
			if (ngp_set_envmap(p, width, height, rgba) != 0) throw std::runtime_error(p->error);
		}
	});
}

} // extern "C"
