// Irradiance, host side of the C ABI (contract: include/ngp_hip.h): envmap probes and their E(n) tables, caller rays and traced E(p, n)
// through the ray-list tracer, SH9 irradiance volumes, probe visibility, the sun pass and the diffuse bounce passes. What the generations share is
// written once, up here: one tracer call, one whole-probe chunk loop, one ray download, a point lookup in each of its two forms, one check of each kind.
#include "ngp_host.h"
#include "sh9.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

using namespace ngp;

namespace ngp {
// the models the probe tracer serves: base.json's heads and the Frequency architecture (`what` names the caller's work in the refusal)
void require_probe_model(ngp_ctx* ctx, const char* what) {
	require_model(ctx);
	sync_inference_model(ctx);
	if (ctx->M.rgb_mid != 1 && !ctx->M.wide.width) throw std::runtime_error(std::string(what) + " are built for the configs/nerf/base.json rgb head (2 hidden layers)");
	ensure_frame_buffers(ctx, 0);
}
// what a tracer launch on history slot `slot` needs of FrameParams: the slot's queue and counters, one shard, the call's transmittance floor
void tracer_frame_params(const ngp_ctx* ctx, int slot, float min_transmittance, FrameParams& F) {
	ctx->bind_slot(F, slot);
	F.shard_index = 0;
	F.shard_count = 1;
	F.min_transmittance = min_transmittance > 0.f ? min_transmittance : 0.01f;
	F.linear_colors = ctx->desc.linear_colors;
	memcpy(F.tune, ctx->tune, sizeof(F.tune));
}
// n caller rays (o, dir, t as launch_ray_list_prep left them) into rgba and depth (nullable)
ProbeParams ray_list_params(uint32_t n, const float* o, const float* dir, const float2* t, float4* rgba, float* depth) {
	ProbeParams P{};
	P.mode = PROBE_RAY_LIST;
	P.n_rays = n;
	P.ray_o = o;
	P.ray_d = dir;
	P.ray_t = t;
	P.ray_rgba = rgba;
	P.ray_depth = depth;
	return P;
}
// one persistent launch over the P.n_rays rays of P (its ray_rgba and ray_depth are cleared here); add_results: the launch's counters
// are added to F.results instead of replacing them. Nothing here waits: a frame puts it on its own stream.
void launch_probe_trace(const ngp_ctx* ctx, const ModelParams& M, FrameParams& F, const ProbeParams& P, bool add_results, hipStream_t stream) {
	NGP_HIP_CHECK(hipMemsetAsync(P.ray_rgba, 0, (size_t)P.n_rays * sizeof(float4), stream));
	if (P.ray_depth) NGP_HIP_CHECK(hipMemsetAsync(P.ray_depth, 0, (size_t)P.n_rays * sizeof(float), stream));
	F.n_local_tiles = (P.n_rays + 63) / 64;
	F.add_results = add_results ? 1 : 0;
	launch_trace_probe(M, F, P, ctx->n_cus, stream);
}
} // namespace ngp

namespace {
// rays per tracer launch: bounds the ray-list workspace (48 B a ray). Every ray is traced on its own, so chunking changes no result.
constexpr uint32_t RAY_CHUNK = 1u << 21;
constexpr uint64_t MAX_TRACED_RAYS = 1ull << 28;
constexpr uint32_t SH_FLOAT4 = 7; // an SH9 record: 28 floats
constexpr uint32_t MAX_BOUNCES = 16;

// ------------------------------------------------------------------------------------------------ the tracer
// the model as probe rays see it: in Geometry mode load_scene made the inflated mesh box the render box (testbed_geometry_training.cu:3185-3189)
ModelParams probe_model(const ngp_ctx* ctx) {
	ModelParams M = ctx->M;
	if (!ctx->meshes.empty()) {
		for (int i = 0; i < 3; ++i) { M.raabb_min[i] = ctx->mesh_scene.scene_min[i]; M.raabb_max[i] = ctx->mesh_scene.scene_max[i]; }
		const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
		memcpy(M.r2l, ident, sizeof(ident));
		M.r2l_identity = 1u;
	}
	return M;
}

// the launches of one call of a tracer entry: one history slot, reported by ngp_get_render_stats (a ray-list entry's chunks' counters and
// device ticks add up; kernel_ms spans the first chunk's trace to the last one's). The slot is taken as render_frames takes it
// (ngp_render.cpp); unlike a frame, a call ends synchronised.
class TracerCall {
public:
	TracerCall(ngp_ctx* ctx, uint64_t n_rays, float min_transmittance) : ctx_(ctx), n_rays_(n_rays) {
		stream_ = ctx->stream;
		if (ctx->last_stream && ctx->last_stream != stream_) NGP_HIP_CHECK(hipStreamSynchronize(ctx->last_stream));
		slot_ = (int)(ctx->n_calls % ngp_ctx::HISTORY);
		if (ctx->n_calls >= (uint64_t)ngp_ctx::HISTORY) NGP_HIP_CHECK(hipStreamWaitEvent(stream_, ctx->ev_frame1[slot_], 0)); // the slot's previous launch
		tracer_frame_params(ctx, slot_, min_transmittance, F_);
		M_ = probe_model(ctx);
		NGP_HIP_CHECK(hipEventRecord(ctx->ev_frame0[slot_], stream_));
	}
	const ModelParams& model() const { return M_; }
	// one persistent launch over the P.n_rays rays of P (launch_probe_trace); the call's launches add up in its slot
	void trace(const ProbeParams& P) {
		if (!traced_) NGP_HIP_CHECK(hipEventRecord(ctx_->ev_kern0[slot_], stream_));
		launch_probe_trace(ctx_, M_, F_, P, traced_, stream_);
		NGP_HIP_CHECK(hipEventRecord(ctx_->ev_kern1[slot_], stream_));
		traced_ = true;
	}
	// n caller rays (o, dir, t as launch_ray_list_prep left them) into rgba and depth (nullable)
	void trace_rays(uint32_t n, const float* o, const float* dir, const float2* t, float4* rgba, float* depth = nullptr) { trace(ray_list_params(n, o, dir, t, rgba, depth)); }
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
	FrameParams F_{};
	ModelParams M_{};
};

// ------------------------------------------------------------------------------------------------ copies
void download(ngp_ctx* ctx, void* dst, const void* src, size_t bytes) {
	NGP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}
void upload(ngp_ctx* ctx, void* dst, const void* src, size_t bytes) {
	NGP_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
}
// rays [r0, r0 + m) of a *_rays entry, as a generator left them in o, dir, t: origins, directions and t.y = t_max
void download_rays(ngp_ctx* ctx, uint64_t r0, uint32_t m, const float* o, const float* dir, const float2* t, std::vector<float2>& t_host, float* origins_out,
                   float* directions_out, float* t_max_out) {
	download(ctx, origins_out + 3 * r0, o, (size_t)m * 3 * sizeof(float));
	download(ctx, directions_out + 3 * r0, dir, (size_t)m * 3 * sizeof(float));
	download(ctx, t_host.data(), t, (size_t)m * sizeof(float2));
	for (uint32_t i = 0; i < m; ++i) t_max_out[r0 + i] = t_host[i].y;
}
// E at n points, the two forms the lookup entries come in; launch(d_positions, d_normals, d_out) runs on the context's stream.
// The envmap entries: blocking uploads (positions nullable: a lookup by normal alone), 3 floats a point out
template <typename L>
void lookup_rgb(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, float* rgb_out, L&& launch) {
	DevArray<float> d_p, d_n;
	if (positions) d_p.upload(positions, (size_t)n * 3);
	d_n.upload(normals, (size_t)n * 3);
	DevArray<float4> d_o(n);
	launch(d_p.get(), d_n.get(), d_o.get());
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	std::vector<float4> tmp(n);
	NGP_HIP_CHECK(hipMemcpy(tmp.data(), d_o.get(), (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
	for (uint32_t i = 0; i < n; ++i) { rgb_out[3 * i] = tmp[i].x; rgb_out[3 * i + 1] = tmp[i].y; rgb_out[3 * i + 2] = tmp[i].z; }
	NGP_HIP_CHECK(hipGetLastError());
}
// The volume entries: everything on the stream, 4 floats a point out (E and the weight)
template <typename L>
void lookup_rgbw(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, float* out, L&& launch) {
	DevArray<float> d_p(3 * (size_t)n), d_n(3 * (size_t)n);
	DevArray<float4> d_o(n);
	upload(ctx, d_p.get(), positions, (size_t)n * 3 * sizeof(float));
	upload(ctx, d_n.get(), normals, (size_t)n * 3 * sizeof(float));
	launch(d_p.get(), d_n.get(), d_o.get());
	download(ctx, out, d_o.get(), (size_t)n * sizeof(float4));
	NGP_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ checks
bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
bool nonzero3(const float* p) { return p[0] != 0.0f || p[1] != 0.0f || p[2] != 0.0f; }

// (the refusals stand out of line: with the strings built in place the compiler kept these two as calls, a million a lookup)
[[noreturn]] void refuse_position(uint32_t i) { throw std::runtime_error("position " + std::to_string(i) + " is not finite"); }
[[noreturn]] void refuse_normal(uint32_t i) { throw std::runtime_error("normal " + std::to_string(i) + " is zero or not finite"); }
inline void check_position(const float* positions, uint32_t i) {
	if (!finite3(positions + 3 * (size_t)i)) refuse_position(i);
}
inline void check_normal(const float* normals, uint32_t i) {
	if (!finite3(normals + 3 * (size_t)i) || !nonzero3(normals + 3 * (size_t)i)) refuse_normal(i);
}
void check_positions(uint32_t n, const float* positions) {
	if (n && !positions) throw std::runtime_error("null argument");
	for (uint32_t i = 0; i < n; ++i) check_position(positions, i);
}
void check_normals(uint32_t n, const float* normals) {
	for (uint32_t i = 0; i < n; ++i) check_normal(normals, i);
}

// the points' checks shared by ngp_irradiance_rays and ngp_irradiance_traced (point by point: its position, then its normal); returns K
uint32_t check_irradiance_request(uint32_t n, const float* positions, const float* normals, const ngp_irradiance_trace_desc* d) {
	if (!d) throw std::runtime_error("null argument");
	if (d->n_u == 0 || d->n_v == 0) throw std::runtime_error("invalid irradiance descriptor: n_u and n_v must be at least 1");
	if (!std::isfinite(d->offset) || d->offset < 0.0f) throw std::runtime_error("invalid irradiance descriptor: offset must be finite and >= 0");
	const uint64_t K = (uint64_t)d->n_u * d->n_v;
	if (K * n > MAX_TRACED_RAYS) throw std::runtime_error("irradiance request too large: n * n_u * n_v > 2^28 rays");
	if (n && (!positions || !normals)) throw std::runtime_error("null argument");
	for (uint32_t i = 0; i < n; ++i) {
		check_position(positions, i);
		check_normal(normals, i);
	}
	return (uint32_t)K;
}

// the descriptor's checks shared by the SH entries, for n probes; returns K
uint32_t check_sh_desc(uint64_t n, const ngp_irradiance_sh_desc* d) {
	if (!d) throw std::runtime_error("null argument");
	if (d->n_u == 0 || d->n_v == 0) throw std::runtime_error("invalid irradiance descriptor: n_u and n_v must be at least 1");
	const uint64_t K = (uint64_t)d->n_u * d->n_v;
	if (K > RAY_CHUNK) throw std::runtime_error("irradiance request too large: n_u * n_v > 2^21 rays per probe");
	if (n > MAX_TRACED_RAYS || K * n > MAX_TRACED_RAYS) throw std::runtime_error("irradiance request too large: probes * n_u * n_v > 2^28 rays");
	return (uint32_t)K;
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

void check_albedo(const float* albedo) {
	if (!albedo) throw std::runtime_error("null argument");
	for (int c = 0; c < 3; ++c)
		if (!std::isfinite(albedo[c]) || albedo[c] < 0.0f || albedo[c] > 1.0f)
			throw std::runtime_error("invalid irradiance bounce descriptor: albedo must be finite and in [0, 1] on every channel");
}

// a sun descriptor as the passes use it: the unit direction (formed in double, rounded to float) and albedo x radiance per channel
struct SunLight {
	float dir[3], source[3], radiance[3], bias;
	bool lit; // some channel of the source is not 0
};
SunLight check_sun(const ngp_irradiance_sun_desc* s, const float* albedo) {
	if (!finite3(s->direction) || !nonzero3(s->direction)) throw std::runtime_error("invalid irradiance sun descriptor: direction must be finite and not zero");
	for (int c = 0; c < 3; ++c)
		if (!std::isfinite(s->radiance[c]) || s->radiance[c] < 0.0f) throw std::runtime_error("invalid irradiance sun descriptor: radiance must be finite and >= 0 on every channel");
	if (!std::isfinite(s->shadow_bias) || s->shadow_bias < 0.0f) throw std::runtime_error("invalid irradiance sun descriptor: shadow_bias must be finite and >= 0");
	SunLight L{};
	const double x = s->direction[0], y = s->direction[1], z = s->direction[2], len = std::sqrt(x * x + y * y + z * z);
	L.dir[0] = (float)(x / len); L.dir[1] = (float)(y / len); L.dir[2] = (float)(z / len);
	for (int c = 0; c < 3; ++c) {
		L.radiance[c] = s->radiance[c];
		L.source[c] = albedo[c] * s->radiance[c];
		if (!std::isfinite(L.source[c])) throw std::runtime_error("invalid irradiance sun descriptor: albedo x radiance is not finite");
		L.lit = L.lit || L.source[c] != 0.0f;
	}
	L.bias = s->shadow_bias;
	return L;
}

// bounce, then sun, then the NeRF shadow: what the sunlit entries look at before anything else. Returns the sun as the passes use it.
SunLight check_sunlit(const ngp_irradiance_bounce_desc* bounce, const ngp_irradiance_sun_desc* sun, const ngp_irradiance_sun_nerf_desc* nerf) {
	if (!bounce) throw std::runtime_error(sun ? "invalid irradiance sun descriptor: the bounce descriptor (its albedo) is needed with a sun" : "null argument");
	if (bounce->n_bounces > MAX_BOUNCES) throw std::runtime_error("invalid irradiance bounce descriptor: n_bounces must be at most 16");
	check_albedo(bounce->albedo);
	SunLight L{};
	if (sun) L = check_sun(sun, bounce->albedo);
	if (nerf) check_desc(*nerf); // (nullable: the meshes alone shadow the sun)
	return L;
}

// ---- mesh albedos (contract: include/ngp_hip.h, "mesh albedos"): one call's table of one float4 a mesh, the resolved albedo a_m for the
// bounce passes or the source fl(a_m radiance) for the sun pass. While no mesh owns an albedo there is no table, and the passes launch the
// kernels that take the call's three scalars.
struct MeshColours {
	std::vector<float4> host; // empty: no mesh owns an albedo
	DevArray<float4> dev;     // the host's entries once upload_colours ran; get() is nullptr without a table
	bool any = false;         // some channel of some mesh's entry is not 0 (without a table: of the call's)
};
bool owns_albedo(const ngp_ctx* ctx) {
	for (const HostMesh& m : ctx->meshes)
		if (m.own_albedo) return true;
	return false;
}
// a_m of every mesh for a call whose albedo is `albedo`
void resolve_albedos(const ngp_ctx* ctx, const float* albedo, MeshColours& T) {
	T.any = nonzero3(albedo);
	if (!owns_albedo(ctx)) return;
	T.any = false;
	for (const HostMesh& m : ctx->meshes) {
		const float* a = m.own_albedo ? m.albedo : albedo;
		T.host.push_back(make_float4(a[0], a[1], a[2], 0.0f));
		T.any = T.any || nonzero3(a);
	}
}
// fl(a_m radiance) of every mesh, formed and checked as check_sun forms the call's
void resolve_sources(const ngp_ctx* ctx, const float* albedo, const SunLight& sun, MeshColours& T) {
	T.any = sun.lit;
	if (!owns_albedo(ctx)) return;
	T.any = false;
	for (const HostMesh& m : ctx->meshes) {
		const float* a = m.own_albedo ? m.albedo : albedo;
		float src[3];
		for (int c = 0; c < 3; ++c) {
			src[c] = a[c] * sun.radiance[c];
			if (!std::isfinite(src[c])) throw std::runtime_error("invalid irradiance sun descriptor: albedo x radiance is not finite");
		}
		T.host.push_back(make_float4(src[0], src[1], src[2], 0.0f));
		T.any = T.any || nonzero3(src);
	}
}
// the table onto the device, once a call, on the context's stream ahead of its passes; it goes with T, behind the call's last synchronisation
void upload_colours(ngp_ctx* ctx, MeshColours& T) {
	if (T.host.empty()) return;
	T.dev.reset(T.host.size());
	upload(ctx, T.dev.get(), T.host.data(), T.host.size() * sizeof(float4));
}

void require_volume(const ngp_ctx* ctx) {
	if (!ctx->d_sh_volume) throw std::runtime_error("no irradiance volume: call ngp_compute_irradiance_volume or ngp_set_irradiance_volume first");
}
void require_reference(const ngp_ctx* ctx) {
	if (!ctx->d_sh_reference)
		throw std::runtime_error("no reference irradiance volume: call ngp_compute_reference_irradiance_volume or ngp_set_reference_irradiance_volume first");
}
void require_visibility(const ngp_ctx* ctx) {
	if (!ctx->d_sh_visibility)
		throw std::runtime_error("no irradiance visibility: call ngp_compute_irradiance_volume_visibility or ngp_set_irradiance_volume_visibility first");
}

// ------------------------------------------------------------------------------------------------ chunks
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

// n probes of K <= RAY_CHUNK rays each, in chunks of whole probes: at most `cap` rays and `cap_pts` probes a chunk, which size the
// caller's buffers. Owns the chunk's positions on the device.
struct ProbeChunks {
	const uint32_t n, K, cap, cap_pts;
	DevArray<float> pts;
	ProbeChunks(uint32_t n, uint32_t K)
		: n(n), K(K), cap((uint32_t)std::min<uint64_t>((uint64_t)n * K, RAY_CHUNK)), cap_pts((uint32_t)std::min<uint64_t>(n, cap)), pts(3 * (size_t)cap_pts) {}
	// f(p0, np, r0, m): probes [p0, p0 + np) of the request, their positions uploaded to pts, are its rays [r0, r0 + m)
	template <typename F>
	void for_each(ngp_ctx* ctx, const float* positions, F&& f) {
		for_each_irradiance_chunk(n, K, [&](uint64_t r0, uint32_t m) {
			const uint64_t p0 = r0 / K;
			const uint32_t np = m / K;
			upload(ctx, pts.get(), positions + 3 * p0, (size_t)np * 3 * sizeof(float));
			f(p0, np, r0, m);
		});
	}
};

// the generator for rays [r0, r0 + m) of the request into o, d, t (the chunk's points are uploaded from the host arrays first)
void generate_irradiance_rays(ngp_ctx* ctx, const ngp_irradiance_trace_desc* d, uint32_t K, const float* positions, const float* normals, uint64_t r0, uint32_t m,
                              DevArray<float>& pts, float* o, float* dir, float2* t) {
	const uint64_t p0 = r0 / K, p1 = (r0 + m - 1) / K + 1;
	upload(ctx, pts.get(), positions + 3 * p0, (size_t)(p1 - p0) * 3 * sizeof(float));
	upload(ctx, pts.get() + pts.size() / 2, normals + 3 * p0, (size_t)(p1 - p0) * 3 * sizeof(float));
	launch_irradiance_rays(ctx->mesh_scene, d->occlude_by_meshes != 0, d->n_u, d->n_v, d->offset, r0, m, pts.get(), pts.get() + pts.size() / 2, o, dir, t, ctx->stream);
}

// ------------------------------------------------------------------------------------------------ envmap probes
// trace the fan(s) described by P in ONE persistent launch, reduce to the probe texture(s), tabulate E(n) at the texel directions
void compute_probes(ngp_ctx* ctx, ProbeParams P, float min_transmittance) {
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
	TracerCall tr(ctx, P.n_rays, min_transmittance);
	tr.trace(P); // (Geometry mode: the shell positions lie inside the mesh box)
	launch_probe_reduce(P, ctx->d_envmap.get(), ctx->stream);
	launch_irradiance(P, ctx->d_envmap.get(), n_texels, nullptr, ctx->d_irradiance.get(), ctx->stream);
	tr.finish(); // (synchronises the stream: ray_rgba may go)
	P.ray_rgba = nullptr;
	++ctx->probe_generation;
	ctx->env_probe = P;
	ctx->env_n_theta = P.n_theta;
	ctx->env_n_phi = P.n_phi;
}

// ------------------------------------------------------------------------------------------------ SH9 irradiance volumes
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
	ProbeChunks chunks(n, K);
	DevArray<float> o(3 * (size_t)chunks.cap), dir(3 * (size_t)chunks.cap);
	DevArray<float2> t(chunks.cap);
	DevArray<float4> rgba(chunks.cap), rec(SH_FLOAT4 * (size_t)chunks.cap_pts);
	TracerCall tr(ctx, (uint64_t)n * K, d->min_transmittance);
	chunks.for_each(ctx, positions, [&](uint64_t p0, uint32_t np, uint64_t r0, uint32_t m) {
		launch_irradiance_sphere_rays(ctx->mesh_scene, d->occlude_by_meshes != 0, d->n_u, d->n_v, m, chunks.pts.get(), o.get(), dir.get(), t.get(), ctx->stream);
		launch_ray_list_prep(tr.model(), m, o.get(), dir.get(), t.get(), false, ctx->stream);
		tr.trace_rays(m, o.get(), dir.get(), t.get(), rgba.get());
		launch_irradiance_sh_reduce(d->n_u, d->n_v, np, rgba.get(), t.get(), rec.get(), ctx->stream);
		if (d_sh) NGP_HIP_CHECK(hipMemcpyAsync(d_sh + SH_FLOAT4 * p0, rec.get(), (size_t)np * SH_FLOAT4 * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
		if (d_alpha) launch_ray_alpha(m, rgba.get(), d_alpha + r0, ctx->stream);
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
// maps of the context's volume and the descriptor they were made with, max_distance resolved to D
void commit_visibility(ngp_ctx* ctx, DevArray<float2>& maps, const ngp_irradiance_visibility_desc& d, float D) {
	ctx->d_sh_visibility = std::move(maps);
	ctx->sh_visibility_desc = d;
	ctx->sh_visibility_desc.max_distance = D;
}
// records for the lattice of d; the maps of the volume before it go (the lattice may have changed)
void commit_volume(ngp_ctx* ctx, DevArray<float4>& sh, const ngp_irradiance_volume_desc& d) {
	ctx->d_sh_volume = std::move(sh);
	ctx->sh_volume_desc = d;
	drop_visibility(ctx);
	++ctx->sh_volume_generation;
}
// no volume on this context (the primary or a replica, its device current), once its stream has drained
void drop_volume(ngp_ctx* ctx) {
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	ctx->d_sh_volume.reset();
	ctx->sh_volume_desc = ngp_irradiance_volume_desc{};
	drop_visibility(ctx);
}
// the reference volume (the scene before the meshes): records for the lattice of d; it has no maps
void commit_reference(ngp_ctx* ctx, DevArray<float4>& sh, const ngp_irradiance_volume_desc& d) {
	ctx->d_sh_reference = std::move(sh);
	ctx->sh_reference_desc = d;
	++ctx->sh_reference_generation;
}
void drop_reference(ngp_ctx* ctx) {
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream));
	ctx->d_sh_reference.reset();
	ctx->sh_reference_desc = ngp_irradiance_volume_desc{};
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
	ProbeChunks chunks(n, K);
	DevArray<float> o(3 * (size_t)chunks.cap), dir(3 * (size_t)chunks.cap);
	DevArray<float2> t(chunks.cap), maps(DISTANCE_MAP_TEXELS * (size_t)chunks.cap_pts);
	chunks.for_each(ctx, positions, [&](uint64_t p0, uint32_t np, uint64_t, uint32_t m) {
		launch_irradiance_sphere_rays(ctx->mesh_scene, true, d->n_u, d->n_v, m, chunks.pts.get(), o.get(), dir.get(), t.get(), ctx->stream);
		launch_irradiance_distance_reduce(d->n_u, d->n_v, np, d->sharpness_log2, D, t.get(), maps.get(), ctx->stream);
		const size_t bytes = (size_t)np * DISTANCE_MAP_TEXELS * sizeof(float2);
		if (d_maps) NGP_HIP_CHECK(hipMemcpyAsync(d_maps + DISTANCE_MAP_TEXELS * p0, maps.get(), bytes, hipMemcpyDeviceToDevice, ctx->stream));
		if (h_maps) download(ctx, h_maps + 2 * DISTANCE_MAP_TEXELS * p0, maps.get(), bytes);
	});
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (the chunk buffers may go)
	NGP_HIP_CHECK(hipGetLastError());
}

// ---- light off the meshes: the sun pass and the diffuse bounce passes (contract: include/ngp_hip.h, "bounces" and "sun")
// one pass at n probes (host positions), in chunks of whole probes: rays(pts, r0, m, rgba, t) launches the generator that leaves a chunk's
// rays' (B rgb, t) and (0, t), the projection follows (no tracer: a pass needs the BVHs alone, a bounce pass the records too). Each chunk's
// records R go to h_sh (host, n x 28), its rays to h_rays (host, n K x 4) and d_v0 + R to d_next (device, 7 n float4 each, not d_v0
// itself); all nullable. ms: the pass's device time.
template <typename Rays>
void mesh_light_pass(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* d, uint32_t K, Rays&& rays, float* h_sh, float* h_rays,
                     const float4* d_v0, float4* d_next, float* ms) {
	ProbeChunks chunks(n, K);
	DevArray<float2> t(chunks.cap);
	DevArray<float4> rgba(chunks.cap), rec(SH_FLOAT4 * (size_t)chunks.cap_pts);
	const Event ev0 = new_event(), ev1 = new_event();
	NGP_HIP_CHECK(hipEventRecord(ev0, ctx->stream));
	chunks.for_each(ctx, positions, [&](uint64_t p0, uint32_t np, uint64_t r0, uint32_t m) {
		rays(chunks.pts.get(), r0, m, rgba.get(), t.get());
		launch_irradiance_sh_reduce(d->n_u, d->n_v, np, rgba.get(), t.get(), rec.get(), ctx->stream);
		if (d_next) launch_irradiance_volume_add(SH_FLOAT4 * np, d_v0 + SH_FLOAT4 * p0, rec.get(), d_next + SH_FLOAT4 * p0, ctx->stream);
		if (h_rays) download(ctx, h_rays + 4 * r0, rgba.get(), (size_t)m * sizeof(float4));
		if (h_sh) download(ctx, h_sh + 4 * SH_FLOAT4 * p0, rec.get(), (size_t)np * SH_FLOAT4 * sizeof(float4));
	});
	NGP_HIP_CHECK(hipEventRecord(ev1, ctx->stream));
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (the chunk buffers may go)
	NGP_HIP_CHECK(hipGetLastError());
	NGP_HIP_CHECK(hipEventElapsedTime(ms, ev0, ev1));
}
// one bounce pass from the source volume V (VV non-null: through its visible lookup): the lookup at the rays' mesh hits. d_alpha: the
// rays' NeRF alpha, n K floats on the device (nullable: 0). d_albedos: the call's table of the meshes' albedos (nullable: `albedo` for all).
void bounce_pass(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* d, uint32_t K, const float* albedo, const float4* d_albedos, const IrradianceVolume& V,
                 const IrradianceVolumeVisible* VV, const float* d_alpha, float* h_sh, float* h_rays, const float4* d_v0, float4* d_next) {
	mesh_light_pass(ctx, n, positions, d, K, [&](const float* pts, uint64_t r0, uint32_t m, float4* rgba, float2* t) {
		launch_irradiance_bounce_rays(ctx->mesh_scene, V, VV, d->occlude_by_meshes != 0, d->n_u, d->n_v, m, pts, albedo, d_albedos, d_alpha ? d_alpha + r0 : nullptr, rgba, t, ctx->stream);
	}, h_sh, h_rays, d_v0, d_next, &ctx->sh_bounce_ms);
}
// the sun pass: the shadow query at the rays' mesh hits that face the sun; no volume is read. d_alpha as above. d_sources: the call's table
// of the meshes' sources (nullable: sun.source for all).
void sun_pass(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* d, uint32_t K, const SunLight& sun, const float4* d_sources, const float* d_alpha, float* h_sh,
              float* h_rays, const float4* d_v0, float4* d_next) {
	mesh_light_pass(ctx, n, positions, d, K, [&](const float* pts, uint64_t r0, uint32_t m, float4* rgba, float2* t) {
		launch_irradiance_sun_rays(ctx->mesh_scene, d->occlude_by_meshes != 0, d->n_u, d->n_v, m, pts, sun.dir, sun.bias, sun.source, d_sources, d_alpha ? d_alpha + r0 : nullptr, rgba, t,
		                           ctx->stream);
	}, h_sh, h_rays, d_v0, d_next, &ctx->sh_sun_ms);
	ctx->sh_sun_shadow_ms = 0.f;
}

// the sun pass with the NeRF's density in front of the sun: per chunk the generator also leaves the shadow-ray list (one entry a probe ray,
// dead where the sun lights nothing), the ray-list tracer walks it inside ONE tracer call, and the apply kernel scales B ahead of the
// projection. h_shadow (host, n K x 4, nullable): (q, alpha_s) per ray. Needs a model (require_probe_model is the caller's).
void sun_pass_shadowed(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* d, uint32_t K, const SunLight& sun, const float4* d_sources,
                       const ngp_irradiance_sun_nerf_desc& nerf, const float* d_alpha, float* h_sh, float* h_rays, float* h_shadow, const float4* d_v0, float4* d_next) {
	const size_t cap = (size_t)std::min<uint64_t>((uint64_t)n * K, RAY_CHUNK); // (ProbeChunks' cap)
	DevArray<float> o(3 * cap), dir(3 * cap);
	DevArray<float2> st(cap);
	DevArray<float4> traced(cap), shadow(h_shadow ? cap : 0);
	std::vector<std::pair<Event, Event>> spans; // one chunk's prep and trace each
	TracerCall tr(ctx, (uint64_t)n * K, nerf.min_transmittance);
	mesh_light_pass(ctx, n, positions, d, K, [&](const float* pts, uint64_t r0, uint32_t m, float4* rgba, float2* t) {
		launch_irradiance_sun_shadow_rays(ctx->mesh_scene, d->occlude_by_meshes != 0, d->n_u, d->n_v, m, pts, sun.dir, sun.bias, sun.source, d_sources, d_alpha ? d_alpha + r0 : nullptr,
		                                  nerf.t_min, rgba, t, o.get(), dir.get(), st.get(), ctx->stream);
		spans.emplace_back(new_event(), new_event());
		NGP_HIP_CHECK(hipEventRecord(spans.back().first, ctx->stream));
		launch_ray_list_prep(tr.model(), m, o.get(), dir.get(), st.get(), true, ctx->stream);
		tr.trace_rays(m, o.get(), dir.get(), st.get(), traced.get());
		NGP_HIP_CHECK(hipEventRecord(spans.back().second, ctx->stream));
		launch_irradiance_sun_shadow_apply(m, traced.get(), o.get(), st.get(), rgba, shadow.get(), ctx->stream);
		if (h_shadow) download(ctx, h_shadow + 4 * r0, shadow.get(), (size_t)m * sizeof(float4));
	}, h_sh, h_rays, d_v0, d_next, &ctx->sh_sun_ms);
	tr.finish(); // (synchronises the stream: the list may go)
	ctx->sh_sun_shadow_ms = 0.f;
	for (const auto& s : spans) {
		float ms = 0.f;
		NGP_HIP_CHECK(hipEventElapsedTime(&ms, s.first, s.second));
		ctx->sh_sun_shadow_ms += ms;
	}
}

// the volume of desc: V_0 traced through the NeRF, then the sun's first bounce off the meshes S = V_0 + R_sun (`sun` nullable: none, S =
// V_0; `nerf` nullable: the NeRF's density does not shadow the sun), then `bounce` (nullable: none) passes V_b = S + R(V_{b-1}) looked up through the distance maps of `visibility` (nullable: none,
// and none kept). The context's volume is replaced once every launch has succeeded; `reference`: the context's reference volume instead
// (ngp_compute_reference_irradiance_volume: V_0 alone, its caller passes no pass and a descriptor that does not occlude), the volume untouched.
void compute_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const ngp_irradiance_bounce_desc* bounce, const ngp_irradiance_visibility_desc* visibility,
                    const SunLight* sun = nullptr, const ngp_irradiance_sun_nerf_desc* nerf = nullptr, bool reference = false) {
	require_probe_model(ctx, "SH irradiance probes");
	const uint64_t probes = check_volume_lattice(desc);
	const uint32_t K = check_sh_desc(probes, &desc->sh);
	const uint32_t K_vis = visibility ? check_visibility_desc(probes, visibility, true) : 0;
	const float D = visibility ? visibility_distance(visibility, *desc) : 0.0f;
	const std::vector<float> positions = volume_positions(desc, probes);
	// without a source (no pass asked for, every mesh's albedo black, nothing to hit) the records are V_0's own: no pass runs
	const float* al = bounce ? bounce->albedo : nullptr;
	MeshColours albedos, sources; // (the meshes' own albedos resolved against the call's; no tables while no mesh owns one)
	if (al) resolve_albedos(ctx, al, albedos);
	if (al && sun) resolve_sources(ctx, al, *sun, sources);
	const bool hits = !ctx->meshes.empty() && desc->sh.occlude_by_meshes != 0;
	const uint32_t n_bounces = al && albedos.any && hits ? bounce->n_bounces : 0;
	const bool sunlit = sun && sources.any && hits; // (black albedos leave no channel of any source lit)
	DevArray<float4> traced(SH_FLOAT4 * (size_t)probes), lit(sunlit ? traced.size() : 0), even(n_bounces > 1 ? traced.size() : 0), odd(n_bounces > 0 ? traced.size() : 0);
	DevArray<float> alpha(n_bounces || sunlit ? (size_t)probes * K : 0); // the whole volume's rays: the NeRF is traced once
	// (alpha is empty without a pass: an empty DevArray's get() is nullptr, which is how trace_sh_probes and bounce_pass are told "none")
	trace_sh_probes(ctx, (uint32_t)probes, positions.data(), &desc->sh, K, nullptr, traced.get(), nullptr, alpha.get());
	DevArray<float2> maps(visibility ? DISTANCE_MAP_TEXELS * (size_t)probes : 0);
	if (visibility) distance_maps(ctx, (uint32_t)probes, positions.data(), visibility, K_vis, D, nullptr, maps.get());
	IrradianceVolumeVisible A{};
	A.maps = maps.get();
	A.D = D;
	A.normal_bias = visibility ? visibility->normal_bias : 0.0f;
	if (sunlit) upload_colours(ctx, sources);
	if (n_bounces) upload_colours(ctx, albedos);
	if (sunlit && nerf) sun_pass_shadowed(ctx, (uint32_t)probes, positions.data(), &desc->sh, K, *sun, sources.dev.get(), *nerf, alpha.get(), nullptr, nullptr, nullptr, traced.get(), lit.get());
	else if (sunlit) sun_pass(ctx, (uint32_t)probes, positions.data(), &desc->sh, K, *sun, sources.dev.get(), alpha.get(), nullptr, nullptr, traced.get(), lit.get());
	DevArray<float4>& v0 = sunlit ? lit : traced; // what the passes add to: the sun's light bounces with the NeRF's
	const float4* prev = v0.get();
	for (uint32_t b = 1; b <= n_bounces; ++b) { // every probe of a pass reads the pass before it alone
		float4* next = b % 2u ? odd.get() : even.get();
		A.V = irradiance_volume_from(*desc, prev);
		bounce_pass(ctx, (uint32_t)probes, positions.data(), &desc->sh, K, al, albedos.dev.get(), A.V, visibility ? &A : nullptr, alpha.get(), nullptr, nullptr, v0.get(), next);
		prev = next;
	}
	if (reference) return commit_reference(ctx, v0, *desc);
	commit_volume(ctx, n_bounces == 0 ? v0 : n_bounces % 2u ? odd : even, *desc); // (the previous volume stays in place when a launch throws)
	if (visibility) commit_visibility(ctx, maps, *visibility, D);
}

// a caller's records for the lattice of desc, checked and on the device (ngp_set_irradiance_volume, ngp_set_reference_irradiance_volume)
DevArray<float4> upload_volume_records(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const float* sh) {
	const uint64_t probes = check_volume_lattice(desc);
	if (!sh) throw std::runtime_error("null argument");
	for (size_t i = 0; i < 4 * SH_FLOAT4 * (size_t)probes; ++i)
		if (!std::isfinite(sh[i])) throw std::runtime_error("irradiance volume: value " + std::to_string(i % 28) + " of probe " + std::to_string(i / 28) + " is not finite");
	DevArray<float4> d;
	d.upload(reinterpret_cast<const float4*>(sh), SH_FLOAT4 * (size_t)probes);
	NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (a lookup still in flight reads the old records)
	return d;
}

} // namespace

extern "C" {

int ngp_compute_envmap(ngp_ctx* ctx, const ngp_probe_desc* d, float* rgba_out) {
	return guarded(ctx, [&] {
		if (!d || d->n_theta == 0 || d->n_phi == 0 || d->mode < 0 || d->mode > 2) throw std::runtime_error("invalid probe descriptor");
		if (d->mode == NGP_PROBE_MULTI_CENTER && d->n_origin == 0) throw std::runtime_error("invalid probe descriptor: n_origin");
		ProbeParams P{};
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
		ProbeParams P{};
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
		const ProbeParams& P = ctx->env_probe;
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

int ngp_irradiance(ngp_ctx* ctx, uint32_t n, const float* normals, float* rgb_out) {
	return guarded(ctx, [&] {
		if (!ctx->d_envmap) throw std::runtime_error("no probe texture: call ngp_compute_envmap first");
		if (ctx->env_probe.mode == 3) throw std::runtime_error("the probe texture is a grid: use ngp_irradiance_at (position + normal)");
		if (n == 0) return;
		if (!normals || !rgb_out) throw std::runtime_error("null argument");
		lookup_rgb(ctx, n, nullptr, normals, rgb_out,
		             [&](const float*, const float* d_n, float4* d_o) { launch_irradiance(ctx->env_probe, ctx->d_envmap.get(), n, d_n, d_o, ctx->stream); });
	});
}

int ngp_irradiance_at(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, float* rgb_out) {
	return guarded(ctx, [&] {
		if (!ctx->d_irradiance) throw std::runtime_error("no probe texture: call ngp_compute_envmap / ngp_compute_envmap_grid first");
		if (n == 0) return;
		if (!positions || !normals || !rgb_out) throw std::runtime_error("null argument");
		lookup_rgb(ctx, n, positions, normals, rgb_out,
		             [&](const float* d_p, const float* d_n, float4* d_o) { launch_irradiance_lookup(irradiance_map_of(ctx), n, d_p, d_n, d_o, ctx->stream); });
	});
}

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
		TracerCall tr(ctx, n, min_transmittance);
		for (uint32_t r0 = 0; r0 < n; r0 += cap) {
			const uint32_t m = std::min(cap, n - r0);
			upload(ctx, o.get(), origins + 3 * (size_t)r0, (size_t)m * 3 * sizeof(float));
			upload(ctx, dir.get(), directions + 3 * (size_t)r0, (size_t)m * 3 * sizeof(float));
			for (uint32_t i = 0; i < m; ++i)
				t_host[i] = t_range ? make_float2(t_range[2 * (size_t)(r0 + i)], t_range[2 * (size_t)(r0 + i) + 1]) : make_float2(0.0f, std::numeric_limits<float>::infinity());
			upload(ctx, t.get(), t_host.data(), (size_t)m * sizeof(float2));
			launch_ray_list_prep(tr.model(), m, o.get(), dir.get(), t.get(), true, ctx->stream);
			tr.trace_rays(m, o.get(), dir.get(), t.get(), rgba.get(), depth.get());
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
			download_rays(ctx, r0, m, o.get(), dir.get(), t.get(), t_host, origins_out, directions_out, t_max_out);
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
		TracerCall tr(ctx, (uint64_t)n * K, desc->min_transmittance);
		for_each_irradiance_chunk(n, K, [&](uint64_t r0, uint32_t m) {
			generate_irradiance_rays(ctx, desc, K, positions, normals, r0, m, pts, o.get(), dir.get(), t.get());
			launch_ray_list_prep(tr.model(), m, o.get(), dir.get(), t.get(), false, ctx->stream);
			tr.trace_rays(m, o.get(), dir.get(), t.get(), rgba.get());
			launch_irradiance_reduce(K, r0, m, rgba.get(), t.get(), part.get(), E.get(), ctx->stream);
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
		ProbeChunks chunks(n, K);
		DevArray<float> o(3 * (size_t)chunks.cap), dir(3 * (size_t)chunks.cap);
		DevArray<float2> t(chunks.cap);
		std::vector<float2> t_host(chunks.cap);
		chunks.for_each(ctx, positions, [&](uint64_t, uint32_t, uint64_t r0, uint32_t m) {
			launch_irradiance_sphere_rays(ctx->mesh_scene, desc->occlude_by_meshes != 0, desc->n_u, desc->n_v, m, chunks.pts.get(), o.get(), dir.get(), t.get(), ctx->stream);
			download_rays(ctx, r0, m, o.get(), dir.get(), t.get(), t_host, origins_out, directions_out, t_max_out);
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
	return guarded(ctx, [&] { compute_volume(ctx, desc, nullptr, nullptr); });
}

int ngp_compute_irradiance_volume_bounced(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const ngp_irradiance_bounce_desc* bounce,
                                          const ngp_irradiance_visibility_desc* visibility) {
	return guarded(ctx, [&] {
		if (!bounce) throw std::runtime_error("null argument");
		if (bounce->n_bounces > MAX_BOUNCES) throw std::runtime_error("invalid irradiance bounce descriptor: n_bounces must be at most 16");
		check_albedo(bounce->albedo);
		compute_volume(ctx, desc, bounce, visibility);
	});
}

int ngp_compute_irradiance_volume_sunlit(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const ngp_irradiance_bounce_desc* bounce,
                                         const ngp_irradiance_visibility_desc* visibility, const ngp_irradiance_sun_desc* sun) {
	return guarded(ctx, [&] {
		const SunLight L = check_sunlit(bounce, sun, nullptr);
		compute_volume(ctx, desc, bounce, visibility, sun ? &L : nullptr);
	});
}

int ngp_compute_irradiance_volume_sunlit_shadowed(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const ngp_irradiance_bounce_desc* bounce,
                                                  const ngp_irradiance_visibility_desc* visibility, const ngp_irradiance_sun_desc* sun, const ngp_irradiance_sun_nerf_desc* nerf) {
	return guarded(ctx, [&] {
		const SunLight L = check_sunlit(bounce, sun, nerf);
		compute_volume(ctx, desc, bounce, visibility, sun ? &L : nullptr, nerf);
	});
}

int ngp_irradiance_sh_sun(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* desc, const ngp_irradiance_sun_desc* sun, const float* albedo,
                          const float* alpha, float* sh_out, float* rays_out) {
	return guarded(ctx, [&] {
		check_albedo(albedo);
		if (!sun) throw std::runtime_error("null argument");
		const SunLight L = check_sun(sun, albedo);
		require_device(ctx);
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
		MeshColours sources;
		resolve_sources(ctx, albedo, L, sources);
		upload_colours(ctx, sources);
		sun_pass(ctx, n, positions, desc, K, L, sources.dev.get(), d_alpha.get(), sh_out, rays_out, nullptr, nullptr); // (no alpha: d_alpha is empty, get() nullptr)
	});
}

int ngp_irradiance_sh_sun_shadowed(ngp_ctx* ctx, uint32_t n, const float* positions, const ngp_irradiance_sh_desc* desc, const ngp_irradiance_sun_desc* sun, const float* albedo,
                                   const float* alpha, const ngp_irradiance_sun_nerf_desc* nerf, float* rays_out, float* shadow_out, float* sh_out) {
	return guarded(ctx, [&] {
		check_albedo(albedo);
		if (!sun || !nerf) throw std::runtime_error("null argument");
		const SunLight L = check_sun(sun, albedo);
		if (nerf) check_desc(*nerf);
		require_model(ctx, "the sun's shadow rays are traced through the model");
		require_probe_model(ctx, "the sun's shadow rays");
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
		MeshColours sources;
		resolve_sources(ctx, albedo, L, sources);
		upload_colours(ctx, sources);
		sun_pass_shadowed(ctx, n, positions, desc, K, L, sources.dev.get(), *nerf, d_alpha.get(), sh_out, rays_out, shadow_out, nullptr, nullptr); // (no alpha: d_alpha is empty, get() nullptr)
	});
}

int ngp_get_irradiance_sun_shadow_ms(ngp_ctx* ctx, float* ms) {
	return guarded(ctx, [&] {
		require_device(ctx);
		if (!ms) throw std::runtime_error("null argument");
		*ms = ctx->sh_sun_shadow_ms;
	});
}

int ngp_get_irradiance_sun_ms(ngp_ctx* ctx, float* ms) {
	return guarded(ctx, [&] {
		require_device(ctx);
		if (!ms) throw std::runtime_error("null argument");
		*ms = ctx->sh_sun_ms;
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
		const IrradianceVolumeVisible A = use_visible ? sh_volume_visible_of(ctx) : IrradianceVolumeVisible{};
		MeshColours albedos;
		resolve_albedos(ctx, albedo, albedos);
		upload_colours(ctx, albedos);
		bounce_pass(ctx, n, positions, desc, K, albedo, albedos.dev.get(), sh_volume_of(ctx), use_visible ? &A : nullptr, d_alpha.get(), sh_out, rays_out, nullptr, nullptr); // (no alpha: d_alpha is empty, get() nullptr)
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
		DevArray<float4> d = upload_volume_records(ctx, desc, sh);
		commit_volume(ctx, d, *desc);
	});
}

int ngp_get_irradiance_volume(ngp_ctx* ctx, ngp_irradiance_volume_desc* desc_out, float* sh_out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		require_volume(ctx);
		if (desc_out) *desc_out = ctx->sh_volume_desc;
		if (sh_out) download(ctx, sh_out, ctx->d_sh_volume.get(), ctx->d_sh_volume.size() * sizeof(float4));
	});
}

int ngp_clear_irradiance_volume(ngp_ctx* ctx) {
	return guarded(ctx, [&] {
		require_device(ctx);
		drop_volume(ctx);
		++ctx->sh_volume_generation;
		for (ngp_ctx* p : ctx->peers) { // the replicas go too: a multi-device frame refuses like a single-device one
			DeviceGuard g(p->device);
			drop_volume(p);
			p->synced_sh_volume_generation = ctx->sh_volume_generation;
		}
	});
}

int ngp_compute_reference_irradiance_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc) {
	return guarded(ctx, [&] {
		if (!desc) throw std::runtime_error("null argument");
		ngp_irradiance_volume_desc d = *desc;
		d.sh.occlude_by_meshes = 0; // the scene before anything was inserted, whatever the caller's descriptor says
		compute_volume(ctx, &d, nullptr, nullptr, nullptr, nullptr, true);
	});
}

int ngp_set_reference_irradiance_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const float* sh) {
	return guarded(ctx, [&] {
		require_device(ctx);
		DevArray<float4> d = upload_volume_records(ctx, desc, sh);
		commit_reference(ctx, d, *desc);
	});
}

int ngp_get_reference_irradiance_volume(ngp_ctx* ctx, ngp_irradiance_volume_desc* desc_out, float* sh_out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		require_reference(ctx);
		if (desc_out) *desc_out = ctx->sh_reference_desc;
		if (sh_out) download(ctx, sh_out, ctx->d_sh_reference.get(), ctx->d_sh_reference.size() * sizeof(float4));
	});
}

int ngp_clear_reference_irradiance_volume(ngp_ctx* ctx) {
	return guarded(ctx, [&] {
		require_device(ctx);
		drop_reference(ctx);
		++ctx->sh_reference_generation;
		for (ngp_ctx* p : ctx->peers) { // the replicas go too
			DeviceGuard g(p->device);
			drop_reference(p);
			p->synced_sh_reference_generation = ctx->sh_reference_generation;
		}
	});
}

int ngp_irradiance_volume_ratio(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, const ngp_ambient_change_desc* desc, float* out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		require_volume(ctx);
		require_reference(ctx);
		if (!desc) throw std::runtime_error("null argument");
		check_desc(*desc);
		if (n == 0) return;
		if (!positions || !normals || !out) throw std::runtime_error("null argument");
		check_positions(n, positions);
		check_normals(n, normals);
		lookup_rgbw(ctx, n, positions, normals, out, [&](const float* d_p, const float* d_n, float4* d_o) {
			launch_irradiance_volume_ratio(sh_volume_of(ctx), sh_reference_of(ctx), n, d_p, d_n, desc->min_irradiance, desc->max_gain, d_o, ctx->stream);
		});
	});
}

int ngp_irradiance_volume_at(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, float* out) {
	return guarded(ctx, [&] {
		require_device(ctx);
		require_volume(ctx);
		if (n == 0) return;
		if (!positions || !normals || !out) throw std::runtime_error("null argument");
		check_positions(n, positions);
		check_normals(n, normals);
		lookup_rgbw(ctx, n, positions, normals, out,
		             [&](const float* d_p, const float* d_n, float4* d_o) { launch_irradiance_volume_lookup(sh_volume_of(ctx), n, d_p, d_n, d_o, ctx->stream); });
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
		DevArray<float2> maps(DISTANCE_MAP_TEXELS * (size_t)probes);
		distance_maps(ctx, (uint32_t)probes, positions.data(), desc, K, D, nullptr, maps.get());
		commit_visibility(ctx, maps, *desc, D); // (the previous maps stay in place when a launch throws)
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
		const size_t probes = ctx->d_sh_volume.size() / SH_FLOAT4, texels = DISTANCE_MAP_TEXELS * probes;
		for (size_t i = 0; i < 2 * texels; ++i)
			if (!std::isfinite(maps[i]) || maps[i] < 0.0f)
				throw std::runtime_error("irradiance visibility: m" + std::to_string(i % 2 + 1) + " of texel " + std::to_string(i / 2 % 64) + " of probe " + std::to_string(i / 128) +
				                         (std::isfinite(maps[i]) ? " is negative" : " is not finite"));
		DevArray<float2> d;
		d.upload(reinterpret_cast<const float2*>(maps), texels);
		NGP_HIP_CHECK(hipStreamSynchronize(ctx->stream)); // (a lookup still in flight reads the old maps)
		commit_visibility(ctx, d, *desc, desc->max_distance);
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
		lookup_rgbw(ctx, n, positions, normals, out, [&](const float* d_p, const float* d_n, float4* d_o) {
			launch_irradiance_volume_lookup_visible(sh_volume_visible_of(ctx), n, d_p, d_n, d_o, ctx->stream);
		});
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
		sh9_irradiance(sh + 28 * (size_t)i, x / len, y / len, z / len, E);
		for (int c = 0; c < 3; ++c) rgb_out[3 * (size_t)i + c] = (float)E[c];
	}
	return 0;
}

} // extern "C"
