// Host-side state behind the C ABI (include/ngp_hip.h): model, dataset, frame buffers.
#pragma once

#include "../../include/ngp_hip.h"
#include "mc_table.h"
#include "minijson.h"
#include "ngp_kernels.h"
#include "pcg32.h"
#include "train_kernels.h"

#include <hip/hip_runtime.h>

#include <array>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <sstream>
#include <sys/stat.h>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace ngp {

#define NGP_HIP_CHECK(expr)                                                                                        \
	do {                                                                                                           \
		hipError_t _e = (expr);                                                                                    \
		if (_e != hipSuccess) throw std::runtime_error(std::string(#expr " failed: ") + hipGetErrorString(_e));   \
	} while (0)

// ------------------------------------------------------------------------------------------------ owners of HIP resources
// Move-only. An empty owner makes no HIP call, so host-only contexts (ngp_create(-1)) never touch the runtime.
template <typename T, bool Pinned = false>
class HipArray { // n elements of device memory, or of page-locked host memory
public:
	HipArray() = default;
	explicit HipArray(size_t n) { reset(n); }
	HipArray(HipArray&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
	HipArray& operator=(HipArray&& o) noexcept {
		if (this != &o) {
			reset();
			std::swap(p_, o.p_);
			std::swap(n_, o.n_);
		}
		return *this;
	}
	~HipArray() { reset(); }
	// frees the old allocation before it makes the new one (peak memory of a regrow = the new size)
	void reset(size_t n = 0) {
		if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
		p_ = nullptr;
		n_ = 0;
		if (!n) return;
		if (Pinned) NGP_HIP_CHECK(hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault));
		else NGP_HIP_CHECK(hipMalloc((void**)&p_, n * sizeof(T)));
		n_ = n;
	}
	void upload(const T* src, size_t n) { // reset(n) + a synchronous copy from the host
		reset(n);
		if (n) NGP_HIP_CHECK(hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice));
	}
	T* get() const { return p_; }
	size_t size() const { return n_; }
	size_t bytes() const { return n_ * sizeof(T); }
	explicit operator bool() const { return p_ != nullptr; }

private:
	T* p_ = nullptr;
	size_t n_ = 0;
};
template <typename T> using DevArray = HipArray<T>;
template <typename T> using PinnedArray = HipArray<T, true>;

template <typename H, hipError_t (*Destroy)(H)>
class HipHandle { // an event or a stream; converts to the raw handle for the runtime's calls
public:
	HipHandle() = default;
	explicit HipHandle(H h) : h_(h) {}
	HipHandle(HipHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
	HipHandle& operator=(HipHandle&& o) noexcept {
		if (this != &o) {
			if (h_) (void)Destroy(h_);
			h_ = o.h_;
			o.h_ = nullptr;
		}
		return *this;
	}
	~HipHandle() {
		if (h_) (void)Destroy(h_);
	}
	operator H() const { return h_; }

private:
	H h_ = nullptr;
};
using Event = HipHandle<hipEvent_t, hipEventDestroy>;
using Stream = HipHandle<hipStream_t, hipStreamDestroy>;
inline Event new_event(unsigned flags = hipEventDefault) {
	hipEvent_t e = nullptr;
	NGP_HIP_CHECK(hipEventCreateWithFlags(&e, flags));
	return Event(e);
}
inline Stream new_stream(unsigned flags = hipStreamDefault) {
	hipStream_t s = nullptr;
	NGP_HIP_CHECK(hipStreamCreateWithFlags(&s, flags));
	return Stream(s);
}

// makes `device` current for a scope; the previous device is current again when it ends, on a throw as well
struct DeviceGuard {
	int prev = 0;
	explicit DeviceGuard(int dev) {
		(void)hipGetDevice(&prev);
		NGP_HIP_CHECK(hipSetDevice(dev));
	}
	~DeviceGuard() { (void)hipSetDevice(prev); }
};

// kernel launchers, nerf_kernels.hip
const char* launch_render_nerf(const ModelParams& M, const CameraParams& C, const FrameParams& F, int n_cus, hipStream_t stream); // returns the name of the kernel it chose (ngp_last_render_kernel)
void launch_grid_encode(const ModelParams& M, uint32_t n, const float* pos01, uint16_t* out, hipStream_t stream);
void launch_build_normals_fragments(uint4* wfrags, hipStream_t stream); // after every change of the forward fragments
void launch_density_gradient(const ModelParams& M, uint32_t n, const float* pos01, float* out, hipStream_t stream);
// wide_kernels.hip (ModelParams::wide): the launchers above that take a model forward to these when M.wide.width != 0
void launch_render_nerf_wide(const ModelParams& M, const CameraParams& C, const FrameParams& F, int n_cus, hipStream_t stream);
void launch_trace_probe_wide(const ModelParams& M, const FrameParams& F, const ProbeParams& P, int n_cus, hipStream_t stream);
void launch_network_inference_wide(const ModelParams& M, uint32_t n, const float* pos01, const float* dir01, uint16_t* out, int n_cus, hipStream_t stream);
void launch_density_gradient_wide(const ModelParams& M, uint32_t n, const float* pos01, float* out, int n_cus, hipStream_t stream);
void launch_frequency_encode(const ModelParams& M, uint32_t n, const float* pos01, uint16_t* out, hipStream_t stream);
void launch_network_inference(const ModelParams& M, uint32_t n, const float* pos01, const float* dir01, uint16_t* out, hipStream_t stream);
void launch_density_grid_update(const ModelParams& M, uint32_t n_samples, const Pcg32& rng, uint32_t step, uint32_t n_cascades, float thresh, const float* grid,
                                float* grid_tmp, hipStream_t stream);
void launch_density_grid_update_wide(const ModelParams& M, uint32_t n_samples, const Pcg32& rng, uint32_t step, uint32_t n_cascades, float thresh, const float* grid,
                                     float* grid_tmp, float* d_pos01, uint32_t* d_cell, uint16_t* d_out, int n_cus, hipStream_t stream);
void launch_density_grid_ema(uint32_t n_elements, float decay, float* grid, const float* grid_tmp, hipStream_t stream);
void launch_init_rays(const ModelParams& M, const CameraParams& C, NerfPayload* payloads, hipStream_t stream);
void launch_density_grid_to_bitfield(const uint16_t* d_grid_fp16, uint32_t n_grid, uint32_t max_cascade, float* d_grid_f32, double* d_partial,
                                     uint8_t* d_bitfield, float* out_mean, hipStream_t stream);
void launch_coarse_occupancy(const uint8_t* bitfield, uint32_t* coarse, hipStream_t stream);
void launch_accumulate_tonemap(uint32_t n_pixels, const float4* frame_buffer, float4* accumulate_buffer, float sample_count, const float* background,
                               float exposure, int to_srgb, int color_space, float4* rgba_out, hipStream_t stream);

// the frame's one-thread-a-pixel passes; L: the pixels the launch owns and the extent of every per-pixel buffer (FrameLayout, ngp_kernels.h).
// materials (nullable: no mesh owns a material, the launch is the kernel it was before materials existed): the device table of one
// MeshMaterial a mesh; with it the material instantiation runs and ids is the frame's int32 id plane (ngp_get_frame_mesh_ids)
void launch_render_mesh(const MeshSceneParams& S, const MeshShadeParams& P, const IrradianceMap& I, const IrradianceVolume* V, const IrradianceVolumeVisible* VV,
                        const CameraParams& C, const FrameLayout& L, float4* frame_buffer, float* depth_buffer, const MeshMaterial* materials, int32_t* ids,
                        hipStream_t stream); // V: the ShadeIrradianceVolume instantiation; VV: the one that weights the probes by visibility
void launch_mesh_gbuffer(const MeshSceneParams& S, const MeshShadeParams& P, const CameraParams& C, const FrameLayout& L, float* depth_buffer, float t_min, float4* gbuf,
                         float* ray_o, float* ray_d, float2* ray_t, int32_t* ids, hipStream_t stream); // M1-M4 of launch_render_mesh + the shadow-ray list
void launch_mesh_shade_deferred(const MeshShadeParams& P, const IrradianceMap& I, const IrradianceVolume* V, const IrradianceVolumeVisible* VV, const CameraParams& C,
                                const FrameLayout& L, float4* frame_buffer, const float4* gbuf, const float* ray_o, const float2* ray_t, const float4* traced, float4* record,
                                const MeshReflectionList& R, const MeshMaterial* materials, const int32_t* ids,
                                hipStream_t stream); // M5 of launch_render_mesh behind the trace(s); traced == nullptr: no shadow trace was run (T_s = 1, no record)
void launch_mesh_reflection_rays(const MeshSceneParams& S, const CameraParams& C, const FrameLayout& L, float t_min, const float4* gbuf, float* ray_o, float* ray_d,
                                 float2* ray_t, int2* hit_ids,
                                 hipStream_t stream); // the G-buffer's mirror rays (ngp_set_mesh_reflection); hit_ids (nullable): each ray's closest (mesh, triangle)
// ngp_set_mesh_reflection_meshes: M5 at the mesh hit of every cut mirror ray, on the list as launch_mesh_reflection_rays left it (before its
// prep step); hits: 2 float4 a pixel, (p2, shadow2), (C2, 1)
void launch_mesh_reflection_hit_shade(const MeshSceneParams& S, const MeshShadeParams& P, const IrradianceMap& I, const IrradianceVolume* V, const IrradianceVolumeVisible* VV,
                                      const CameraParams& C, const FrameLayout& L, const float* ray_o, const float* ray_d, const float2* ray_t, const int2* hit_ids, float4* hits,
                                      const MeshMaterial* materials, hipStream_t stream);
void launch_nerf_mesh_shadow(const MeshSceneParams& S, const MeshShadeParams& P, const ModelParams& M, const CameraParams& C, float4* frame_buffer, const float* depth_buffer,
                             const float4* nerf, float4* record, const FrameLayout& L, float strength, float bias,
                             hipStream_t stream); // the NeRF pass's composite behind the meshes' shadow on it (ngp_set_mesh_shadow_on_nerf)
// ngp_set_sun_disk: K shadow rays a pixel over the sun's disk against all meshes. On the G-buffer behind launch_mesh_gbuffer: V over plane 0's w,
// the owners' shadow-list entries rewritten, record (q, 1 + count); and launch_nerf_mesh_shadow with the blocked fraction in the boolean's place.
// wave: a pixel's rays on adjacent lanes, else one thread a pixel looping over them (the same integers)
void launch_mesh_sun_disk(const MeshSceneParams& S, const CameraParams& C, const FrameLayout& L, const SunDisk& D, bool wave, float t_min, float4* gbuf, float* ray_o,
                          float2* ray_t, float4* record, hipStream_t stream);
void launch_nerf_mesh_soft_shadow(const MeshSceneParams& S, const MeshShadeParams& P, const ModelParams& M, const CameraParams& C, float4* frame_buffer,
                                  const float* depth_buffer, const float4* nerf, float4* record, const FrameLayout& L, const SunDisk& D, bool wave, float strength, float bias,
                                  hipStream_t stream);
// ngp_set_ambient_change_on_nerf: the NeRF's normal at every owner pixel's surface point (record: 3 float4 a pixel), then g = E_after / E_before
// there, n.rgb scaled in place; launch_nerf_composite closes the frame when the meshes' shadow on the NeRF is off (f = 1, no traversal)
void launch_nerf_surface_normals(const ModelParams& M, const CameraParams& C, const FrameLayout& L, const float* depth_buffer, const float4* nerf, float4* record,
                                 hipStream_t stream);
void launch_nerf_ambient_ratio(const IrradianceVolume& after, const IrradianceVolume& before, uint32_t n_pixels, float4* nerf, float4* record, float min_irradiance,
                               float max_gain, hipStream_t stream);
void launch_nerf_composite(const CameraParams& C, float4* frame_buffer, const float4* nerf, const FrameLayout& L, hipStream_t stream);
void launch_irradiance_volume_ratio(const IrradianceVolume& after, const IrradianceVolume& before, uint32_t n, const float* positions, const float* normals, float min_irradiance,
                                    float max_gain, float4* out, hipStream_t stream);
void launch_trace_probe(const ModelParams& M, const FrameParams& F, const ProbeParams& P, int n_cus, hipStream_t stream);
void launch_probe_reduce(const ProbeParams& P, float4* envmap, hipStream_t stream);
void launch_irradiance(const ProbeParams& P, const float4* envmap, uint32_t n, const float* normals, float4* out, hipStream_t stream);
void launch_irradiance_lookup(const IrradianceMap& I, uint32_t n, const float* positions, const float* normals, float4* out, hipStream_t stream);
void launch_trace_mesh_rays(const MeshSceneParams& S, uint32_t n, float* positions, float* directions, hipStream_t stream);
void launch_ray_list_prep(const ModelParams& M, uint32_t n, const float* o, float* d, float2* t, bool normalize, hipStream_t stream);
void launch_irradiance_rays(const MeshSceneParams& S, bool occlude, uint32_t n_u, uint32_t n_v, float offset, uint64_t r0, uint32_t n, const float* positions,
                            const float* normals, float* o, float* d, float2* t, hipStream_t stream);
void launch_irradiance_reduce(uint32_t K, uint64_t r0, uint32_t n, const float4* rgba, const float2* t, float4* part, float4* out, hipStream_t stream);
void launch_irradiance_sphere_rays(const MeshSceneParams& S, bool occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* positions, float* o, float* d, float2* t,
                                   hipStream_t stream);
void launch_irradiance_sh_reduce(uint32_t n_u, uint32_t n_v, uint32_t n_probes, const float4* rgba, const float2* t, float4* out, hipStream_t stream);
void launch_irradiance_volume_lookup(const IrradianceVolume& V, uint32_t n, const float* positions, const float* normals, float4* out, hipStream_t stream);
void launch_irradiance_distance_reduce(uint32_t n_u, uint32_t n_v, uint32_t n_probes, uint32_t sharpness_log2, float D, const float2* t, float2* out, hipStream_t stream);
void launch_irradiance_volume_lookup_visible(const IrradianceVolumeVisible& A, uint32_t n, const float* positions, const float* normals, float4* out, hipStream_t stream);
void launch_irradiance_bounce_rays(const MeshSceneParams& S, const IrradianceVolume& V, const IrradianceVolumeVisible* VV, bool occlude, uint32_t n_u, uint32_t n_v, uint32_t n,
                                   const float* positions, const float* albedo, const float4* albedos, const float* alpha, float4* rgba, float2* t, hipStream_t stream); // VV: the visible lookup; albedos (nullable): one float4 a mesh instead of albedo
void launch_irradiance_volume_add(uint32_t n_float4, const float4* v0, const float4* r, float4* out, hipStream_t stream);
void launch_ray_alpha(uint32_t n, const float4* rgba, float* alpha, hipStream_t stream);
void launch_irradiance_sun_rays(const MeshSceneParams& S, bool occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* positions, const float* sun, float bias,
                                const float* source, const float4* sources, const float* alpha, float4* rgba, float2* t, hipStream_t stream); // sun: unit; source: albedo x radiance; sources (nullable): one float4 a mesh instead
void launch_irradiance_sun_shadow_rays(const MeshSceneParams& S, bool occlude, uint32_t n_u, uint32_t n_v, uint32_t n, const float* positions, const float* sun, float bias,
                                       const float* source, const float4* sources, const float* alpha, float t_min, float4* rgba, float2* t, float* o, float* d, float2* st, hipStream_t stream);
void launch_irradiance_sun_shadow_apply(uint32_t n, const float4* traced, const float* o, const float2* st, float4* rgba, float4* shadow_out, hipStream_t stream);

// marching cubes, mc_kernels.hip (ngp_mc.cpp). Wide models evaluate the lattice in chunks of `chunk` points through the caller's
// scratch (chunk x 3 floats, chunk x 4 fp16); grid models need none.
void launch_mc_density(const ModelParams& M, const McLattice& L, float* d_out, float* d_scratch_pos, uint16_t* d_scratch_net, uint32_t chunk, int n_cus, hipStream_t stream);
uint32_t mc_n_blocks(uint32_t n_points); // blocks of the count / emit kernels = entries of the block-offset array
void launch_mc_count_scan(const McGrid& G, uint2* d_blocks, unsigned long long* d_totals, hipStream_t stream);
void launch_mc_emit(const McGrid& G, const McLattice& L, const uint2* d_blocks, uint32_t* d_vofs, uint32_t* d_vmask, float* d_V, uint32_t* d_F, hipStream_t stream);
void launch_mc_vertex_inputs(const ModelParams& M, uint32_t n, const float* d_V, float* d_pos01, float* d_dir01, hipStream_t stream);
void launch_mc_vertex_attributes(const ModelParams& M, uint32_t n, const float* d_grad, const uint16_t* d_net, float* d_N, float* d_C, hipStream_t stream);

// kernel launchers, train_kernels.hip
void launch_train_generate_samples(const ModelParams& M, const TrainStepParams& P, const TrainImage* images, const TrainBatch& B, hipStream_t stream);
void launch_train_inference(const ModelParams& M, const uint4* frags, const uint32_t* counters, uint32_t max_samples, const float* coords, uint16_t* out, int n_cus,
                            hipStream_t stream);
void launch_train_loss(const ModelParams& M, const TrainStepParams& P, const TrainImage* images, const TrainBatch& B, hipStream_t stream);
void launch_train_build_fragments(const uint16_t* params, uint4* frags, uint2* kfrags, hipStream_t stream);
void launch_train_backward(const ModelParams& M, const uint4* frags, const uint2* kfrags, const uint32_t* counters, uint32_t target_batch, const float* coords,
                           const uint16_t* dloss, float* grad, uint32_t n_matrix_params, float* block_partials, int n_blocks, hipStream_t stream);
size_t train_backward_partials_floats(int n_blocks);
void launch_train_optimizer(const AdamParams& A, float* weights_fp32, uint16_t* weights, float* grad, float* m1, float* m2, uint32_t* steps, float* ema_tmp,
                            uint16_t* weights_ema, hipStream_t stream);
void launch_train_xor_layout(const ModelParams& M, const uint2* src, char* dst, hipStream_t stream);
void launch_train_loss_sum(const float* loss, uint32_t n, float* out, hipStream_t stream);
void launch_overlay_image(int width, int height, float exposure, const float* background4, const TrainImage& im, int color_space, int to_srgb, int fov_axis, float zoom, float4* out,
                          hipStream_t stream);

struct HostMesh { // MeshData (mesh.h:18-24) after load_mesh
	std::vector<Triangle> tris;        // reordered by the BVH build
	std::vector<TriangleBvhNode> nodes;
	float bmin[3], bmax[3];
	float center[3];
	ngp_mesh_material material{}; // its own material where own_material (ngp_set_mesh_material); a peer's copy follows the primary's
	bool own_material = false;
	float albedo[3] = {0.f, 0.f, 0.f}; // its own albedo in the SH9 volume's passes where own_albedo (ngp_set_mesh_albedo)
	bool own_albedo = false;
	DevArray<Triangle> d_tris; // (a peer's replica holds these alone: the host vectors stay empty, ngp_mesh.cpp sync_peer_geometry)
	DevArray<TriangleBvhNode> d_nodes;
};

// NerfDataset subset (nerf_loader.h:60-170): what rendering and the harness read
struct TrainingView {
	std::array<float, 12> xform; // ngp-space camera-to-world, column-major 4x3
	int32_t resolution[2];
	float focal_length[2];
	float principal_point[2];
	int32_t lens_mode = 0; // ELensMode
	float lens_params[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
	std::string path;
	std::string abs_path; // the image file the loader resolved (extension probing, nerf_loader.cu), may not exist
	bool white_transparent = false, black_transparent = false; // transforms.json flags (NSVF-style data), src/nerf_loader.cu:462-468
	DevArray<uint8_t> d_pixels; // training image on the device (ngp_set_training_image), RGBA
	int32_t image_type = 0;   // ngp_image_type
};
struct Dataset {
	std::vector<TrainingView> views;
	int32_t aabb_scale = 1;
	float scale = 1.0f;
	float offset[3] = {0.f, 0.f, 0.f};
	float up[3] = {0.f, 1.f, 0.f};
	bool from_mitsuba = false;
	bool is_hdr = false;
	bool has_render_aabb = false;
	float render_aabb_min[3], render_aabb_max[3];
	float render_aabb_to_local[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	int32_t n_extra_learnable_dims = 0;
};


// Everything Testbed::train touches beyond the inference model (m_trainer, m_optimizer, NerfCounters, m_rng ...)
struct TrainState {
	ngp_training_opts opts{};
	uint32_t n_params = 0, n_matrix = 0;
	DevArray<float> d_weights_fp32;      // Trainer::m_params_full_precision
	DevArray<uint16_t> d_weights;        // m_params (fp16, what the training kernels read; tcnn order: density MLP, rgb MLP, grid)
	DevArray<uint16_t> d_weights_ema;    // Ema's m_weights_ema = the inference parameters
	DevArray<float> d_ema_tmp;
	DevArray<float> d_grad;              // fp32, cleared by the optimizer kernel
	DevArray<float> d_m1;
	DevArray<float> d_m2;
	DevArray<uint32_t> d_steps;
	DevArray<uint4> d_tfrags;            // MFMA fragments of the training parameters (forward + transposed)
	DevArray<uint2> d_kfrags;
	DevArray<uint4> d_tfrags_inference;
	DevArray<uint2> d_kfrags_inference;
	DevArray<TrainImage> d_images;
	uint32_t n_images = 0;
	bool images_dirty = true;
	TrainBatch B{}; // the step in flight, a view: gen[cur]'s buffers + the shared ones below
	DevArray<uint16_t> mlp_out;
	DevArray<float> coords_compacted;
	DevArray<uint16_t> dloss;
	DevArray<float> loss;
	// sample generation only reads the images, the occupancy bitfield and the step's rng: step N+1's runs on a second
	// stream beside step N's backward pass, into the other of two buffer sets
	struct GenSet {
		DevArray<uint32_t> counters;
		DevArray<uint32_t> ray_indices;
		DevArray<float> rays;
		DevArray<uint32_t> numsteps;
		DevArray<float> coords;
		uint32_t cap_rays = 0, cap_samples = 0;
	} gen[2];
	int cur = 0;
	bool pregenerated = false; // gen[cur ^ 1] holds the next step's samples (ev_gen marks them complete)
	TrainStepParams pre_P{};
	Stream stream2;
	Event ev_gen, ev_loss;
	PinnedArray<uint32_t> h_counters; // counters[4] + loss sum
	uint32_t cap_loss = 0, cap_out = 0, cap_target = 0;
	DevArray<float> d_loss_sum;
	DevArray<float> d_partials; // per-block weight-gradient sums of train_backward_kernel
	// NerfCounters + Testbed members
	uint32_t training_step = 0;
	uint32_t rays_per_batch = 1u << 12;
	uint32_t n_rays_total = 0;
	uint32_t measured_batch_size = 0, measured_batch_size_before_compaction = 0;
	float loss_scalar = 0.f;
	Pcg32 rng{};
	uint32_t optimizer_step = 0; // Adam::m_current_step
	float lr_factor = 1.0f;      // ExponentialDecay
	bool inference_dirty = false; // the render model lags the training parameters
	bool host_params_dirty = false;
	bool batch_ready = false;
	TrainStepParams last_step{};
};

constexpr int FRAME_HISTORY = 256; // the render calls whose slot, events and flags a context keeps (ngp_ctx::HISTORY)

// ---- the frame options (Geometry frames). Three places hold an option: its settings (FrameOptions), the passes it runs (FRAME_PASSES and
// ngp_ctx::passes) and the scratch those passes share (the *Scratch groups below). ngp_render.cpp's plan_frame joins them once a call.

// The settings, as the ngp_set_* entries took them: plain data, what a peer of a multi-device context inherits with one assignment
// (ngp_mesh.cpp sync_peer_geometry). Every device then runs the options' passes over its own share of the frame.
template <typename Desc>
struct FrameOption {
	bool on = false;
	Desc desc{}; // zeros while off
};
struct FrameOptions {
	FrameOption<ngp_irradiance_sun_nerf_desc> sun_nerf_shadow;        // the NeRF in front of the frames' sun (ngp_set_sun_nerf_shadow)
	FrameOption<ngp_mesh_shadow_on_nerf_desc> mesh_shadow_on_nerf;    // the meshes in front of the sun on the NeRF (ngp_set_mesh_shadow_on_nerf)
	FrameOption<ngp_ambient_change_desc> ambient_change_on_nerf;      // what the meshes change in the ambient light on the NeRF (ngp_set_ambient_change_on_nerf)
	FrameOption<ngp_mesh_reflection_desc> mesh_reflection;            // the NeRF mirrored in the meshes (ngp_set_mesh_reflection)
	bool mesh_reflection_meshes = false;                              // ... and the meshes in it (ngp_set_mesh_reflection_meshes)
	FrameOption<ngp_sun_disk_desc> sun_disk;                          // the sun's disk (ngp_set_sun_disk)
};
// the refusals of the options' descriptors (the ngp_set_* entries; ngp_irradiance.cpp's entries that take the same descriptors)
inline void check_desc(const ngp_irradiance_sun_nerf_desc& d) {
	if (std::isnan(d.min_transmittance)) throw std::runtime_error("invalid irradiance sun NeRF descriptor: min_transmittance is NaN");
	if (!std::isfinite(d.t_min) || d.t_min < 0.0f) throw std::runtime_error("invalid irradiance sun NeRF descriptor: t_min must be finite and >= 0");
}
inline void check_desc(const ngp_mesh_shadow_on_nerf_desc& d) {
	if (!(d.strength >= 0.0f && d.strength <= 1.0f)) throw std::runtime_error("invalid mesh shadow descriptor: strength must lie in [0, 1]");
	if (!std::isfinite(d.bias) || d.bias < 0.0f) throw std::runtime_error("invalid mesh shadow descriptor: bias must be finite and >= 0");
}
inline void check_desc(const ngp_ambient_change_desc& d) {
	if (!std::isfinite(d.min_irradiance) || d.min_irradiance < 0.0f) throw std::runtime_error("invalid ambient change descriptor: min_irradiance must be finite and >= 0");
	if (!std::isfinite(d.max_gain) || d.max_gain < 1.0f) throw std::runtime_error("invalid ambient change descriptor: max_gain must be finite and >= 1");
}
inline void check_desc(const ngp_mesh_reflection_desc& d) {
	if (!std::isfinite(d.strength) || d.strength < 0.0f) throw std::runtime_error("invalid mesh reflection descriptor: strength must be finite and >= 0");
	if (std::isnan(d.min_transmittance)) throw std::runtime_error("invalid mesh reflection descriptor: min_transmittance is NaN");
	if (!std::isfinite(d.t_min) || d.t_min < 0.0f) throw std::runtime_error("invalid mesh reflection descriptor: t_min must be finite and >= 0");
}
inline void check_desc(const ngp_sun_disk_desc& d) {
	if (!std::isfinite(d.angular_radius) || d.angular_radius < 0.0f || d.angular_radius > 0.5f)
		throw std::runtime_error("invalid sun disk descriptor: angular_radius must be finite and lie in [0, 0.5] rad");
	const uint32_t k = d.n_rays;
	if (!(k == 1 || k == 2 || k == 4 || k == 8 || k == 16)) throw std::runtime_error("invalid sun disk descriptor: n_rays must be 1, 2, 4, 8 or 16");
}

// The optional passes of a frame, one row each: the bytes a pixel of the record the pass leaves, the byte the record is cleared to, what the
// pass's ngp_get_frame_*_ms does after a frame that did not run it, and the refusal of its getters after such a frame.
enum FramePassId { PASS_SUN_SHADOW, PASS_REFLECTION, PASS_REFLECTION_HITS, PASS_MESH_SHADOW, PASS_AMBIENT_CHANGE, PASS_SUN_DISK, PASS_MESH_IDS, N_FRAME_PASSES };
enum class PassMs { none, zero, refuses }; // no such getter (and no events); it returns 0; it refuses like the record's getter
struct FramePassInfo {
	uint32_t bytes;
	int fill;
	PassMs ms;
	const char* none;
};
constexpr FramePassInfo FRAME_PASSES[N_FRAME_PASSES] = {
	{16, 0, PassMs::zero, "the last frame traced no sun shadow rays (ngp_set_sun_nerf_shadow)"},         // (q, alpha_s); events around prep + trace
	{48, 0, PassMs::zero, "the last frame traced no reflection rays (ngp_set_mesh_reflection)"},         // (q, t_hit), (r, 0), (rgb_r, alpha_r); around prep + trace
	{32, 0, PassMs::zero, "the last frame shaded no reflection hits (ngp_set_mesh_reflection_meshes)"},  // (p2, shadow2), (C2, 1); around the hit shade, inside the reflection's
	{16, 0, PassMs::zero, "the last frame ran no mesh shadow pass (ngp_set_mesh_shadow_on_nerf)"},       // (p, 2 blocked / 1 open, or 1 + count / K); around the (soft) shadow kernel
	{48, 0, PassMs::zero, "the last frame ran no ambient change pass (ngp_set_ambient_change_on_nerf)"}, // (p, state), (N, W_after), (g, W_before); around normals + ratio
	{16, 0, PassMs::refuses, "the last frame ran no sun disk pass (ngp_set_sun_disk)"},                  // (q, 1 + count); around mesh_sun_disk_kernel
	{4, 0xff, PassMs::none, "the last frame ran without mesh materials (ngp_set_mesh_material)"},        // int32: the mesh of the pixel's primary hit, -1 elsewhere
};

// What a pass keeps on a device for its getters (ngp_render.cpp read_record, read_ms): the per-pixel record of the frame's last sample, events
// around the pass in that sample, and which calls of the ring ran it. A scratch group like the ones below (release, allocate, capacity).
struct FramePass {
	const FramePassInfo* info = nullptr; // its row of FRAME_PASSES (ngp_ctx's constructor)
	DevArray<char> record;
	size_t capacity = 0;
	Event ev0[FRAME_HISTORY], ev1[FRAME_HISTORY];
	bool hist[FRAME_HISTORY] = {}; // the slot's call was a frame that ran the pass
	size_t n_pixels = 0;           // pixels of the last such frame
	void release() { record.reset(); }
	void allocate(size_t n) {
		if (info->ms != PassMs::none && !ev1[FRAME_HISTORY - 1]) {
			for (int i = 0; i < FRAME_HISTORY; ++i) {
				ev0[i] = new_event();
				ev1[i] = new_event();
			}
		}
		record.reset((size_t)info->bytes * n);
	}
	float4* f4() const { return (float4*)record.get(); }
	void clear(size_t n, hipStream_t stream) const { NGP_HIP_CHECK(hipMemsetAsync(record.get(), info->fill, (size_t)info->bytes * n, stream)); }
	// around the pass; the events of a frame's last sample are the ones read_ms reads
	void begin(int slot, hipStream_t stream, bool last) const { if (last) NGP_HIP_CHECK(hipEventRecord(ev0[slot], stream)); }
	void end(int slot, hipStream_t stream, bool last) const { if (last) NGP_HIP_CHECK(hipEventRecord(ev1[slot], stream)); }
	void ran(int slot, bool on, size_t n) {
		hist[slot] = on;
		if (on) n_pixels = n;
	}
};

// a ray list for the ray-list tracer with one entry a local pixel of a frame, in the frame's pixel order and not compacted
struct RayList {
	DevArray<float> o, d;
	DevArray<float2> t;
	DevArray<float4> traced;                    // the tracer's rgba of the list
	DevArray<unsigned long long> results;       // where the trace's counters go: the slot's results stay the NeRF pass's
	void release() { o.reset(), d.reset(), t.reset(), traced.reset(); }
	void allocate(size_t n) {
		if (!results) {
			results.reset(8);
			NGP_HIP_CHECK(hipMemset(results.get(), 0, results.bytes()));
		}
		o.reset(3 * n);
		d.reset(3 * n);
		t.reset(n);
		traced.reset(n);
		// (list entries no pixel of a frame owns -- another shard's, a partial tile's -- are dead through their t alone; their o and d are never garbage)
		NGP_HIP_CHECK(hipMemset(o.get(), 0, o.bytes()));
		NGP_HIP_CHECK(hipMemset(d.get(), 0, d.bytes()));
	}
};

// The passes' scratch, grouped as the passes share it. A group owns its buffers and says how many pixels they hold; only ngp_render.cpp's
// ensure_pass_buffers allocates and releases them, by the rule written there (grow_scratch).
struct GbufferScratch { // the split mesh pass's: frames with the sun shadow, the reflection or the sun's disk fill both
	DevArray<float4> gbuf; // 3 planes: (pos, shadow), (raw normal, covered), (primary_dir, the primary ray found a triangle)
	RayList rays;          // the shadow-ray list
	size_t capacity = 0;
	void release() { gbuf.reset(), rays.release(); }
	void allocate(size_t n) { gbuf.reset(3 * n), rays.allocate(n); }
};
struct ReflectionScratch { // the reflection's
	RayList rays; // the reflection-ray list
	size_t capacity = 0;
	void release() { rays.release(); }
	void allocate(size_t n) { rays.allocate(n); }
};
struct ReflectionHitScratch { // the reflection hits'
	DevArray<int2> ids; // the (mesh, triangle) each mirror ray is cut at, (-1, -1) without a hit
	size_t capacity = 0;
	void release() { ids.reset(); }
	void allocate(size_t n) { ids.reset(n); }
};
struct NerfScratch { // the mesh shadow's and the ambient change's
	DevArray<float4> nerf; // where the NeRF launch composites instead of the frame: premultiplied (r, g, b, a), zeros where it wrote nothing
	size_t capacity = 0;
	void release() { nerf.reset(); }
	void allocate(size_t n) { nerf.reset(n); }
};
} // namespace ngp

struct ngp_ctx {
	ngp_ctx() {
		for (int i = 0; i < ngp::N_FRAME_PASSES; ++i) passes[i].info = &ngp::FRAME_PASSES[i];
	}
	int device = 0;
	int n_cus = 256;
	std::string error;
	ngp::Stream stream;

	// ---- model
	bool model_loaded = false; // uploaded to the device
	bool have_desc = false;    // parsed + validated on the host
	ngp_model_desc desc{};
	std::vector<uint16_t> params;
	std::vector<uint16_t> density_grid;
	uint32_t max_cascade = 0;
	ngp::DevArray<uint16_t> d_params; // the grid table, tcnn order
	ngp::DevArray<uint64_t> d_xgrid;  // the grid table again, in the xor layout (ngp_model.cpp build_xor_layout)
	ngp::DevArray<uint4> d_wfrags;
	ngp::DevArray<uint8_t> d_bitfield;
	ngp::DevArray<uint32_t> d_coarse;
	ngp::DevArray<float> d_density_tmp; // density_grid_tmp of update_density_grid_nerf
	uint64_t grid_rng_state = 0, grid_rng_inc = 0; // m_nerf.training.density_grid_rng
	uint32_t grid_ema_step = 0, grid_updates = 0;
	ngp::DevArray<uint16_t> d_density_f16;
	ngp::DevArray<float> d_density_f32;
	ngp::DevArray<double> d_partial;
	float bitfield_mean = 0.f;
	ngp::ModelParams M{};

	// ---- snapshot extras (src/testbed.cu:5396-5424) and dataset
	mj::Value config; // network config (+ "snapshot" on load)
	ngp_session_state session{}; // background, exposure, sun / up direction, camera scale / aperture / focus of the snapshot
	bool has_snapshot_camera = false;
	float snap_camera[12];
	float snap_relative_focal_length[2] = {1.f, 1.f};
	int32_t snap_fov_axis = 1;
	float snap_screen_center[2] = {0.5f, 0.5f};
	float snap_zoom = 1.f;
	ngp::Dataset dataset;
	std::string data_path;

	// ---- geometry mode
	std::vector<ngp::HostMesh> meshes;
	ngp::DevArray<ngp::MeshRef> d_meshrefs;
	ngp::MeshSceneParams mesh_scene{};
	// ---- mesh materials (ngp_set_mesh_material): the device table of one record a mesh, uploaded when a material or the mesh list changes
	// (ngp_mesh.cpp upload_mesh_materials); null while no mesh owns one, and frames then launch the kernels they always launched
	ngp::DevArray<ngp::MeshMaterial> d_mesh_materials;
	uint32_t n_own_materials = 0;
	uint64_t material_generation = 0, synced_material_generation = 0; // (a peer's replica follows the primary's: sync_peer_geometry)
	ngp::MeshShadeParams shade{{0.57735026f, 0.57735026f, 0.57735026f}, {0.f, 1.f, 0.f}, 0.f, 0.f, 1.f, 0.5f, 0.f, 0.f, 0.f, {0.8f, 0.8f, 0.8f}, {0.f, 0.f, 0.f}};

	// ---- irradiance probe texture(s) (m_envmap_tex / gridSize, testbed.h:949-950) and E(n) tabulated at their texels
	ngp::DevArray<float4> d_envmap;
	ngp::DevArray<float4> d_irradiance;
	uint32_t env_n_theta = 0, env_n_phi = 0;
	ngp::ProbeParams env_probe{}; // what was traced: mode, shell position(s), grid

	// ---- the SH9 irradiance volume (ngp_compute_irradiance_volume / ngp_set_irradiance_volume): data, never recomputed behind the caller
	ngp::DevArray<float4> d_sh_volume; // 7 float4 a probe, probe-major (a peer holds a replica for ShadeIrradianceVolume frames: sync_peer_geometry)
	ngp_irradiance_volume_desc sh_volume_desc{};
	// ---- its probes' distance maps (ngp_compute_irradiance_volume_visibility / ngp_set_irradiance_volume_visibility): data like the volume, dropped with it
	ngp::DevArray<float2> d_sh_visibility; // 64 float2 a probe, probe-major; empty: no visibility (a peer holds a replica like the volume's)
	ngp_irradiance_visibility_desc sh_visibility_desc{}; // max_distance holds D
	// ---- the reference SH9 volume, the scene before the meshes (ngp_compute_reference_irradiance_volume / ngp_set_reference_irradiance_volume):
	// data like d_sh_volume, without visibility maps (a peer holds a replica for ambient-change frames: sync_peer_geometry)
	ngp::DevArray<float4> d_sh_reference;
	ngp_irradiance_volume_desc sh_reference_desc{};

	// ---- environment map behind the NeRF (m_envmap.inference_view(), testbed.h:1297-1316)
	ngp::DevArray<float4> d_bg_envmap;
	int32_t bg_env_w = 0, bg_env_h = 0;

	// ---- frame
	ngp::DevArray<float4> d_frame; // (d_rgba, allocated last, holds the size of all four)
	ngp::DevArray<float> d_depth;
	ngp::DevArray<float4> d_accum;
	ngp::DevArray<float4> d_rgba;
	// a ring of per-call slots of 128 B, as 8-byte words: 0-2 accumulators [alive, hit, samples], 3 {tile queue, exited waves}, 4-7 results [alive, hit, samples, device ticks],
	// 8 start stamp, 9-12 the eight XCD queues, 13 / 14 culled tiles: accumulator and result (results[RESULT_CULL_SUM], results[RESULT_CULLED]; ngp_get_culled_tiles), 15 free.
	// Zeroed once; every launch's last wave leaves its slot's first four words zero again (nerf_kernels.hip fused_body)
	static constexpr int HISTORY = ngp::FRAME_HISTORY;
	static constexpr size_t SLOT_BYTES = 128;
	ngp::DevArray<char> d_sync;
	void bind_slot(ngp::FrameParams& F, int slot) const {
		unsigned long long* w = (unsigned long long*)(d_sync.get() + SLOT_BYTES * (size_t)slot);
		F.counters = w;
		F.queue = (uint32_t*)(w + 3);
		F.done = F.queue + 1;
		F.results = w + 4;
		F.add_results = 0;
		static const bool xcd_queues = []() { const char* e = getenv("NGP_XCD_QUEUES"); return !e || atoi(e) != 0; }(); // 0: one queue (A/B)
		F.xqueue = xcd_queues ? (uint32_t*)(w + 9) : nullptr; // bytes 72..103 of the 128-byte slot
	}
	ngp::Event ev_frame0[HISTORY], ev_frame1[HISTORY], ev_kern0[HISTORY], ev_kern1[HISTORY];
	uint64_t hist_n_rays[HISTORY] = {};
	ngp::Event ev_mesh0[HISTORY], ev_mesh1[HISTORY]; // around the mesh pass of a frame's last sample (ngp_get_mesh_pass_ms)
	bool hist_mesh_pass[HISTORY] = {};               // the slot's call was a frame with a mesh pass
	// ---- the frame options (FrameOptions, FramePass and the scratch groups above): the settings, a peer's copy of which follows the primary's
	// with the geometry, and per device the passes' records and the scratch of the passes that share it
	ngp::FrameOptions options;
	ngp::FramePass passes[ngp::N_FRAME_PASSES];
	ngp::GbufferScratch gbuffer_scratch;
	ngp::ReflectionScratch reflection_scratch;
	ngp::ReflectionHitScratch reflection_hit_scratch;
	ngp::NerfScratch nerf_scratch;
	uint64_t n_calls = 0; // render calls so far; call k uses slot k % HISTORY
	hipStream_t last_stream = nullptr;
	// Ordering between frames (any stream) and updates of what they read (render tables after training steps, the occupancy grid after a
	// refresh, peer copies into a replica) without stalling the host: an update first orders ITS stream behind every frame issued
	// since the previous update (ngp::order_after_frames: device-side waits on the frames' end events), does its work, and records
	// ev_model; every later frame orders its stream behind ev_model (ngp::order_after_model).
	uint64_t fenced_calls = 0;        // frames [0, fenced_calls) are already ordered before the last update
	ngp::Event ev_model;              // end of the last update of the render model / occupancy grid on this device
	bool ev_model_valid = false;
	ngp::Event ev_synced;             // peer: its copies out of the primary's buffers are done
	ngp::DevArray<unsigned long long> d_prof;
	ngp::DevArray<char> d_grid_scratch; // occupancy-grid refresh of a Frequency-encoding model: positions, cells, network outputs of a batch of samples (24 B each)
	ngp::DevArray<uint32_t> d_trace; // wave timelines of the diagnostic build (NGP_PROFILE_TRACE)
	static constexpr uint32_t TRACE_WAVES = 64, TRACE_ITERS = 1024;
	int32_t tune[8] = {64, 4, 32, 1, 1, 4, 1, 1}; // FrameParams::tune; changed only through validate_schedule (ngp_render.cpp)
	const char* last_render_kernel = ""; // what launch_render_nerf chose for the last frame ("": no frame yet, or one of meshes alone)

	// ---- several devices behind this context (ngp_multi.cpp): replicas on the auxiliary devices, tile gather at the primary
	std::vector<ngp_ctx*> peers;  // owned; empty for a single-device context
	ngp_ctx* primary = nullptr;   // set on a peer
	uint64_t model_generation = 0, synced_generation = 0;               // the model was replaced (set_model, snapshot)
	uint64_t grid_generation = 0, synced_grid_generation = 0;           // the occupancy grid was refreshed from the network
	uint64_t params_generation = 0, synced_params_generation = 0;       // the inference parameters followed a training step
	uint64_t mesh_generation = 0, synced_mesh_generation = 0;           // the mesh list / BVHs changed (Geometry mode)
	uint64_t probe_generation = 0, synced_probe_generation = 0;         // the irradiance probe textures were (re)computed
	uint64_t sh_volume_generation = 0, synced_sh_volume_generation = 0; // the SH9 irradiance volume or its visibility was computed, set or cleared
	uint64_t sh_reference_generation = 0, synced_sh_reference_generation = 0; // the reference SH9 volume was computed, set or cleared
	ngp::DevArray<float4> d_pack_rgba;   // this device's tiles of the current frame, tile-packed
	ngp::DevArray<float> d_pack_depth;   // (allocated last: its size is that of both)
	ngp::DevArray<float4> d_gather_rgba; // primary: [device][slots * 64]
	ngp::DevArray<float> d_gather_depth; // (allocated last: its size is that of both)
	ngp::Event ev_pack, ev_unpacked;
	uint64_t n_multi_frames = 0;
	bool last_was_multi = false; // the last frame was rendered over all devices (ngp_get_render_stats sums the shares)
	bool streams_mixed = false; // frames were issued on more than one stream since the last device-wide wait

	// ---- the last marching-cubes mesh (ngp_mc.cpp), ngp space; N / C empty for a mesh of a caller's lattice
	std::vector<float> mc_V, mc_N, mc_C;
	std::vector<uint32_t> mc_F;
	bool mc_valid = false, mc_attrs = false;
	float sh_bounce_ms = 0.f; // device time of the last bounce pass over the SH9 volume's probes (ngp_get_irradiance_bounce_ms)
	float sh_sun_ms = 0.f;    // device time of the last sun pass over them (ngp_get_irradiance_sun_ms)
	float sh_sun_shadow_ms = 0.f; // of it, the shadow rays through the NeRF: prep and trace (ngp_get_irradiance_sun_shadow_ms); 0 after a pass without them
	float mc_ms[3] = {0.f, 0.f, 0.f}; // device time of the last ngp_compute_marching_cubes_mesh: lattice, marching cubes, normals + colours

	// ---- training (ngp_train.cpp)
	std::unique_ptr<ngp::TrainState> train;
	bool density_grid_host_dirty = false; // ctx->density_grid lags d_density_f32
};

namespace ngp {
// ------------------------------------------------------------------------------------------------ helpers
// Preconditions of the entry points that run on the GPU. The messages reach callers (ngp_last_error); `needs` says what cannot run.
inline void require_device(const ngp_ctx* ctx, const char* needs = nullptr) {
	if (ctx->device < 0)
		throw std::runtime_error(std::string("this context has no HIP device (host-only); ") + (needs ? std::string(needs) + " -- " : std::string()) + "there is no CPU fallback");
}
inline void require_model(const ngp_ctx* ctx, const char* needs = nullptr) {
	require_device(ctx, needs);
	if (!ctx->model_loaded) throw std::runtime_error("No network available.");
}

template <typename F>
inline int guarded(ngp_ctx* ctx, F&& f) {
	if (!ctx) return -1;
	try {
		if (ctx->device >= 0) NGP_HIP_CHECK(hipSetDevice(ctx->device));
		f();
		ctx->error.clear();
		return 0;
	} catch (const std::exception& e) {
		ctx->error = e.what();
		return -1;
	}
}

inline std::string read_file(const std::string& path) {
	std::ifstream f(path, std::ios::in | std::ios::binary);
	if (!f) throw std::runtime_error("cannot open '" + path + "'");
	std::stringstream ss;
	ss << f.rdbuf();
	return ss.str();
}

inline bool file_exists(const std::string& p) {
	struct stat st;
	return stat(p.c_str(), &st) == 0;
}
inline bool is_directory(const std::string& p) {
	struct stat st;
	return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
inline std::string parent_dir(const std::string& p) {
	size_t k = p.find_last_of('/');
	return k == std::string::npos ? std::string(".") : p.substr(0, k);
}
inline bool ends_with_ci(const std::string& s, const std::string& suffix) {
	if (s.size() < suffix.size()) return false;
	for (size_t i = 0; i < suffix.size(); ++i)
		if (tolower(s[s.size() - suffix.size() + i]) != tolower(suffix[i])) return false;
	return true;
}


inline void order_after_frames(ngp_ctx* ctx, hipStream_t stream) {
	const uint64_t pending = ctx->n_calls - ctx->fenced_calls, n = pending < (uint64_t)ngp_ctx::HISTORY ? pending : (uint64_t)ngp_ctx::HISTORY;
	for (uint64_t k = 0; k < n; ++k) NGP_HIP_CHECK(hipStreamWaitEvent(stream, ctx->ev_frame1[(ctx->n_calls - 1 - k) % ngp_ctx::HISTORY], 0));
	ctx->fenced_calls = ctx->n_calls;
}
inline void mark_model_updated(ngp_ctx* ctx, hipStream_t stream) {
	if (!ctx->ev_model) ctx->ev_model = new_event(hipEventDisableTiming);
	NGP_HIP_CHECK(hipEventRecord(ctx->ev_model, stream));
	ctx->ev_model_valid = true;
}
inline void order_after_model(ngp_ctx* ctx, hipStream_t stream) {
	if (ctx->ev_model_valid) NGP_HIP_CHECK(hipStreamWaitEvent(stream, ctx->ev_model, 0));
}

// frame tiles of 8 x 8 pixels dealt round-robin to `count` shards: how many of them shard `index` renders
inline uint32_t tile_share(int32_t width, int32_t height, uint32_t index, uint32_t count) {
	const uint32_t tiles = (uint32_t)((width + 7) / 8) * (uint32_t)((height + 7) / 8);
	return tiles > index ? (tiles - index + count - 1) / count : 0;
}

// numbers out of untrusted files: a double that does not fit the integer type must not reach the cast (undefined behaviour); out-of-range values
// become ones that every later validation refuses
inline uint32_t to_u32(double v) { return v >= 0.0 && v < 4294967296.0 ? (uint32_t)v : 0xffffffffu; }
inline int to_int(double v) { return v > -2147483648.0 && v < 2147483648.0 ? (int)v : (v < 0.0 ? -2147483647 - 1 : 2147483647); }

// ngp_model.cpp
void set_model_impl(ngp_ctx* ctx, const ngp_model_desc& d); // validates the descriptor, then replaces the context's model
void free_model(ngp_ctx* ctx);
void update_density_grid_device(ngp_ctx* ctx, float decay, uint32_t n_uniform, uint32_t n_nonuniform, uint32_t n_iterations);
void refresh_density_grid_host(ngp_ctx* ctx);
// ngp_snapshot.cpp
void load_snapshot_path(ngp_ctx* ctx, const std::string& path);
uint16_t float_to_half(float f);
void read_vec(const mj::Value& v, float* out, size_t n);
// ngp_render.cpp
void schedule_from_env(ngp_ctx* ctx);
void ensure_frame_buffers(ngp_ctx* ctx, size_t n_pixels); // (0: the per-call slots and events alone)
CameraParams make_camera_params(const ngp_camera& cam, uint32_t spp_index);
void render_frames(ngp_ctx* ctx, const ngp_camera& cam, const ngp_render_opts& opts, float4* d_rgba, float* d_depth, hipStream_t stream);
// ngp_irradiance.cpp: the ray-list tracer as a frame uses it (TracerCall, there, adds the slot bookkeeping of a call of its own)
void require_probe_model(ngp_ctx* ctx, const char* what); // the models the tracer serves; `what` names the caller's work in the refusal
void tracer_frame_params(const ngp_ctx* ctx, int slot, float min_transmittance, FrameParams& F);
ProbeParams ray_list_params(uint32_t n, const float* o, const float* dir, const float2* t, float4* rgba, float* depth);
void launch_probe_trace(const ngp_ctx* ctx, const ModelParams& M, FrameParams& F, const ProbeParams& P, bool add_results, hipStream_t stream); // clears P's outputs, then one persistent launch
// ngp_train.cpp
void free_training(ngp_ctx* ctx);
bool probe_image_size(const std::string& path, int& width, int& height);
void sync_inference_model(ngp_ctx* ctx); // render what has been trained (no-op when nothing changed)
void sync_host_params(ngp_ctx* ctx);     // ctx->params <- training parameters, for snapshots
// ngp_multi.cpp
void render_frames_multi(ngp_ctx* ctx, const ngp_camera& cam, const ngp_render_opts& opts, float4* d_rgba, float* d_depth, hipStream_t stream);
// ngp_mesh.cpp: Geometry mode on an auxiliary device -- the primary's meshes (BVHs as built), shading parameters, irradiance tables and the SH9 volume
void sync_peer_geometry(ngp_ctx* primary, ngp_ctx* peer);
// what ngp_irradiance.cpp computes, as the kernels take it (the render and the peer sync read these too)
inline IrradianceMap irradiance_map_of(const ngp_ctx* ctx) {
	IrradianceMap I{};
	I.irradiance = ctx->d_irradiance.get();
	I.n_theta = ctx->env_n_theta;
	I.n_phi = ctx->env_n_phi;
	if (ctx->env_probe.mode == 3) {
		I.grid_x = ctx->env_probe.grid_x;
		I.grid_y = ctx->env_probe.grid_y;
	}
	for (int i = 0; i < 3; ++i) I.center[i] = ctx->env_probe.center[i];
	return I;
}
// texels of the context's probe texture(s): a grid holds grid_x * grid_y textures back to back
inline size_t env_texels(const ngp_ctx* ctx) {
	const ProbeParams& P = ctx->env_probe;
	return (size_t)P.n_theta * P.n_phi * (P.mode == 3 ? P.grid_x * P.grid_y : 1u);
}
// the lattice of d over the records sh (device, 7 float4 a probe)
inline IrradianceVolume irradiance_volume_from(const ngp_irradiance_volume_desc& d, const float4* sh) {
	IrradianceVolume V{};
	V.sh = sh;
	for (int a = 0; a < 3; ++a) {
		V.res[a] = d.res[a];
		V.lo[a] = d.aabb_min[a];
		V.hi[a] = d.aabb_max[a];
	}
	return V;
}
inline IrradianceVolume sh_volume_of(const ngp_ctx* ctx) { return irradiance_volume_from(ctx->sh_volume_desc, ctx->d_sh_volume.get()); }
inline IrradianceVolume sh_reference_of(const ngp_ctx* ctx) { return irradiance_volume_from(ctx->sh_reference_desc, ctx->d_sh_reference.get()); }
inline IrradianceVolumeVisible sh_volume_visible_of(const ngp_ctx* ctx) {
	IrradianceVolumeVisible A{};
	A.V = sh_volume_of(ctx);
	A.maps = ctx->d_sh_visibility.get();
	A.D = ctx->sh_visibility_desc.max_distance;
	A.normal_bias = ctx->sh_visibility_desc.normal_bias;
	return A;
}
} // namespace ngp
