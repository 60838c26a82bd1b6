/*
 * libngp_hip.so -- C ABI of the MI355X-native NeRF volume renderer.
 *
 * The reference (fnysalehi/Surface-Irradiance-Estimation-from-Neural-Radiance-Fields) has no FFI seam:
 * its public surface is the C++ class ngp::Testbed (include/neural-graphics-primitives/testbed.h)
 * re-exported by pybind11 (src/python_api.cu). This header is the seam the build inserts UNDER that
 * class: every entry point names the Testbed member (file:line in the reference) it replaces. Plain
 * pointers and sizes only; no exceptions cross the boundary (0 = ok, otherwise ngp_last_error()).
 *
 * Threading: a context is not re-entrant -- one host thread per context. All inputs are copied during
 * the call; no borrowed pointer survives a call.
 */
#ifndef NGP_HIP_H
#define NGP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGP_API __attribute__((visibility("default")))

typedef struct ngp_ctx ngp_ctx;

enum ngp_activation { NGP_ACT_NONE = 0, NGP_ACT_RELU = 1, NGP_ACT_LOGISTIC = 2, NGP_ACT_EXPONENTIAL = 3 };

/* ERenderMode subset (common.h:58-72). Only Shade is on the hot path; AO..Cost are "next" (SURVEY 8f-3). */
/* ELensMode, common.h:223-230 */
enum ngp_lens_mode { NGP_LENS_PERSPECTIVE = 0, NGP_LENS_OPENCV = 1, NGP_LENS_FTHETA = 2, NGP_LENS_LATLONG = 3, NGP_LENS_OPENCV_FISHEYE = 4, NGP_LENS_EQUIRECTANGULAR = 5 };

enum ngp_render_mode {
	NGP_RENDER_SHADE = 0,
	NGP_RENDER_SHADE_ENVMAP = 1, /* ERenderMode::ShadeEnvMap: meshes lit by the NeRF-derived irradiance probe (ngp_compute_envmap) */
	/* G-buffer modes of composite_kernel_nerf (src/testbed_nerf.cu:689-702): the per-sample colour is replaced, the compositing is unchanged,
	 * and shade_kernel_nerf skips the sRGB -> linear conversion (:1393). NeRF mode only. */
	NGP_RENDER_AO = 2,        /* rgb = alpha of the sample */
	NGP_RENDER_POSITIONS = 3, /* rgb = (pos - 0.5) / 2 + 0.5 */
	NGP_RENDER_DEPTH = 4,     /* rgb = dot(cam_fwd, pos - ray origin) * depth_scale */
	NGP_RENDER_COST = 5,      /* ERenderMode::Cost (shade_kernel_nerf :1382-1384): grey = samples composited on the ray / 128, opaque. The reference's
	                           * payload.n_steps holds that count for rays that saturate and the last compaction batch's for rays that leave the
	                           * volume (:466, :730); here it is the ray's total in both cases */
	NGP_RENDER_NORMALS = 7,   /* ERenderMode::Normals (composite_kernel_nerf :688-693, shade_kernel_nerf :1379-1381): every sample's colour is the unit
	                           * vector opposite to the density's gradient w.r.t. the position -- tcnn's input_gradient (src/testbed_nerf.cu:2106-2107):
	                           * a backward pass through the density MLP and the grid encoding per sample; the pixel is (0.5 n + 0.5) alpha. Grid models. */
	NGP_RENDER_SHADE_GRID_ENVMAP = 6, /* ERenderMode::ShadeGridEnvMap, the fork's default (testbed.h:880): meshes lit by the GRID of NeRF-derived
	                           * irradiance probes (ngp_compute_envmap_grid), position-dependent */
	NGP_RENDER_SHADE_IRRADIANCE_VOLUME = 8 /* this project's own: in Geometry mode every mesh pixel's ambient light is max(E(p, N), 0) / pi per channel, E the
	                           * SH9 irradiance volume's estimate (ngp_irradiance_volume_at) at the hit point p for the shading normal N = the hit
	                           * triangle's unit normal as the table modes use it, not face-forwarded. The clamp is there because nine coefficients
	                           * ring: E can dip below zero on the far side of a bright lobe. Where every probe around p is dead (W = 0) the
	                           * ambient light is 0. A hit point outside the volume's box is clamped onto it per axis (the lookup's rule). Sun,
	                           * shadow ray, BRDF, depth, coverage, sharding and packing are those of the other shade modes; ambientcolor and up_dir
	                           * are not used. While the context holds probe visibility (ngp_compute_irradiance_volume_visibility) E is the
	                           * visible lookup's (ngp_irradiance_volume_at_visible). Refused with meshes present and no volume ("needs ngp_compute_irradiance_volume or
	                           * ngp_set_irradiance_volume first"), on a multi-device context too: its auxiliary devices keep replicas of the
	                           * records, refreshed when the volume is computed, set or cleared. Without meshes, or in NGP_MODE_NERF, it is Shade */
};

/* ETestbedMode subset (common.h:35-43): Nerf, and the fork's Geometry mode (meshes + NeRF, depth composited) */
enum ngp_testbed_mode { NGP_MODE_NERF = 0, NGP_MODE_GEOMETRY = 1 };

/* What Testbed::reset_network (src/testbed.cu:3844-4212) + load_nerf_post (src/testbed_nerf.cu:2652-2739)
 * + the snapshot (src/testbed.cu:5285-5463) leave behind for rendering. */
typedef struct ngp_model_desc {
	/* tcnn HashGrid encoding */
	uint32_t n_levels;
	uint32_t n_features_per_level;
	uint32_t log2_hashmap_size; /* 31 = tcnn DenseGrid: no level is ever hashed or capped */
	uint32_t base_resolution;
	float per_level_scale; /* explicit: the fork derives it with aabb_scale = 1, src/testbed.cu:3959-3966 */
	/* tcnn FullyFusedMLP / CutlassMLP density and rgb heads (nerf_network.h:81-101). Grid architecture: n_hidden_density 1 with
	 * n_hidden_rgb 0..3 (configs/nerf/base_0layer .. base_3layer.json; base.json: 2), or both 0 (linear.json). A head without a
	 * hidden layer is tcnn's CutlassMLP with one (padded output) x (input) matrix. */
	uint32_t n_neurons;
	uint32_t n_hidden_density;
	uint32_t n_hidden_rgb;
	uint32_t density_out_dims;
	uint32_t rgb_activation;     /* ngp_activation */
	uint32_t density_activation; /* ngp_activation */
	/* Trainer::serialize "params_binary": density MLP, rgb MLP, grid (nerf_network.h:356-371), fp16 */
	const uint16_t* params_fp16;
	uint64_t n_params;
	/* snapshot "density_grid_binary": (max_cascade+1) x 128^3 fp16, Morton order (src/testbed.cu:5339-5347) */
	const uint16_t* density_grid_fp16;
	uint64_t n_density_grid;
	float aabb_min[3], aabb_max[3];               /* m_aabb */
	float render_aabb_min[3], render_aabb_max[3]; /* m_render_aabb */
	float render_aabb_to_local[9];                /* column-major mat3 */
	uint32_t aabb_scale;                          /* dataset.aabb_scale -> max_cascade, src/testbed_nerf.cu:2729-2732 */
	float cone_angle_constant;                    /* src/testbed_nerf.cu:2736 */
	int32_t linear_colors;                        /* m_nerf.training.linear_colors */
	/* The second architecture the renderer implements: configs/nerf/frequency.json, the original NeRF's network (tcnn Frequency
	 * encodings, CutlassMLPs 128 or 256 wide with any number of hidden layers). All zero = the grid architecture above.
	 *   pos_encoding  0: the grid encoding described by the fields above; 1: Frequency with pos_n_frequencies (the grid fields are
	 *                 ignored, params_fp16 holds the two MLPs only); 2: Identity (configs/nerf/none.json: the position itself, padded
	 *                 with ones to mlp_alignment)
	 *   dir_encoding  0: SphericalHarmonics degree 4; 1: Frequency with dir_n_frequencies; 2: Identity (with pos_encoding 1 or 2)
	 *   mlp_alignment 16: FullyFusedMLP, 8: CutlassMLP (0 = 16) -- what encodings, the rgb network's input and its output are padded
	 *                 to (nerf_network.h:81-100). For the grid architecture it is the RGB network's alignment (:83): 8 makes the rgb
	 *                 output layer 8 rows (linear.json, base_0layer.json)
	 * Inference only: ngp_train_* refuse such a model. */
	uint32_t pos_encoding, pos_n_frequencies;
	uint32_t dir_encoding, dir_n_frequencies;
	uint32_t mlp_alignment;
} ngp_model_desc;

/* Arguments of Testbed::render_frame (testbed.h:561-575) that the NeRF path consumes. */
typedef struct ngp_camera {
	float matrix[12];       /* camera-to-world 4x3 column-major (m_camera) */
	int32_t width, height;
	float focal_length[2];  /* pixels: calc_focal_length, src/testbed.cu:4474-4476 */
	float screen_center[2]; /* render_screen_center */
	uint32_t spp_index;     /* render_buffer.spp() */
	int32_t snap_to_pixel_centers;
	float near_distance;    /* m_render_near_distance */
	/* m_nerf.render_lens when m_nerf.render_with_lens_distortion (uv_to_ray, common_device.cuh:416-483): ngp_lens_mode +
	 * parameters (OpenCV: k1 k2 p1 p2; OpenCVFisheye: k1 k2 k3 k4; FTheta: r0..r4 of the angle polynomial, then the resolution
	 * x, y the intrinsics refer to -- f_theta_undistortion, common_device.cuh:361-375). All zero = perspective. */
	int32_t lens_mode;
	float lens_params[7];
	/* depth of field (uv_to_ray, common_device.cuh:471-477): m_aperture_size and the focus distance plane_z = m_slice_plane_z + m_scale
	 * (src/testbed_nerf.cu:2342); aperture_size 0 or focus_z < 0 = pinhole */
	float aperture_size, focus_z;
	/* camera_matrix1 and rolling_shutter of Testbed::render_frame (testbed.h:561-575): when has_matrix1 is set and matrix1 differs
	 * from matrix (= camera_matrix0), every pixel is rendered by the camera of its own time
	 *   t = rolling_shutter[0] + [1] u + [2] v + [3] ld_random_val(spp_index, pixel * 72239731),  camera_slerp(matrix, matrix1, t)
	 * (get_xform_given_rolling_shutter, common_device.cuh:651-659; src/testbed_nerf.cu:1468) and depth is measured along matrix1.
	 * rolling_shutter (0, 0, 0, 1) -- what Testbed::render passes -- is motion blur over the whole interval. NeRF mode. */
	int32_t has_matrix1;
	float matrix1[12];
	float rolling_shutter[4];
} ngp_camera;

typedef struct ngp_render_opts {
	int32_t render_mode;      /* ngp_render_mode */
	float min_transmittance;  /* m_nerf.render_min_transmittance */
	float background[4];      /* m_background_color (sRGB, straight) */
	float exposure;           /* m_exposure */
	int32_t to_srgb;          /* !linear of Testbed::render (python_api.cu:124,189) */
	int32_t spp;              /* samples accumulated by ngp_render */
	/* camera-tile sharding across GPUs: this context renders 8x8-pixel tiles t with t % shard_count == shard_index */
	uint32_t shard_index, shard_count;
	int32_t testbed_mode;     /* ngp_testbed_mode: Geometry = render_geometry_mesh then render_geometry_nerf (src/testbed.cu:4833-4889) */
	/* 0: rgba/depth are W*H images (pixel x + W*y). 1: tile-packed -- only this shard's tiles, local tile q (global tile
	 * shard_index + q*shard_count, tiles numbered row-major over ceil(W/8) x ceil(H/8)) occupies pixels [64q, 64q+64),
	 * slot (x&7) + 8*(y&7); buffers hold 64 * ngp_packed_tiles(...) pixels. This is the layout the per-frame RCCL
	 * all_gather moves, so no pack pass is needed on the sending side. */
	int32_t packed_output;
	float depth_scale;        /* NGP_RENDER_DEPTH: 1 / dataset scale in the reference (src/testbed_nerf.cu:2478); 0 selects 1 / 0.33 (NERF_SCALE) */
	int32_t color_space;      /* EColorSpace in which samples are averaged and the background is blended: 0 Linear, 1 SRGB
	                           * (accumulate_kernel / tonemap_kernel, src/render_buffer.cu:241-248, 324-340, 537-541; run.py --nerf_compatibility) */
} ngp_render_opts;

/* BRDFParams (common.h:167-177) + m_sun_dir / m_up_dir (testbed.h:875-876) used by shade_kernel_mesh_geometry */
typedef struct ngp_geometry_opts {
	float sun_dir[3], up_dir[3];
	float metallic, subsurface, specular, roughness, sheen, clearcoat, clearcoat_gloss;
	float basecolor[3], ambientcolor[3];
} ngp_geometry_opts;

typedef struct ngp_render_stats {
	uint64_t n_rays;
	uint64_t n_rays_alive_after_init;
	uint64_t n_rays_hit;
	uint64_t n_samples;      /* network queries composited */
	float kernel_ms;         /* duration of the fused march/encode/MLP/composite kernel, HIP events on its stream */
	float frame_ms;          /* whole frame on the device (clear .. tonemap), HIP events */
	float kernel_device_ms;  /* the fused kernel from its first wave's start to its last wave's exit, read inside the kernel from the chip's
	                          * 100 MHz clock (s_memrealtime): unlike the HIP events it does not include the time a launch waits for CUs
	                          * behind another frame's kernel when frames overlap on several streams */
} ngp_render_stats;

/* --- lifetime: Testbed::Testbed / ~Testbed (testbed.h:80-95). device = HIP device ordinal; -1 creates a host-only
 * context that can read/validate/write the file formats but cannot render (there is no CPU renderer). NULL on failure. */
NGP_API ngp_ctx* ngp_create(int device);
/* Several GPUs behind one context: Testbed's device list (m_devices, src/testbed.cu:5490-5616 -- a replica per device kept in step
 * by sync_device, auxiliary devices render on their own streams, peer copies return frame + depth to the primary). devices[0] is
 * the primary; every other call takes the returned context as if it had one device. ngp_render / ngp_render_device deal the camera's
 * 8x8 tiles round-robin to the devices, each renders its share tile-packed and pushes it to device 0 (hipMemcpyPeerAsync over xGMI),
 * which scatters the tiles into the image; nothing waits on the host. NeRF mode. The same ordinal may be listed twice (a rehearsal
 * of the path on one GPU). NULL on failure. */
NGP_API ngp_ctx* ngp_create_multi(const int* devices, int n_devices);
NGP_API int ngp_n_devices(const ngp_ctx* ctx);
NGP_API void ngp_destroy(ngp_ctx* ctx);
NGP_API const char* ngp_last_error(const ngp_ctx* ctx);
NGP_API const char* ngp_version(void);

/* --- model: Testbed::reset_network + Trainer::deserialize (src/testbed.cu:3844,5428-5433) */
NGP_API int ngp_set_model(ngp_ctx* ctx, const ngp_model_desc* desc);
/* Testbed::load_snapshot(std::istream&, bool is_compressed) (src/testbed.cu:5477-5488): msgpack, optionally zlib (.ingp) */
NGP_API int ngp_load_snapshot(ngp_ctx* ctx, const void* bytes, size_t n_bytes, int is_compressed);
/* Testbed::load_snapshot(const fs::path&) (src/testbed.cu:5465-5475) */
NGP_API int ngp_load_snapshot_file(ngp_ctx* ctx, const char* path);
/* Testbed::save_snapshot (src/testbed.cu:5219-5283), inference state only */
NGP_API int ngp_save_snapshot_file(ngp_ctx* ctx, const char* path, int compress);
/* the model as currently loaded, trained parameters and a refreshed occupancy grid included; params_fp16 / density_grid_fp16 point at the
 * context's own host copies (read-only, valid until the next call that changes the model) */
NGP_API int ngp_get_model(ngp_ctx* ctx, ngp_model_desc* out);
/* session state a snapshot carries beside the model and the camera (save_snapshot / load_snapshot, src/testbed.cu:5245-5263,
 * 5395-5418): m_background_color, m_exposure, m_sun_dir, m_up_dir, camera scale / aperture_size / autofocus_depth (= m_slice_plane_z).
 * get: what the loaded snapshot held (valid = 0 when nothing was loaded); set: what the next ngp_save_snapshot_file writes,
 * together with the camera (matrix12 may be NULL to leave the camera as it is). */
typedef struct ngp_session_state {
	int32_t valid;
	float background_color[4];
	float exposure;
	float sun_dir[3], up_dir[3];
	float camera_scale, aperture_size, autofocus_depth;
} ngp_session_state;
NGP_API int ngp_get_session_state(const ngp_ctx* ctx, ngp_session_state* out);
NGP_API int ngp_set_session_state(ngp_ctx* ctx, const ngp_session_state* state, const float* matrix12, const float* relative_focal_length2, int32_t fov_axis,
                                  const float* screen_center2, float zoom);
/* camera stored in the snapshot: m_camera, relative focal length, fov axis, screen center, zoom */
NGP_API int ngp_get_snapshot_camera(const ngp_ctx* ctx, float* matrix12, float* relative_focal_length2, int32_t* fov_axis, float* screen_center2, float* zoom);

/* --- data: Testbed::load_training_data (src/testbed.cu:125-152) -> ngp::load_nerf (src/nerf_loader.cu:273):
 * camera metadata of a transforms.json (or a directory of them); images are not decoded (inference path). */
NGP_API int ngp_load_training_data(ngp_ctx* ctx, const char* path);
NGP_API int ngp_n_training_views(const ngp_ctx* ctx);
/* per-view: ngp-space camera matrix (nerf_matrix_to_ngp applied), resolution, focal length (pixels), principal point */
NGP_API int ngp_get_training_view(const ngp_ctx* ctx, int view, float* matrix12, int32_t* resolution2, float* focal_length2, float* principal_point2);
/* the view's lens (read_lens, src/nerf_loader.cu:175-240): ngp_lens_mode and 7 parameters */
NGP_API int ngp_get_training_view_lens(const ngp_ctx* ctx, int view, int32_t* lens_mode, float* lens_params7);
NGP_API int ngp_get_dataset_info(const ngp_ctx* ctx, int32_t* aabb_scale, float* scale, float* offset3, int32_t* is_hdr);

/* --- render: Testbed::render_frame (src/testbed.cu:4694-4721) = clear + render_nerf (src/testbed_nerf.cu:2328-2488)
 * + accumulate/tonemap (src/render_buffer.cu:631-694) for opts->spp samples, then the copy that
 * Testbed::render_to_cpu (src/python_api.cu:197-201) does. rgba_out: host, H*W*4 floats, premultiplied alpha.
 * depth_out (nullable): host, H*W floats. */
NGP_API int ngp_render(ngp_ctx* ctx, const ngp_camera* cam, const ngp_render_opts* opts, float* rgba_out, float* depth_out);
/* Page-locked host memory for images, pooled by size (thread-safe; usable before any context exists). ngp_render copies
 * into such a buffer with one DMA at the link's rate; into ordinary memory the runtime stages the copy (about 2.5x slower for
 * a 1080p frame). pyngp's Testbed.render returns arrays that own such buffers. No counterpart in the reference (its
 * render_to_cpu reads back from a CUDA array, src/python_api.cu:197-201). */
NGP_API void* ngp_host_alloc(size_t bytes);
NGP_API void ngp_host_free(void* p);
/* Same frame, results left in device memory (d_rgba: W*H*4 floats, d_depth nullable: W*H floats) and enqueued on
 * `stream` (a hipStream_t, NULL = default stream) without synchronising: for callers that keep the image on the GPU
 * (RCCL gather of tiles, benchmarks). */
NGP_API int ngp_render_device(ngp_ctx* ctx, const ngp_camera* cam, const ngp_render_opts* opts, void* d_rgba, void* d_depth, void* stream);
/* number of local tiles (hence 64x that many pixels) of a tile-packed frame */
NGP_API uint32_t ngp_packed_tiles(int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count);
/* counters + timings of the last ngp_render / ngp_render_device (synchronises the stream) */
NGP_API int ngp_get_render_stats(ngp_ctx* ctx, ngp_render_stats* out);
/* duration of the mesh pass (render_mesh_fused) of the last frame's last sample, HIP events on its stream; refused when that frame had none */
NGP_API int ngp_get_mesh_pass_ms(ngp_ctx* ctx, float* ms_out);
/* per device of a multi-device context (0 = primary): the last frame's counters and timings of that device's share */
NGP_API int ngp_get_device_render_stats(ngp_ctx* ctx, int device_index, ngp_render_stats* out);
/* the same for the last n calls (oldest first; the context keeps 256), read once after a batch of asynchronous
 * ngp_render_device calls so that measuring does not serialise them */
NGP_API int ngp_get_render_history(ngp_ctx* ctx, int n, ngp_render_stats* out);
/* Which render kernel the last ngp_render / ngp_render_device of this context launched (for a multi-device context: the primary's share):
 * "render_nerf_fused" (any box, any camera), "render_nerf_fused_unit" / "_unit_plain" (aabb_scale 1; plain = pinhole, no aperture, no
 * environment map), "_c5" / "_c5_plain" (aabb_scale up to 16, render box inside the grid), "_mid0" / "_mid2" / "_lin_rgb" / "_lin" (an rgb
 * head with 1 / 3 hidden layers; an rgb head, or both heads, without one), "_normals", the stamped diagnostic twins "_prof" / "_unit_plain_prof" /
 * "_unit_plain_prof2", or "wide" (Frequency / Identity encodings). "" before the first frame and after a frame of meshes alone. The string
 * is static. Recorded on the host where the launch is chosen; tests use it to assert that a frame exercised the kernel they mean. */
NGP_API const char* ngp_last_render_kernel(ngp_ctx* ctx);
/* How many 8 x 8 camera tiles of the last ngp_render / ngp_render_device (summed over its samples per pixel; the primary's share) the
 * unit render kernels dropped right after ray setup because no ray of the tile can meet an occupied cell (csrc/tile_probe.h). Such a tile
 * shows the empty pixel it would have shown anyway: frames and ngp_render_stats do not depend on the cull. 0 after any other kernel and in
 * a library built without the cull. Synchronises the stream. */
NGP_API int ngp_get_culled_tiles(ngp_ctx* ctx, uint64_t* out);

/* Scheduling of the persistent render kernel: knobs[0..n) = refill_min [16,64], skip_steps [1,64], go_min [1,64], max_stall [0,64],
 * samples a ray may emit per round while most of a wave's ray slots are live [1,8], at most once fewer are [1,8] (the reference's n_steps
 * between two compactions, src/testbed_nerf.cu:2080-2086), block_jumps {0,1}, share {0,1} (a wave that has run out of work takes over half
 * the rays of a busy wave of its workgroup). Performance only, except block_jumps: 1 (default) leaves empty 4^3 / 16^3 blocks of the occupancy grid in
 * one step, 0 walks them voxel by voxel exactly as if_unoccupied_advance_to_next_occupied_voxel (nerf_device.cuh:461-494) does.
 * Out-of-range values are refused (they would hang the kernel). No counterpart in the reference; the environment variable
 * NGP_TUNE sets the same list at ngp_create. */
NGP_API int ngp_set_schedule(ngp_ctx* ctx, const int32_t* knobs, int n);
/* Diagnostic, no counterpart in the reference: with NGP_PROFILE_SECTIONS=1|2 and NGP_PROFILE_TRACE=<stride> in the environment the render
 * kernel's stamped twin records the timeline of every stride-th wave that was dealt rays (one record per loop round: s_memtime at the
 * top of the round and after refill / march / network / composite, what the round carried). Copies the last frame's trace
 * (n_words 32-bit words at most; layout: csrc/ngp_kernels.h FrameParams::trace, decoder tools/wave_trace.py); out == NULL only
 * reports the capacities. */
NGP_API int ngp_get_profile_trace(ngp_ctx* ctx, uint32_t* out, uint64_t n_words, uint32_t* cap_waves, uint32_t* cap_iters);

/* --- stage entry points (what the reference launches as separate kernels; used by parity tests and tools)
 * K5a tcnn GridEncoding::inference (call site nerf_network.h:113-118): host pos01 n x 3 -> host fp16 n x (L*F) */
NGP_API int ngp_grid_encode(ngp_ctx* ctx, uint32_t n, const float* pos01, uint16_t* out_fp16);
/* tcnn DifferentiableObject::input_gradient(stream, 3, ...) as ERenderMode::Normals calls it (src/testbed_nerf.cu:2106-2107): d density
 * logit / d position for n positions, host n x 3 floats. Grid models. */
NGP_API int ngp_density_gradient(ngp_ctx* ctx, uint32_t n, const float* pos01, float* out_grad);
/* K5 NerfNetwork::inference_mixed_precision (nerf_network.h:105-139): pos01/dir01 n x 3 -> fp16 n x 4 (rgb logits, density logit) */
NGP_API int ngp_network_inference(ngp_ctx* ctx, uint32_t n, const float* pos01, const float* dir01, uint16_t* out_fp16);
/* K8/K9 update_density_grid_mean_and_bitfield (src/testbed_nerf.cu:2863-2880): the bitfield in use, 8 x 128^3 / 8 bytes */
NGP_API int ngp_get_density_bitfield(ngp_ctx* ctx, uint8_t* out, float* out_mean);
/* m_render_aabb / m_render_aabb_to_local (python_api.cu: testbed.render_aabb, .render_aabb_to_local): the crop box of the render,
 * min/max in ngp space; to_local9 column-major mat3 or NULL for identity */
NGP_API int ngp_set_render_aabb(ngp_ctx* ctx, const float* min3, const float* max3, const float* to_local9);
/* m_envmap (testbed.h:1297-1316; filled from the dataset's environment image or trained, src/testbed.cu:4194-4208): a lat-long RGBA
 * radiance map of width x height texels behind the NeRF. Every pixel with a valid ray starts from read_envmap(map, ray direction)
 * (envmap.cuh:24-50: bilinear, x periodic, y clamped; src/testbed_nerf.cu:1526-1528) and the NeRF is composited over it. NeRF mode.
 * rgba = NULL (or a zero size) removes the map. */
NGP_API int ngp_set_envmap(ngp_ctx* ctx, int32_t width, int32_t height, const float* rgba);
/* m_nerf.cone_angle_constant (python_api.cu: testbed.nerf.cone_angle_constant, run.py:167): 0 = fixed step size */
NGP_API int ngp_set_cone_angle_constant(ngp_ctx* ctx, float cone_angle_constant);
/* Testbed::update_density_grid_nerf (src/testbed_nerf.cu:2772-2861; kernels :185-232, :253-276): refresh the occupancy
 * grid from the density network -- n_uniform samples in random cells + n_nonuniform samples in cells above
 * NERF_MIN_OPTICAL_THICKNESS, density MLP, max-splat, decayed maximum into the grid -- n_iterations times, then the
 * mean / bitfield / max-pool of K8/K9. The generator (pcg32, seeded like reset_network does, testbed.cu:3848-3861) and
 * the EMA step counter live in the context. n_uniform = n_nonuniform = 0 selects training_prep_nerf's schedule
 * (:3432-3446): 128^3 x cascades uniform samples for the first 256 steps, then a quarter of that of each kind. */
NGP_API int ngp_update_density_grid(ngp_ctx* ctx, float decay, uint32_t n_uniform, uint32_t n_nonuniform, uint32_t n_iterations);
/* the float density grid in use: (max_cascade + 1) x 128^3 values, Morton order per cascade */
NGP_API int ngp_get_density_grid(ngp_ctx* ctx, float* out, uint64_t n);
/* K1+K2 init_rays_with_payload_kernel_nerf + advance_pos_nerf_kernel (src/testbed_nerf.cu:1428-1544,333-381):
 * out: W*H NerfPayload records of 40 bytes (nerf_device.cuh:144-152) */
NGP_API int ngp_init_rays(ngp_ctx* ctx, const ngp_camera* cam, void* payloads_out);


/* --- geometry mode: Testbed::load_scene / load_mesh (src/testbed_geometry_training.cu:3101-3210, 2786-2866)
 * load_scene: {"geometry":[{"center":[x,y,z],"path":..., "type":"Mesh"|"Nerf"}]}; Mesh -> load_mesh (.obj/.stl),
 * Nerf -> load_snapshot. Relative paths resolve against the json's directory. */
NGP_API int ngp_load_scene(ngp_ctx* ctx, const char* json_path);
/* load_mesh on triangles already in memory: vertices = n_tris*9 floats in file space; normalised into the unit cube
 * around `center`, BVH4 (8 triangles per leaf) built on the host, uploaded. Rebuilds the scene AABB. */
NGP_API int ngp_add_mesh(ngp_ctx* ctx, const float* vertices, uint32_t n_tris, const float* center3);
NGP_API int ngp_load_mesh_file(ngp_ctx* ctx, const char* path, const float* center3);
NGP_API int ngp_clear_meshes(ngp_ctx* ctx);
NGP_API int ngp_n_meshes(const ngp_ctx* ctx);
/* per mesh: triangle / node counts and the mesh AABB; mesh = -1: the scene AABB (root inflated by 4) */
NGP_API int ngp_get_mesh_info(const ngp_ctx* ctx, int mesh, uint32_t* n_tris, uint32_t* n_nodes, float* aabb6);
/* the built BVH: nodes (n_nodes x 32 B: bb.min, bb.max, left_idx, right_idx) and reordered triangles (n_tris x 36 B) */
NGP_API int ngp_get_mesh_bvh(const ngp_ctx* ctx, int mesh, void* nodes_out, void* triangles_out);
NGP_API int ngp_set_geometry_opts(ngp_ctx* ctx, const ngp_geometry_opts* opts);
/* M2 mesh_raytrace_kernel (src/geometry_bvh.cu:646-676): host positions / directions n x 3, updated in place.
 *   Of the loaded meshes only one is traced: the one whose box the ray's line enters at the smallest slab distance below 100.
 *   The distance's sign is not looked at: a box behind the origin counts, with its negative entry, and beats every box ahead of it (so a
 *   ray that starts on a mesh only sees that mesh). Within that mesh the closest triangle at a distance t in [0, 100) is the hit:
 *   position o + t d, direction replaced by the triangle's winding normal (b - a) x (c - a), normalised. Without a hit the ray comes back
 *   as o + 100 d with its direction unchanged. A ray whose line enters no box within 100 comes back untouched; the mesh
 *   pass of ngp_render shades such a pixel at the camera's position: alpha 1, depth 0, normal = the ray's direction. */
NGP_API int ngp_trace_mesh_rays(ngp_ctx* ctx, uint32_t n, float* positions, float* directions);


/* --- irradiance probes: Testbed::computeEnvmap / computeEnvmapMultiple (declared testbed.h:709-743, no body in the
 * reference; ray generators src/testbed_nerf.cu:1559-1773, tracer trace_mesh :2146-2262). Traces n_theta x n_phi
 * (x n_origin^2) rays through the NeRF and stores the lat-long RGBA texture (texel idx = i_theta + n_theta*j_phi,
 * mean over a texel's rays) in the context, plus E(n) tabulated at the texel directions. */
enum ngp_probe_mode { NGP_PROBE_CENTER = 0, NGP_PROBE_CENTER_OUTWARD = 1, NGP_PROBE_MULTI_CENTER = 2 };
typedef struct ngp_probe_desc {
	int32_t mode; /* ngp_probe_mode */
	uint32_t n_theta, n_phi, n_origin;
	float origin[3];         /* NGP_PROBE_CENTER_OUTWARD: shell position */
	float min_transmittance;
} ngp_probe_desc;
NGP_API int ngp_compute_envmap(ngp_ctx* ctx, const ngp_probe_desc* desc, float* rgba_out /* nullable: n_theta*n_phi*4 */);
/* the probe texture(s) and E(n) tabulated at the texel directions; after ngp_compute_envmap_grid: grid_x*grid_y textures back to back */
NGP_API int ngp_get_envmap(ngp_ctx* ctx, uint32_t* n_theta, uint32_t* n_phi, float* rgba_out, float* irradiance_rgba_out);
/* E(n) = sum_texels L(w) max(0, n.w) dOmega, dOmega = 4 pi/(n_theta n_phi), w = the direction the texel's ray travelled (for an
 * outward probe: -frame(normalize(origin)) * texel direction): host normals n x 3 -> host rgb n x 3. One probe only. */
NGP_API int ngp_irradiance(ngp_ctx* ctx, uint32_t n, const float* normals, float* rgb_out);

/* Testbed::computeEnvmapGrid (declared testbed.h:743, called src/main.cu:187-188 when m_render_mode == ShadeGridEnvMap -- the
 * fork's default, testbed.h:880 -- no body in the reference) with gridSize / m_envmap_tex (testbed.h:949-950). Definition used
 * here: grid_x x grid_y shell positions c + shell_radius * cylindrical_to_dir_nerf(
 * (i + .5) / grid_x, (j + .5) / grid_y) around c = render_aabb.center(); at each the K11 fan
 * (init_rays_from_center_outward_with_payload_kernel_nerf, src/testbed_nerf.cu:1611-1673) of n_theta x n_phi rays, all probes
 * traced in ONE launch; E_g(n) tabulated per probe. Mesh shading (NGP_RENDER_SHADE_GRID_ENVMAP) and ngp_irradiance_at blend
 * the four probes around the direction of (surface point - c), each read bilinearly at the normal in the manner of read_envmap
 * (envmap.cuh:24-50). */
typedef struct ngp_probe_grid_desc {
	uint32_t grid_x, grid_y; /* gridSize */
	uint32_t n_theta, n_phi; /* texels per probe */
	float shell_radius;
	float min_transmittance;
} ngp_probe_grid_desc;
NGP_API int ngp_compute_envmap_grid(ngp_ctx* ctx, const ngp_probe_grid_desc* desc, float* rgba_out /* nullable: grid_x*grid_y*n_theta*n_phi*4 */);
/* the grid as computed and its shell positions (nullable: grid_x*grid_y*3) */
NGP_API int ngp_get_envmap_grid(ngp_ctx* ctx, ngp_probe_grid_desc* desc_out, float* origins_out);
/* the lookup mesh shading does, at explicit surface points: positions / normals n x 3 -> rgb n x 3 (one probe: position unused) */
NGP_API int ngp_irradiance_at(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, float* rgb_out);

/* --- traced irradiance: E(p, n) = integral of L(p, w) max(0, n.w) dw estimated at the point itself by tracing the NeRF, L cut off where
 * an inserted mesh blocks the ray. The probes above read E from tables traced elsewhere; this is the quantity they approximate. No
 * counterpart in the reference: this project's own contract. All three entries run on the context's primary device and serve the models
 * the probes serve (grid models with base.json's heads, the Frequency architecture); anything else is refused with a message naming them.
 * A host-only context is refused ("no HIP device").
 *
 * ngp_trace_nerf_rays: the caller's rays through the NeRF with the probe tracer's semantics. Host arrays; positions in ngp space.
 *   Directions are normalised by the library and t is measured along the unit direction. A non-finite origin, or a zero or non-finite
 *   direction, or a NaN in t_range is refused with a message. t_range NULL: t_min = 0, t_max = +inf.
 *   Render box: the model's render box, or the inflated mesh-scene box while meshes are loaded (as for the probes).
 *   Start: t_start = max(t_min, entry), entry = 0 for an origin inside the box, else the box entry distance + 1e-6 (as for camera rays).
 *   A ray that misses the box (or has it behind its origin) or has t_start >= t_max is dead and returns zeros. As for probe rays there is
 *   no start jitter and no K2 advance, and the march gives up after 200 skip iterations without a sample.
 *   End: the march stops when the next sample position would be at t >= t_max, when it leaves the box, or at min_transmittance
 *   (<= 0 selects 0.01); a ray cut at t_max is shaded like one that left the box.
 *   Output: rgba_out n x 4, linear premultiplied RGBA, converted with the probe rule (an sRGB-trained network is linearised); no
 *   background. depth_out (nullable, n): the tracer's accumulated depth, for these rays the distance d.(pos - origin) of the sample of
 *   largest weight (what orc_trace_payloads returns with a camera at the origin looking along d); 0 where the ray was not shaded
 *   (alpha <= 0.001, which also leaves its rgba zero). ngp_get_render_stats reports the call like a probe launch.
 *   Large n is traced in chunks of a fixed size (2^21 rays); every ray is traced on its own, so results do not depend on it. */
NGP_API int ngp_trace_nerf_rays(ngp_ctx* ctx, uint32_t n, const float* origins /* n x 3 */, const float* directions /* n x 3 */,
                                const float* t_range /* nullable, n x 2: t_min, t_max */, float min_transmittance, float* rgba_out /* n x 4 */,
                                float* depth_out /* nullable, n */);
typedef struct ngp_irradiance_trace_desc {
	uint32_t n_u, n_v;        /* K = n_u * n_v directions per point, each at least 1; n * K <= 2^28 */
	float offset;             /* origin = p + offset * normalize(n), ngp units (e.g. 1e-4; finite and >= 0) */
	float min_transmittance;  /* as in ngp_trace_nerf_rays */
	int32_t occlude_by_meshes;
} ngp_irradiance_trace_desc;
/* ngp_irradiance_rays (a stage entry for tests): the hemisphere rays of n points, generated on the GPU. Point i's ray k has index
 *   i K + k, k = u + n_u v. With n^ = normalize(n_i) (a zero or non-finite normal, or a non-finite position, is refused):
 *   stratum centre a = (u + 0.5) / n_u, b = (v + 0.5) / n_v; local direction (Malley's method, cosine-weighted)
 *   (sqrt(a) cos 2 pi b, sqrt(a) sin 2 pi b, sqrt(1 - a)); world direction d = local_frame(n^) * local (compute_local_frame,
 *   random_val.cuh), normalised; origin p_i + offset n^. t_max: with occlude_by_meshes the distance to the closest triangle hit over ALL
 *   loaded meshes (the minimum of the per-mesh BVH4 closest hit, within its 100-unit range; unlike ngp_trace_mesh_rays, which follows the
 *   reference and only looks at the mesh whose box is entered first); +inf without meshes, without a hit or with occlusion off.
 *   Outputs origins_out / directions_out n K x 3, t_max_out n K. */
NGP_API int ngp_irradiance_rays(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, const ngp_irradiance_trace_desc* desc,
                                float* origins_out, float* directions_out, float* t_max_out);
/* ngp_irradiance_traced: the estimate. The generator's rays go through ngp_trace_nerf_rays' tracer (t_min = 0, t_max as generated) and a
 *   reduction writes per point out n x 4: rgb = (pi / K) sum_k rgb_k, the cosine-weighted estimator (a constant radiance L gives pi L),
 *   and w = the fraction of the point's K rays that no mesh blocks (1 without occlusion). A blocked ray still contributes the NeRF
 *   radiance in front of its hit; a mesh adds no radiance of its own here (interreflection: the SH9 volume's bounces, below). The sum runs in a fixed order (one wave per
 *   point, lane-strided, then a butterfly; no atomics), so the result is bit-identical from run to run and does not depend on how many
 *   points one call carries. Limits and refusals as for ngp_irradiance_rays; no model is refused too. */
NGP_API int ngp_irradiance_traced(ngp_ctx* ctx, uint32_t n, const float* positions, const float* normals, const ngp_irradiance_trace_desc* desc,
                                  float* out /* n x 4 */);

/* --- SH9 irradiance volumes: the incident radiance around a point, traced once over the whole sphere with the meshes occluding and kept
 * as nine spherical-harmonic coefficients per channel; E(n) for ANY normal is read back from them, and a lattice of such probes gives
 * E(p, n) inside a box for 8 probe reads where ngp_irradiance_traced traces K rays. This project's own contract (no counterpart in the
 * reference). Models, render box and device as for ngp_trace_nerf_rays: base.json's heads and the Frequency architecture, the inflated
 * mesh-scene box while meshes are loaded, the context's primary device only.
 *
 * Directions: K = n_u n_v world-space directions, the same for every probe, ray k = u + n_u v: a = (u + .5) / n_u, b = (v + .5) / n_v,
 *   z = 1 - 2 a, phi = 2 pi b, w_k = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z), normalised. The strata have equal area: a ray stands
 *   for 4 pi / K. Origin = the probe position itself (no offset, no normal); t_min = 0; t_max = the closest triangle hit over all loaded
 *   meshes with occlude_by_meshes (ngp_irradiance_rays' rule), +inf otherwise.
 * Basis: the nine real SH of degree <= 2 in the order, signs and constants of the network's SH direction encoding: Y_0 = 0.28209479;
 *   Y_1..3 = -0.48860251 y, 0.48860251 z, -0.48860251 x; Y_4..8 = 1.09254843 xy, -1.09254843 yz, 0.94617470 z^2 - 0.31539157,
 *   -1.09254843 xz, 0.54627422 (x^2 - y^2).
 * Probe record: 28 floats. c[3 m + ch] = (4 pi / K) sum_k L_ch(w_k) Y_m(w_k), m = 0..8, ch = r, g, b, with L the linear premultiplied rgb
 *   of ngp_trace_nerf_rays (a blocked ray contributes what lies in front of its hit; a mesh adds no radiance of its own: that is the bounces' part, below). Float 27 = w, the
 *   fraction of the K rays that no mesh blocks. The sum runs in a fixed order (one wave per probe, lane-strided, then a butterfly; no
 *   atomics): a record is bit-identical from run to run and for any split of the probes over calls or chunks.
 * Evaluation: E(n) = sum_m A_m c_m Y_m(n^), n^ = n / |n|, A = pi (m = 0), 2 pi / 3 (m = 1..3), pi / 4 (m = 4..8): the clamped-cosine
 *   convolution. There is NO clamp: nine coefficients cannot hold a sharp radiance, and E can ring slightly negative on the far side of a
 *   bright lobe.
 * Quadrature bias: the midpoint rule in z is not exact for band-limited radiance; its bias falls as 1 / n_u^2. Largest relative error of
 *   E for a random radiance of degree <= 2 (float64): 5.1 % at 8 x 8, 1.29 % at 16 x 16, 0.081 % at 64 x 64, 0.020 % at 128 x 128. A
 *   constant radiance L gives c_0 exactly and a small c_6 = -0.0155 L / 0.2821 at 16 x 16.
 * Limits: n_u, n_v >= 1; K <= 2^21 (a probe never spans a tracer chunk); probes * K <= 2^28 ("too large").
 * Refusals, each with a message: a host-only context ("no HIP device"), no model, an unsupported head, a non-finite position, a zero or
 *   non-finite normal, a bad descriptor. */
typedef struct ngp_irradiance_sh_desc {
	uint32_t n_u, n_v;        /* K = n_u * n_v directions per probe */
	float min_transmittance;  /* as in ngp_trace_nerf_rays */
	int32_t occlude_by_meshes;
} ngp_irradiance_sh_desc;
/* a stage entry for tests: the sphere rays of n probes. origins_out / directions_out n K x 3, t_max_out n K; needs no model */
NGP_API int ngp_irradiance_sphere_rays(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const ngp_irradiance_sh_desc* desc, float* origins_out,
                                       float* directions_out, float* t_max_out);
/* the records of n probes at the caller's positions. rays_rgba_out (the test stage): every ray's radiance as traced */
NGP_API int ngp_irradiance_sh_traced(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const ngp_irradiance_sh_desc* desc, float* sh_out /* n x 28 */,
                                     float* rays_rgba_out /* nullable, n K x 4 */);
/* E(n) of n records at n normals (normalised here): plain host code in double precision, no context or device. Returns 0, -1 for a zero
 * or non-finite normal (nothing is written from that record on), -2 for a null argument */
NGP_API int ngp_irradiance_sh_eval(uint32_t n, const float* sh /* n x 28 */, const float* normals /* n x 3 */, float* rgb_out /* n x 3 */);

/* The volume: res[0] x res[1] x res[2] probes over the box [aabb_min, aabb_max]; probe (i, j, k) sits at
 *   aabb_min + (i / (res[0] - 1), j / (res[1] - 1), k / (res[2] - 1)) (aabb_max - aabb_min), formed in double precision from the descriptor's
 *   floats and rounded to float; an axis of resolution 1 puts its probes at that axis's box centre (fraction 0.5) and takes no part in
 *   interpolation. Linear index g = i + res[0] (j + res[1] k). res >= 1 per axis; the box and its extent max - min finite (in float), min < max on every axis whose res > 1.
 * Lookup at (p, n), per axis: s = clamp((p - min) / (max - min), 0, 1) (r - 1), i0 = min(floor(s), r - 2) (0 when r = 1), f = s - i0;
 *   trilinear weights over the up to 8 corner probes. A probe with w = 0 is dead (every ray blocked: where a probe inside a closed mesh
 *   ends up) and is skipped; W = the sum of the live corners' weights; c~ = sum live weight c / W, or 0 when W = 0;
 *   out = (E_rgb(c~, n), W).
 * Lifetime: the volume is data. It lives on the primary device until it is replaced or cleared (get and the lookup read the primary; the
 *   auxiliary devices of a multi-device context hold replicas for NGP_RENDER_SHADE_IRRADIANCE_VOLUME frames alone); it is NEVER recomputed behind the
 *   caller's back when the model or the meshes change, and it is not stored in snapshots (ngp_get / ngp_set carry it to and from files).
 * Further refusals: a lookup or a get without a volume ("no irradiance volume"), non-finite values given to ngp_set_irradiance_volume. */
typedef struct ngp_irradiance_volume_desc {
	uint32_t res[3];
	float aabb_min[3], aabb_max[3];
	ngp_irradiance_sh_desc sh;
} ngp_irradiance_volume_desc;
NGP_API int ngp_compute_irradiance_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc); /* traced; kept on the primary device */
NGP_API int ngp_get_irradiance_volume(ngp_ctx* ctx, ngp_irradiance_volume_desc* desc_out, float* sh_out /* nullable, probes x 28 */);
/* a caller's own records, e.g. reloaded from a file; desc->sh is kept as given and not looked at */
NGP_API int ngp_set_irradiance_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const float* sh /* probes x 28 */);
NGP_API int ngp_clear_irradiance_volume(ngp_ctx* ctx);
NGP_API int ngp_irradiance_volume_at(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const float* normals /* n x 3 */, float* out /* n x 4 */);

/* --- probe visibility: the plain lookup blends a probe on the far side of an inserted mesh with full weight, so light and darkness leak
 * through walls. Each probe of the volume gets a small map of the mean and mean squared distance to the nearest mesh surface per
 * direction, and the lookup multiplies a probe's trilinear weight by the Chebyshev bound of the chance that the point is visible from
 * it (Majercik et al., "Dynamic Diffuse Global Illumination with Ray-Traced Irradiance Fields", JCGT 2019). This project's own contract.
 * Only BVH rays are traced: no model is needed and the NeRF's density occludes nothing.
 *
 * Distance map of a probe: 8 x 8 octahedral texels, texel q = i + 8 j, stored as 64 float2 (m1, m2) = 512 B a probe, probe-major in the
 *   volume's index order g, 16-B aligned.
 * Texel direction w_q: (a, b) = (2 (i + .5) / 8 - 1, 2 (j + .5) / 8 - 1), z = 1 - |a| - |b|, (x, y) = (a, b); if z < 0:
 *   (x, y) = ((1 - |b|) sgn a, (1 - |a|) sgn b) with sgn 0 = +1; (x, y, z) normalised.
 * Rays: the K = n_u n_v sphere directions w_k of the SH9 section, origin = the probe, t_min = 0. d_k = min(t_max_k, D), t_max_k the closest
 *   triangle hit over all loaded meshes (+inf without one: d_k = D). D = max_distance; a descriptor value <= 0 selects 1.5 x the diagonal
 *   of one lattice cell (an axis of resolution 1 counts with extent 0; every axis of resolution 1: 1.5 x the box diagonal), formed in
 *   double and rounded to float. ngp_get_irradiance_volume_visibility writes the D in use back.
 * Moments: x_qk = max(0, w_q . w_k); rho_qk = x_qk^(2^e), formed by e squarings in float32, e = sharpness_log2 in 0..6;
 *   S_q = sum_k rho_qk, m1_q = sum_k rho_qk d_k / S_q, m2_q = sum_k rho_qk d_k^2 / S_q; a texel with S_q = 0 (possible at very small K;
 *   every rho underflowing float32 counts) stores (D, D^2). The sums run over k ascending, one texel a lane, no atomics: a map is
 *   bit-identical from run to run and for any split of the probes over calls or chunks.
 * Visible lookup at (p, n): axis cells and trilinear weights wgt_c exactly those of ngp_irradiance_volume_at (from the clamped position);
 *   dead probes (w = 0) are skipped as there. For each remaining corner with wgt_c != 0: v = (p + normal_bias n^) - x_g with the UNCLAMPED p
 *   and x_g the probe position as the lattice formula gives it in float; r = |v|; r = 0: vis = 1. Otherwise the corner probe's map is read at
 *   v / r: the octahedral encode is the inverse of the decode above (divide by |x| + |y| + |z|, fold when z < 0), s = 4 (a + 1) - .5,
 *   t = 4 (b + 1) - .5, bilinear over the texels (floor s + {0, 1}, floor t + {0, 1}); an index outside 0..7 wraps across the octahedron's
 *   edge: i < 0 -> (-1 - i, 7 - j), i > 7 -> (15 - i, 7 - j), then the same rule for j with the roles swapped (no border texels).
 *   vis = 1 if r <= m1; else var = max(m2 - m1^2, 1e-4 D^2) and vis = (var / (var + (r - m1)^2))^3: continuous in r, m1 and m2.
 *   W' = sum wgt_c vis_c, c~ = sum wgt_c vis_c c / W', out = (E_rgb(c~, n), W'), zeros when W' = 0. With no meshes loaded and
 *   normal_bias = 0 every vis is exactly 1 for points inside the box, and the result is ngp_irradiance_volume_at's, bit for bit.
 * Out of scope: the backface (wrap-shading) weight and the weight crush of the DDGI paper; maps larger than 8 x 8; NeRF density as an
 *   occluder. Known limit: a point within about a texel's angular width of a wall, seen from the probe behind it, is only partly
 *   suppressed.
 * Lifetime: visibility is data like the volume. It lives on the primary device (auxiliary devices hold replicas for frames), is NEVER
 *   recomputed behind the caller's back and is not stored in snapshots. Computing, setting or clearing the VOLUME drops it: the lattice may
 *   have changed. While the context holds it, NGP_RENDER_SHADE_IRRADIANCE_VOLUME frames use the visible lookup (ambient light
 *   max(E, 0) / pi, 0 where W' = 0); no other mode looks at it.
 * Limits: n_u, n_v >= 1; K <= 2^21; probes * K <= 2^28.
 * Refusals, each with a message: a host-only context; no volume, for compute, set, get and the visible lookup ("no irradiance volume");
 *   no visibility, for get and the visible lookup ("no irradiance visibility: call ngp_compute_irradiance_volume_visibility or
 *   ngp_set_irradiance_volume_visibility first"); sharpness_log2 > 6; a non-finite max_distance; a non-finite or negative normal_bias;
 *   non-finite positions; a zero or non-finite normal; set with a non-finite value, m1 < 0 or m2 < 0. */
typedef struct ngp_irradiance_visibility_desc {
	uint32_t n_u, n_v;       /* K = n_u * n_v sphere directions per probe */
	uint32_t sharpness_log2; /* e: rho = max(0, cos)^(2^e), 0..6 */
	float max_distance;      /* D; <= 0 selects 1.5 x the lattice cell's diagonal (ngp_irradiance_distance_maps: must be > 0) */
	float normal_bias;       /* finite and >= 0, ngp units */
} ngp_irradiance_visibility_desc;
/* a stage entry for tests: the maps of n probes at the caller's positions. Needs a device, but no model and no volume; max_distance must
 * be > 0; normal_bias is not looked at */
NGP_API int ngp_irradiance_distance_maps(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const ngp_irradiance_visibility_desc* desc,
                                         float* maps_out /* n x 64 x 2 */);
/* the maps of the lattice of the volume the context holds; kept on the primary device */
NGP_API int ngp_compute_irradiance_volume_visibility(ngp_ctx* ctx, const ngp_irradiance_visibility_desc* desc);
NGP_API int ngp_get_irradiance_volume_visibility(ngp_ctx* ctx, ngp_irradiance_visibility_desc* desc_out, float* maps_out /* nullable, probes x 64 x 2 */);
/* a caller's own maps, e.g. reloaded from a file, for the probes of the held volume; desc->max_distance (> 0), sharpness_log2 and
 * normal_bias are kept, n_u and n_v are kept as given and not looked at */
NGP_API int ngp_set_irradiance_volume_visibility(ngp_ctx* ctx, const ngp_irradiance_visibility_desc* desc, const float* maps /* probes x 64 x 2 */);
NGP_API int ngp_clear_irradiance_volume_visibility(ngp_ctx* ctx);
NGP_API int ngp_irradiance_volume_at_visible(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const float* normals /* n x 3 */, float* out /* n x 4 */);

/* --- bounces: diffuse interreflection between the inserted meshes and the volume. A probe ray that a mesh blocks carries, in the records
 * above, the NeRF in front of the hit and nothing from the hit itself: meshes only darken. A bounce pass adds the light the hit surface
 * throws back, read from the volume of the pass before. This project's own contract.
 *
 * Let V_0 be the records ngp_compute_irradiance_volume produces. For bounce b = 1..N and every probe g:
 * Rays: the volume's own K = n_u n_v sphere directions w_k, origin o = the probe.
 * Closest hit: t_k = the closest triangle hit over all loaded meshes (the SH9 section's rule), m its mesh and i its triangle. Without a
 *   hit, or with occlude_by_meshes == 0, the ray carries no bounce.
 * Hit point and normal: h = o + t_k w_k in float32, the product rounded before the sum (no fused multiply-add);
 *   N = normalize(cross(b - a, c - a)) of the hit triangle, the normal ngp_trace_mesh_rays leaves; N_ff = N if N . w_k < 0, else -N.
 * Source: (E, W) = the lookup of V_{b-1} at (h, N_ff): ngp_irradiance_volume_at's, or, when the call is given a visibility descriptor,
 *   ngp_irradiance_volume_at_visible's with that lookup's own normal_bias and no other offset.
 * Radiance leaving the hit: M_ch = albedo_ch max(E_ch, 0) / pi; 0 where W = 0. The mesh is opaque and diffuse. albedo: the call's, or the
 *   hit mesh's own where it owns one ("mesh albedos", below).
 * Bounce radiance of the ray: B_k = (1 - alpha_k) M, alpha_k the alpha of the ray's NeRF trace (the rgba.w V_0 was projected from): the
 *   NeRF in front of the hit attenuates the bounce.
 * Records: R_b = the SH9 section's projection of B (the same order, the 4 pi / K scale, coefficients 0..26); V_b[j] = V_0[j] + R_b[j] in
 *   float32 for j < 27; float 27 (w, the unblocked fraction) stays V_0's, so the dead-probe rule is unchanged.
 * Order: every probe of V_b reads V_{b-1} alone: the records are double-buffered, never updated in place.
 * Determinism: no atomics; bit-identical from run to run and for any chunking. With N = 0, every albedo channel 0, no meshes loaded or
 *   occlude_by_meshes == 0 no pass runs and the records are V_0's as bytes.
 * Limits: N <= 16; every albedo channel finite and in [0, 1]; each refused with a message that names the field.
 * Out of scope: glossy transport in the volume (the frames' own mirror ray is ngp_set_mesh_reflection, below); a NeRF surface lit by the meshes; probes inside closed
 *   meshes (they stay dead: a room built of meshes alone gets nothing); bounces for the lat-long probe tables.
 * Refusals: those of the volume and visibility sections; ngp_irradiance_sh_bounce without a volume ("no irradiance volume") and with
 *   use_visible without visibility ("no irradiance visibility"); a non-finite alpha. */
typedef struct ngp_irradiance_bounce_desc {
	uint32_t n_bounces; /* N, at most 16 */
	float albedo[3];    /* of every mesh without its own (ngp_set_mesh_albedo), each channel in [0, 1] */
} ngp_irradiance_bounce_desc;
/* V_N, kept like ngp_compute_irradiance_volume's result: on the primary device, the held visibility dropped. With `visibility` non-NULL
 * the distance maps of the new lattice are computed BEFORE the bounces, used by them, and left in the context as
 * ngp_compute_irradiance_volume_visibility would leave them. The per-ray alpha of the whole volume (one float a ray, at most 2^28 rays =
 * 1 GB) lives for the duration of the call: the NeRF is traced ONCE however large N is. */
NGP_API int ngp_compute_irradiance_volume_bounced(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const ngp_irradiance_bounce_desc* bounce,
                                                  const ngp_irradiance_visibility_desc* visibility /* nullable */);
/* a stage entry for tests: ONE bounce pass at the caller's probes from the volume (and, with use_visible, the visibility) the context
 * HOLDS. Needs the meshes and a volume, no model. alpha: n K caller-given values (NULL: 0); desc->min_transmittance is not looked at.
 * rays_out (nullable) n K x 4 = (B_rgb, t of the hit or +inf); sh_out n x 28 = R, float 27 = the unblocked fraction */
NGP_API int ngp_irradiance_sh_bounce(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const ngp_irradiance_sh_desc* desc, const float albedo[3],
                                     const float* alpha /* nullable, n K */, int use_visible, float* sh_out /* n x 28 */, float* rays_out /* nullable, n K x 4 */);
/* device time (HIP events) of the last bounce pass of either entry, ms: its chunks' uploads, rays, projections and sums. Nothing in the
 * contract depends on it; tools/irradiance_bounce_rate.py reads it. */
NGP_API int ngp_get_irradiance_bounce_ms(ngp_ctx* ctx, float* ms);

/* --- sun: the sun's light on the inserted meshes as a bounce source. In an NGP_RENDER_SHADE frame the sun is the strongest light on a
 * mesh (suncol = 4 (255, 225, 195) / 255), and the records above hold none of it: a sunlit floor does not brighten what stands on it. The
 * sun pass adds the sun's FIRST bounce off the meshes to V_0, and the bounce passes carry it on. This project's own contract.
 *
 * V_0, the rays w_k, the closest hit (t_k, m, i), h = o + t_k w_k and N_ff are the bounce section's. s^ = direction / |direction|, the
 *   quotient formed in double precision from the descriptor's floats and rounded to float.
 * Per ray: c_k = N_ff . s^. The ray carries no sun light without a hit, with occlude_by_meshes == 0, or where c_k <= 0. Otherwise a shadow
 *   ray starts at q = h + shadow_bias N_ff (float32, every product rounded before its sum) and runs along s^; it is blocked when any
 *   triangle of ANY loaded mesh is hit at 0 <= t < 100 (the traversal's range, MAX_DIST); vis_k = 0 when blocked, else 1.
 *   B^sun_k,ch = (1 - alpha_k) ((albedo_ch radiance_ch) c_k / pi) vis_k in float32, alpha_k the alpha of the ray's NeRF trace, albedo
 *   ngp_irradiance_bounce_desc::albedo, or the hit mesh's own where it owns one ("mesh albedos", below). The term does not depend on the
 *   volume: a hit among dead probes is lit like any other.
 * Records: R_sun = the SH9 section's projection of B^sun (the same kernel, order and 4 pi / K scale); S[j] = V_0[j] + R_sun[j] in float32
 *   for j < 27; float 27 stays V_0's, so dead probes stay dead. S takes V_0's place in the bounce recurrence: V_b = S + R(V_{b-1}) with
 *   V_0 := S. With N = 0 the held volume is S, the sun's first bounce alone; with N passes sun light has bounced N + 1 times and NeRF
 *   light N times.
 * Determinism: no atomics; bit-identical from run to run and for any chunking. With sun == NULL, every radiance channel 0, every albedo
 *   channel 0, no meshes loaded or occlude_by_meshes == 0 no sun pass runs and the records are ngp_compute_irradiance_volume_bounced's as
 *   bytes.
 * Stated limits: the NeRF's density blocks the sun only through the *_shadowed entries below (the frames' own shadow ray does not test
 *   it); the sun as seen directly from a probe is not in the records (the BRDF's direct term has it); one directional light; the frames' shadow ray follows
 *   the reference's one-mesh rule (ngp_trace_mesh_rays), this one sees all meshes.
 * Refusals, each naming its field: a zero or non-finite direction; a negative or non-finite radiance; a negative or non-finite
 *   shadow_bias; a NULL bounce descriptor when the sun is given; albedo x radiance overflowing float; everything the volume, visibility
 *   and bounce sections refuse. */
typedef struct ngp_irradiance_sun_desc {
	float direction[3]; /* towards the sun; normalised here; finite and not zero */
	float radiance[3];  /* what a surface facing the sun receives (the frames' suncol); finite, >= 0 */
	float shadow_bias;  /* finite, >= 0; the frames use 1e-3 */
} ngp_irradiance_sun_desc;
/* ngp_compute_irradiance_volume_bounced with the sun pass between the trace (and the distance maps) and the bounce passes. The per-ray
 * alpha is kept whenever a sun pass or a bounce pass runs. The volume, the maps and one step of the generation counter are committed
 * together; a failed call leaves the held volume alone. */
NGP_API int ngp_compute_irradiance_volume_sunlit(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const ngp_irradiance_bounce_desc* bounce,
                                                 const ngp_irradiance_visibility_desc* visibility /* nullable */, const ngp_irradiance_sun_desc* sun /* nullable */);
/* a stage entry for tests: ONE sun pass at the caller's probes. Needs a device and the meshes, no model and no volume. alpha: n K
 * caller-given values (NULL: 0); desc->min_transmittance is not looked at. rays_out (nullable) n K x 4 = (B^sun_rgb, t of the primary hit
 * or +inf); sh_out n x 28 = R_sun, float 27 = the unblocked fraction */
NGP_API int ngp_irradiance_sh_sun(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const ngp_irradiance_sh_desc* desc, const ngp_irradiance_sun_desc* sun,
                                  const float albedo[3], const float* alpha /* nullable, n K */, float* sh_out /* n x 28 */, float* rays_out /* nullable, n K x 4 */);
/* device time (HIP events) of the last sun pass of either entry, ms, as ngp_get_irradiance_bounce_ms reports a bounce pass's */
NGP_API int ngp_get_irradiance_sun_ms(ngp_ctx* ctx, float* ms);

/* The NeRF's density in front of the sun. Without it a floor under the NeRF's object is lit as if the object were not there.
 *
 * The shadow ray: one exists for every probe ray k the sun pass above lights: a hit, c_k > 0, vis_k = 1. Its origin is q_k = h_k +
 *   shadow_bias N_ff, the very float32 value the mesh shadow query uses; its direction is s^ as formed above. It is traced through the
 *   NeRF with the semantics of ngp_trace_nerf_rays (the tracer's normalisation of the direction, the render box in force, which is the
 *   inflated mesh box while meshes are loaded), with t_range = (t_min, +inf) and min_transmittance from the descriptor below.
 * The result: alpha_s,k = that ray's alpha; T_s,k = max(1 - alpha_s,k, 0) in float32; B'_k,ch = fl(T_s,k B^sun_k,ch), one float32 product
 *   per channel on the sun pass's value. Rays without a shadow ray keep B' = B = 0 and report alpha_s = 0. The projection, S = V_0 + R_sun
 *   and the bounce recurrence are unchanged, with B' in B^sun's place; float 27 of a record is unchanged.
 * Determinism: no atomics; bit-identical from run to run and for any chunking (the shadow-ray list is not compacted: one entry per probe
 *   ray, dead where there is no shadow ray).
 * Stated limits: the NeRF attenuates the sun but is not lit by it; the frames' own direct sun term on a mesh pixel still ignores the NeRF,
 *   as in the reference, unless ngp_set_sun_nerf_shadow (the next block) is on, and no frame of another mode changes; a hit that sits inside the NeRF's own density shadows itself unless t_min
 *   skips it.
 * Refusals, each naming its field: a NaN min_transmittance; a negative or non-finite t_min; everything the sun section refuses. The bounce
 *   descriptor is looked at first, then the sun's, then this one, before anything else, on any context. */
typedef struct ngp_irradiance_sun_nerf_desc {
	float min_transmittance; /* as in ngp_trace_nerf_rays (<= 0 selects 0.01); NaN refused */
	float t_min;             /* the NeRF is ignored within t_min of q along the sun direction; finite, >= 0 */
} ngp_irradiance_sun_nerf_desc;
/* ngp_compute_irradiance_volume_sunlit with the shadow rays in its sun pass. nerf == NULL is that entry as bytes; sun == NULL (or any of
 * its no-source cases) runs no pass and the records are ngp_compute_irradiance_volume_bounced's as bytes. The volume, the maps and one step
 * of the generation counter are committed together, and peers get the volume, as there. ngp_get_render_stats reports the shadow trace
 * like any tracer call. */
NGP_API int ngp_compute_irradiance_volume_sunlit_shadowed(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const ngp_irradiance_bounce_desc* bounce,
                                                          const ngp_irradiance_visibility_desc* visibility /* nullable */, const ngp_irradiance_sun_desc* sun /* nullable */,
                                                          const ngp_irradiance_sun_nerf_desc* nerf /* nullable */);
/* a stage entry for tests: ONE shadowed sun pass at the caller's probes. Needs a device and a model (the meshes too, to light anything), no
 * volume. alpha as in ngp_irradiance_sh_sun. rays_out (nullable) n K x 4 = (B'_rgb, t of the primary hit or +inf); shadow_out (nullable)
 * n K x 4 = (q_xyz, alpha_s), zeros where there is no shadow ray; sh_out n x 28 = the projection of B', float 27 = the unblocked fraction */
NGP_API int ngp_irradiance_sh_sun_shadowed(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const ngp_irradiance_sh_desc* desc, const ngp_irradiance_sun_desc* sun,
                                           const float albedo[3], const float* alpha /* nullable, n K */, const ngp_irradiance_sun_nerf_desc* nerf,
                                           float* rays_out /* nullable, n K x 4 */, float* shadow_out /* nullable, n K x 4 */, float* sh_out /* n x 28 */);
/* device time (HIP events) of the shadow rays' prep and trace in the last sun pass, ms, summed over its chunks; 0 after a pass without them */
NGP_API int ngp_get_irradiance_sun_shadow_ms(ngp_ctx* ctx, float* ms);

/* mesh albedos: a mesh may own an albedo for the SH9 volume's passes, three floats, each finite and in [0, 1]. The bounce passes and the
 * sun pass use it where a probe ray's closest hit is on that mesh; a mesh without one uses the call's albedo, as every mesh does by default.
 * The frames' mesh pass never reads it (a frame's colours come from ngp_geometry_opts and the materials).
 *
 * Resolution at call time: for mesh m, a_m = its own albedo if it owns one, else the call's. The call's albedo is
 *   ngp_irradiance_bounce_desc::albedo for the volume entries (ngp_compute_irradiance_volume_bounced, _sunlit, _sunlit_shadowed) and the
 *   albedo[3] argument of the stage entries (ngp_irradiance_sh_bounce, ngp_irradiance_sh_sun, ngp_irradiance_sh_sun_shadowed).
 * Bounce: M_ch = a_m,ch max(E_ch, 0) / pi with m the mesh of the ray's closest hit; everything else of "bounces" is unchanged.
 * Sun: the source of mesh m is fl(a_m,ch radiance_ch), formed on the host in float like the descriptor's; B^sun uses the source of the hit's mesh.
 * Unchanged: geometry never depends on an albedo: t, N_ff, h, q, vis, the shadow-ray list, alpha_s and float 27 of a record.
 * No-source rules, over the resolved albedos: no bounce pass runs when every mesh's a_m is black on every channel; no sun pass runs when no
 *   mesh's source has a non-zero channel. A black call's albedo with one mesh owning a non-black one DOES run the passes. (The stage
 *   entries always run their one pass, as before.)
 * Lifetime: an albedo belongs to its mesh slot. ngp_clear_meshes and ngp_load_scene drop all of them; a mesh added by ngp_add_mesh or
 *   ngp_load_mesh_file has none; ngp_set_geometry_opts and ngp_set_mesh_material never touch one. ngp_load_scene gives a "Mesh" entry that
 *   carries "albedo": [r, g, b] that albedo. Both entries work on a host-only context.
 * Refusals: a mesh index out of range; a channel that is not finite or outside [0, 1] ("mesh albedo must be finite and in [0, 1] on every
 *   channel"); a per-mesh source that is not finite, like the descriptor's. A refusal leaves the state alone.
 * Identities as bytes: while no mesh owns an albedo every call launches the kernels it launched before albedos existed and returns those
 *   bytes; with every mesh owning the call's albedo the results are those bytes too.
 * Determinism: no atomics; bit-identical from run to run and for any chunking. The device table (16 bytes a mesh) is built and uploaded once
 *   per call, ahead of its passes, and freed behind the call's last synchronisation.
 * Several devices: the volume is computed on the primary alone, so no table travels; the peers get the records.
 * Stated limits: one albedo a mesh: no per-triangle albedo, no textures; the volume's bounce stays diffuse whatever the mesh's material. */
NGP_API int ngp_set_mesh_albedo(ngp_ctx* ctx, int mesh, const float albedo[3] /* nullable: back to the call's */);
/* out (nullable) receives the mesh's own albedo, zeros where it owns none; own (nullable) receives 1 or 0 */
NGP_API int ngp_get_mesh_albedo(ngp_ctx* ctx, int mesh, float out[3], int* own);

/* sun: the NeRF in front of the frames' sun. With the block above the ambient light under the captured object darkens; this option lets the
 * same density stand in front of the frames' own direct sun term on mesh pixels. Context state, set like the geometry options; off by
 * default, and with it off every frame is the one it was, as bytes.
 *
 * Which frames: Geometry mode, meshes loaded, a model loaded (such a frame always takes the general, non-direct path). All four mesh shade
 *   modes (Shade, ShadeEnvMap, ShadeGridEnvMap, ShadeIrradianceVolume with or without visibility).
 * Which pixels get a shadow ray: for each sample of the frame, a pixel whose primary ray hits a mesh inside the scene box AND whose mesh
 *   shadow ray (ngp_trace_mesh_rays' one-mesh rule, as in every frame) is unblocked. Pixels without a hit and pixels the meshes already
 *   shadow get none and report q = 0, alpha_s = 0.
 * The ray: origin q = pos + 1e-3 normalize(ff), the very float32 value the mesh shadow ray starts from before it is advanced to the scene
 *   box, ff the shading normal turned against the primary ray; direction s^ = normalize(normalize(sun_dir)) as the mesh pass forms it. It
 *   is traced with the semantics of ngp_trace_nerf_rays (the tracer normalises the direction; the render box in force, which is the
 *   inflated mesh box), t_range = (t_min, +inf), min_transmittance from the descriptor (<= 0 selects 0.01). alpha_s = that ray's alpha.
 * The colour: T_s = max(1 - alpha_s, 0) in float32; the mesh pass's shadow factor becomes fl(shadow T_s); nothing else changes, so T_s = 1
 *   gives the option-off bits. Depth, coverage, the ambient term, sharding, packing and the NeRF pass that follows are untouched.
 * Determinism: no atomics decide a value; frames are bit-identical from run to run. Everything runs on the frame's stream and
 *   ngp_render_device stays asynchronous.
 * Statistics: ngp_get_render_stats of the frame reports the frame's NeRF pass alone (n_rays, n_rays_hit, n_samples equal the option-off
 *   frame's); the shadow trace's own time is ngp_get_frame_sun_shadow_ms, inside ngp_get_mesh_pass_ms.
 * Identities as bytes (the frame is the option-off frame): the option off; NeRF mode; no meshes; no model (meshes only); a t_min beyond the
 *   box (>= its diagonal); a model whose density is empty along every shadow ray.
 * Refusals: ngp_set_sun_nerf_shadow refuses what ngp_irradiance_sun_nerf_desc's section refuses (a NaN min_transmittance; a negative or
 *   non-finite t_min), on any context. A model the ray-list tracer does not serve (an rgb head other than configs/nerf/base.json's) is
 *   refused when the frame is rendered, with the tracer's message, naming the option. A moving camera with meshes is refused as before.
 * Several devices: the option travels to the peers with the geometry and each device traces the shadow rays of its own tiles;
 *   ngp_get_frame_sun_shadow and ngp_get_frame_sun_shadow_ms read the primary's share only.
 * Stated limits: the NeRF attenuates the sun and is not lit by it; the meshes throw no shadow onto the NeRF unless ngp_set_mesh_shadow_on_nerf (the next block) is on;
 *   one directional light; a hit that sits inside the NeRF's own density shadows itself unless t_min skips it. */
/* nerf == NULL: off (the default). Refusals as ngp_irradiance_sun_nerf_desc's: NaN min_transmittance; negative or non-finite t_min. */
NGP_API int ngp_set_sun_nerf_shadow(ngp_ctx* ctx, const ngp_irradiance_sun_nerf_desc* nerf /* nullable */);
NGP_API int ngp_get_sun_nerf_shadow(ngp_ctx* ctx, ngp_irradiance_sun_nerf_desc* out, int* enabled);
/* stage entry for tests: per pixel of the LAST frame's LAST sample, in the frame's own pixel order (packed or not; on a multi-device context
 * the primary's tile-packed share): (q_xyz, alpha_s); zeros where the pixel had no shadow ray. n_pixels must be that frame's extent.
 * Refuses when the last frame ran no shadow trace. */
NGP_API int ngp_get_frame_sun_shadow(ngp_ctx* ctx, float* out /* n_pixels x 4 */, size_t n_pixels);
/* device time (HIP events) of the shadow rays' prep and trace in the last frame's last sample; 0 after a frame without them */
NGP_API int ngp_get_frame_sun_shadow_ms(ngp_ctx* ctx, float* ms);

/* sun: the meshes in front of the sun on the NeRF. The block above lets the captured object shadow the inserted meshes; this option lets the
 * inserted meshes throw the sun's shadow onto the captured scene. Context state, set like ngp_set_sun_nerf_shadow; off by default, and with
 * it off every frame is the one it was, as bytes.
 *
 * Which frames: Geometry mode, meshes loaded, a model loaded, render modes Shade, ShadeEnvMap, ShadeGridEnvMap and ShadeIrradianceVolume
 *   (with or without visibility). In every other frame (NeRF mode, no meshes, no model) the option is ignored and the frame is the
 *   option-off frame, as bytes; the G-buffer modes AO / Positions / Depth / Cost / Normals apply to NeRF mode alone.
 * Each sample of such a frame runs three steps on the frame's stream:
 *   1. the mesh pass, exactly as with the option off (the fused pass, or the split pass of ngp_set_sun_nerf_shadow when that is on too);
 *   2. the NeRF launch, unchanged, with its colour output pointed at a zeroed per-pixel scratch instead of the frame: the scratch then holds
 *      the NeRF's premultiplied n = (r, g, b, a) of a pixel the NeRF wrote and zero bits of any other (a <= 0.001, or culled by the depth
 *      test against the meshes). The depth buffer, the depth test and the depth writes are those of every frame;
 *   3. nerf_mesh_shadow_kernel, one thread a pixel:
 *      n.w == 0: nothing is written, the pixel stays the mesh pass's; the record is (0, 0, 0, 0).
 *      n.w > 0.2 (the NeRF pass's own rule for writing depth, so the depth buffer holds this ray's depth, the z-depth of its sample of
 *        largest weight): the pixel owns a surface point p = o + d ((depth - cam_fwd . (o - cam_pos)) / (cam_fwd . d)), (o, d) the ray the
 *        NeRF pass forms for that pixel and sample (lens, aperture, near distance and sample offset included). s^ =
 *        normalize(normalize(sun_dir)) as the mesh pass forms it, q = p + bias s^, blocked = a triangle of ANY mesh lies within 100 of q
 *        along s^ (the sunlit volume's shadow query). f = blocked ? fl(1 - strength) : 1. The record is (p, blocked ? 2 : 1).
 *      0 < n.w <= 0.2: f = 1, the record is (0, 0, 0, 0).
 *      The pixel becomes (fl(r f) + m.x k, fl(g f) + m.y k, fl(b f) + m.z k, a + m.w k), m the mesh pass's value of the pixel and
 *      k = 1 - a: the NeRF pass's own composite, in its order, so f = 1 gives the option-off bits.
 *   Accumulation and tonemapping follow as in every frame.
 * strength: the share of the NeRF's own colour that the sun is taken to carry. A photograph does not say what that share is, so it is the
 *   caller's number (the bindings' True: 0.5). bias: how far q is lifted off p towards the sun (True: 1e-2).
 * Determinism: no atomics decide a value; frames are bit-identical from run to run. ngp_render_device stays asynchronous.
 * Statistics: ngp_get_render_stats is the option-off frame's; the new kernel's time is ngp_get_frame_mesh_shadow_ms.
 * Identities as bytes (colour and depth are the option-off frame's): the option off; strength 0; NeRF mode; no meshes; no model; a model
 *   without density. Depth is the option-off frame's in every case.
 * Refusals: a strength that is NaN or outside [0, 1]; a bias that is not finite or is negative; on any context. A refused call leaves the
 *   option alone.
 * Several devices: the option travels to the peers with the geometry and each device shadows its own share; ngp_get_frame_mesh_shadow and
 *   ngp_get_frame_mesh_shadow_ms read the primary's share only.
 * Stated limits: the shadow is hard-edged unless ngp_set_sun_disk (below) is on, and there is one directional light; the NeRF pixel is scaled as a whole at its largest-weight
 *   sample, there is no per-sample shadowing along the ray; a pixel of alpha <= 0.2 is never shadowed; shadows already baked into the
 *   photographs are not removed; the ambient light on the NeRF changes only with ngp_set_ambient_change_on_nerf (the next block). */
typedef struct ngp_mesh_shadow_on_nerf_desc { float strength; float bias; } ngp_mesh_shadow_on_nerf_desc;
/* desc == NULL: off (the default) */
NGP_API int ngp_set_mesh_shadow_on_nerf(ngp_ctx* ctx, const ngp_mesh_shadow_on_nerf_desc* desc /* nullable: off */);
NGP_API int ngp_get_mesh_shadow_on_nerf(ngp_ctx* ctx, ngp_mesh_shadow_on_nerf_desc* out, int* enabled);
/* stage entry for tests: per pixel of the LAST frame's LAST sample, in the frame's own pixel order (packed or not; on a multi-device context
 * the primary's tile-packed share): (p_xyz, 2 blocked / 1 open); zeros where the pixel owns no surface point. n_pixels must be that frame's
 * extent. Refuses when the last frame did not run the pass. */
NGP_API int ngp_get_frame_mesh_shadow(ngp_ctx* ctx, float* out /* n_pixels x 4 */, size_t n_pixels);
/* device time (HIP events) of nerf_mesh_shadow_kernel in the last frame's last sample; 0 after a frame without it */
NGP_API int ngp_get_frame_mesh_shadow_ms(ngp_ctx* ctx, float* ms);

/* sun: the sun's disk. Every sun shadow above is one boolean a pixel, and on a mesh pixel the mesh pass's shadow ray sees one mesh only
 * (M3's rule). This option gives the directional light an angular radius: K shadow rays a pixel are spread over the disk and tested against
 * ALL meshes (the sunlit volume's query: a triangle of any mesh within 100 along the ray), and the open fraction takes the boolean's place
 * wherever a mesh can stand in front of the sun. Context state, set like ngp_set_sun_nerf_shadow; off by default, and with it off every
 * frame is the one it was, as bytes.
 *
 * The table of a sample, formed in double and rounded to float once; K = n_rays, s = the spp index of the sample (ngp_camera::spp_index +
 *   the sample's number in the call, what the sample's pixel offset is drawn with):
 *     s^ = sun_dir / |sun_dir|; a = the coordinate axis where |s^_j| is smallest, the lowest index on ties;
 *     u = (a x s^) / |a x s^|, v = s^ x u;
 *     r_k = sqrt((k + 0.5) / K) for K > 1, r_0 = 0 for K = 1;
 *     phi_k = k pi (3 - sqrt 5) + 2 pi frac(s 0.6180339887498949);
 *     d_k = unit(s^ + tan(angular_radius) r_k (cos phi_k u + sin phi_k v)).
 *   Every pixel of a sample uses the same table, successive samples use rotated ones. The kernels receive the K float directions by value
 *   in their arguments (no copy in the stream, no synchronisation) and use them as they are, without renormalising.
 *   ngp_sun_disk_directions returns that table; it is host arithmetic and works on a host-only context.
 * Mesh pixels, in every Geometry frame with meshes, with or without a model: the frame takes the split mesh pass (G-buffer -> lists ->
 *   deferred shade; meshes alone fill the shadow list without tracing it) and mesh_sun_disk_kernel runs behind mesh_gbuffer_kernel, before
 *   the shadow list's prep step. A pixel owns a disk where it is covered and its primary ray found a triangle. q = pos + 1e-3 normalize(ff),
 *   the shadow list's origin as bits; count = the number of k with a triangle of any mesh within 100 of q along d_k;
 *   V = (K - count) / K, exact in float, takes the place of M4's shadow in the G-buffer, so the deferred shade's sun colour is scaled by
 *   fl(V T_s). The pixel's shadow-list entry is rewritten: live (origin q, t = (t_min, +inf), the central direction it had) where V > 0,
 *   dead otherwise, so with ngp_set_sun_nerf_shadow on the NeRF's shadow ray is still one ray along the sun's centre, from every pixel a
 *   part of the disk reaches. A covered pixel without a triangle keeps M4's value.
 * NeRF pixels, where ngp_set_mesh_shadow_on_nerf is on too: owner, p and q = p + bias s^ are that block's; count as above from q;
 *   f = fl(1 - fl(strength fl(count / K))); the composite is that block's. Its record's w becomes 1 + count / K: 1 is open and 2 is blocked
 *   as before. count = K gives the hard pass's f as bits. Without the disk the pass runs the kernel it ran before.
 * Identities as bytes: the option off; no meshes; NeRF mode. With the disk on, strength 0 gives the NeRF pixels of
 *   ngp_set_mesh_shadow_on_nerf off. Frames and records are bit-identical from run to run: no atomics, and a pixel's count does not depend
 *   on which other pixels its wave holds.
 * Refusals, on any context, leaving the option alone: an angular_radius that is not finite, negative or above 0.5 rad; n_rays outside
 *   {1, 2, 4, 8, 16}. ngp_sun_disk_directions also refuses a sun_dir that is not finite or has no length, and needs the option on.
 * Several devices: the option travels to the peers with the geometry; ngp_get_frame_sun_disk and ngp_get_frame_sun_disk_ms read the
 *   primary's share only.
 * Stated limits: the SH9 volume's sun pass stays hard-edged; the mirrored hit's shadow2 (ngp_set_mesh_reflection_meshes) stays hard-edged;
 *   the NeRF's own shadow ray stays one central ray; the pattern is the same for every pixel of a sample, so at 1 spp a wide penumbra
 *   shows K + 1 levels as bands; there is still one light. */
typedef struct ngp_sun_disk_desc { float angular_radius; /* rad, in [0, 0.5]; the real sun: 0.00465 */ uint32_t n_rays; /* 1, 2, 4, 8 or 16 */ } ngp_sun_disk_desc;
/* desc == NULL: off (the default) */
NGP_API int ngp_set_sun_disk(ngp_ctx* ctx, const ngp_sun_disk_desc* desc /* nullable: off */);
NGP_API int ngp_get_sun_disk(ngp_ctx* ctx, ngp_sun_disk_desc* out, int* enabled);
/* the table the frame's sample of spp index `spp_index` uses under the sun direction sun_dir: 3 n_rays floats */
NGP_API int ngp_sun_disk_directions(ngp_ctx* ctx, const float* sun_dir /* 3 */, uint32_t spp_index, float* out /* 3 n_rays */);
/* stage entry for tests: per pixel of the LAST frame's LAST sample, in the frame's own pixel order (packed or not; on a multi-device context
 * the primary's tile-packed share): (q_xyz, 1 + count); zeros where the pixel owns no disk. n_pixels must be that frame's extent. Refuses
 * when the last frame did not run the pass. */
NGP_API int ngp_get_frame_sun_disk(ngp_ctx* ctx, float* out /* n_pixels x 4 */, size_t n_pixels);
/* device time (HIP events) of mesh_sun_disk_kernel in the last frame's last sample; refuses when the last frame did not run the pass */
NGP_API int ngp_get_frame_sun_disk_ms(ngp_ctx* ctx, float* ms);

/* ambient: what the inserted meshes change in the ambient light on the NeRF (differential rendering). The context holds a second SH9
 * volume, the REFERENCE volume: the scene before anything was inserted. With the option on, a NeRF pixel that owns a surface point has its
 * colour scaled, per channel, by g = E_after(p, N) / E_before(p, N): "after" the context's own volume (ngp_compute_irradiance_volume* /
 * ngp_set_irradiance_volume), "before" the reference, N the NeRF's own normal at p. Off by default, and with it off every frame is the
 * one it was, as bytes.
 *
 * The reference volume is data, held exactly like the context's volume: on the primary device, never recomputed behind the caller's back,
 *   not stored in snapshots, copied to the peers with the geometry (a generation counter of its own). It has no visibility maps.
 *   ngp_compute_reference_irradiance_volume: V_0 of the SH9 block above, traced over the lattice of desc with occlude_by_meshes forced to
 *   0 whatever desc->sh says; no bounces, no sun. The context's own volume is untouched. ngp_set_ / ngp_get_ / ngp_clear_reference_
 *   irradiance_volume: as ngp_set_ / ngp_get_ / ngp_clear_irradiance_volume, with their refusals and messages.
 * The ratio at (p, N^), N^ = N / |N|. Both lookups are the plain ngp_irradiance_volume_at lookup: (E_after, W_after) in the context's
 *   volume, (E_before, W_before) in the reference. The visibility maps are not used. Per channel
 *     a = max(E_after, 0), b = E_before, g = (b > min_irradiance) ? min(a / b, max_gain) : 1
 *   state 1, "no estimate", when W_after = 0 or W_before = 0: g = (1, 1, 1); state 2 otherwise.
 *   IDENTITY: identical records in the two volumes (the same lattice and box) give a / b = 1 exactly on every channel, whatever N is: one
 *   device function evaluates both lookups, a and b are then the same bits, and a correctly rounded quotient of equal numbers is 1. So the
 *   two volumes should be computed with the same lattice, box and ray counts, and away from the meshes, where their records agree, the
 *   option changes nothing.
 * min_irradiance: below it the reference is taken to say nothing about the channel (the bindings' True: 1e-3). max_gain: the cap on g
 *   (True: 4). Refused: values that are not finite, min_irradiance < 0, max_gain < 1; on any context; a refused call leaves the option alone.
 * Which frames: those of ngp_set_mesh_shadow_on_nerf (Geometry mode, meshes, a model, the four shade modes); every other frame ignores the
 *   option and is the option-off frame as bytes. Such a frame is refused when either volume is missing (the message names it), and for
 *   Frequency / Identity (wide) models: the normals kernel runs the grid encoding's gradient.
 * Each sample, on the frame's stream, nothing waits: (1) the mesh pass; (2) the NeRF launch into the zeroed scratch n of the block above;
 *   (3) nerf_surface_normals_kernel: a pixel with n.w > 0.2 owns p exactly as in the block above; N = -(grad / aabb_diag) / |grad /
 *   aabb_diag|, grad the density-gradient stage (ngp_density_gradient) at the warped p: the marching-cubes export's rule. A zero or
 *   non-finite length gives state 1. N is the raw gradient: neither smoothed nor flipped towards the viewer; (4) nerf_ambient_ratio_
 *   kernel, one thread a pixel: g as above, n.rgb <- fl(n.rgb g) in the scratch; (5) the closing composite: nerf_mesh_shadow_kernel when
 *   ngp_set_mesh_shadow_on_nerf is on too (the pixel is fl(fl(n g) f) + m k), else the same expression with f = 1 and no shadow query. g = 1
 *   and f = 1 give the option-off bits. Depth, alpha and ngp_get_render_stats are the option-off frame's.
 * The record: 12 floats a pixel: p (3), state (0 not an owner, 1 no estimate, 2 scaled), N (3), W_after, g (3), W_before.
 * Stated limits: the pixel is scaled as a whole at its largest-weight sample, pixels of alpha <= 0.2 are untouched; the normal is the raw
 *   density gradient; the lookup is plain, so light leaks through thin inserted walls as it does for the meshes without visibility; SH9
 *   holds no sharp contact shadow; grid-encoded models only; shadows and interreflections already in the photographs stay. */
typedef struct ngp_ambient_change_desc { float min_irradiance; float max_gain; } ngp_ambient_change_desc;
NGP_API int ngp_compute_reference_irradiance_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc);
NGP_API int ngp_set_reference_irradiance_volume(ngp_ctx* ctx, const ngp_irradiance_volume_desc* desc, const float* sh /* probes x 28 */);
NGP_API int ngp_get_reference_irradiance_volume(ngp_ctx* ctx, ngp_irradiance_volume_desc* desc_out, float* sh_out /* nullable, probes x 28 */);
NGP_API int ngp_clear_reference_irradiance_volume(ngp_ctx* ctx);
/* desc == NULL: off (the default) */
NGP_API int ngp_set_ambient_change_on_nerf(ngp_ctx* ctx, const ngp_ambient_change_desc* desc /* nullable: off */);
NGP_API int ngp_get_ambient_change_on_nerf(ngp_ctx* ctx, ngp_ambient_change_desc* out, int* enabled);
/* stage entry for tests and tools: (g rgb, state) at explicit points and normals. Refuses without either volume, a zero or non-finite
 * normal, a non-finite position. */
NGP_API int ngp_irradiance_volume_ratio(ngp_ctx* ctx, uint32_t n, const float* positions /* n x 3 */, const float* normals /* n x 3 */,
                                        const ngp_ambient_change_desc* desc, float* out /* n x 4 */);
/* per pixel of the LAST frame's LAST sample, in the frame's own pixel order (packed or not; on a multi-device context the primary's
 * tile-packed share): the 12-float record. n_pixels must be that frame's extent. Refuses when the last frame did not run the pass. */
NGP_API int ngp_get_frame_ambient_change(ngp_ctx* ctx, float* out /* n_pixels x 12 */, size_t n_pixels);
/* device time (HIP events) around the two new kernels in the last frame's last sample; 0 after a frame without them */
NGP_API int ngp_get_frame_ambient_change_ms(ngp_ctx* ctx, float* ms);

/* mesh reflection: the inserted meshes mirror the NeRF, one reflection ray a pixel. The mesh BRDF's GGX lobe, Fresnel term, metallic and
 * specular answer to the sun alone; with this option a mesh pixel also receives what the captured scene sends along its mirror direction.
 * Context state, set like ngp_set_sun_nerf_shadow; off by default, and with it off every frame is the one it was, as bytes.
 *
 * Which frames: Geometry mode, meshes loaded, a model loaded, render modes Shade, ShadeEnvMap, ShadeGridEnvMap and ShadeIrradianceVolume
 *   (with or without visibility). Every other frame ignores the option and is the option-off frame as bytes. Such a frame takes the split
 *   mesh pass of ngp_set_sun_nerf_shadow (G-buffer, ray-list trace, deferred shade) with a second ray list, on the frame's stream.
 * Which pixels own a reflection ray: for each sample of the frame, a pixel that is covered (its hit position lies inside the scene box) AND
 *   whose primary ray found a triangle. The second condition is this block's own: a pixel whose ray chose no mesh is covered too, with
 *   normal = dir, and its mirror ray would run straight back at the camera; it owns no ray.
 * The ray, from the float32 values the pass holds: n^ = normalize(ff), ff the winding normal turned against the primary ray as the mesh pass
 *   forms it; c = -(n^ . primary_dir); origin q = pos + 1e-3 n^, the very value the sun block calls q; direction r = primary_dir + (2 c) n^;
 *   t_range = (t_min, t_hit), t_hit the closest triangle over ALL meshes from q along normalize(r), +inf without one: the rule of
 *   ngp_irradiance_rays with occlude_by_meshes, not the one-mesh rule of the frames' shadow ray. It is traced with the semantics of
 *   ngp_trace_nerf_rays: the tracer normalises the direction; the render box in force is the inflated mesh box; no background; a ray cut at
 *   t_hit is shaded like one that left the box. The result (rgb_r, alpha_r) is linear and premultiplied.
 * The colour, behind the mesh pass's BRDF and only where alpha_r > 0, in float32 and in this order:
 *     Cspec0 = mix3(specular * 0.08 * (1, 1, 1), base^2, metallic)      (the BRDF's own Cspec0 with its tint at 0)
 *     F = mix3(Cspec0, (1, 1, 1), SchlickFresnel(c))
 *     color += fl(fl(F (.) rgb_r) strength)
 *   A pixel with alpha_r = 0, or without a ray, keeps the bits it would have had; so do depth, coverage, the ambient term, sharding and
 *   packing, and the NeRF pass that follows. With ngp_set_sun_nerf_shadow off the shadow trace is not run and T_s = 1; with it on, each
 *   list is traced on its own and each record is that of the frame with only that option on, as bytes.
 * Determinism: no atomics decide a value; frames are bit-identical from run to run. Everything runs on the frame's stream and
 *   ngp_render_device stays asynchronous.
 * Statistics: ngp_get_render_stats reports the frame's NeRF pass alone; the tracer's counters go to a block of the context's own. The time of
 *   prep + trace is ngp_get_frame_mesh_reflection_ms, inside ngp_get_mesh_pass_ms.
 * Identities as bytes (the frame is the option-off frame): the option off; strength 0 (no trace is run); NeRF mode; no meshes; no model
 *   (meshes only); a t_min of at least the box diagonal; a model that is empty along every reflection ray.
 * Refusals: a NaN min_transmittance, a negative or non-finite t_min, a negative or non-finite strength, on any context; a refused call leaves
 *   the option as it was. A model the ray-list tracer does not serve is refused when the frame is rendered, naming the option. The stage
 *   entries refuse a host-only context ("no HIP device"). A moving camera with meshes is refused as before.
 * Several devices: the option travels to the peers with the geometry and each device traces the rays of its own tiles;
 *   ngp_get_frame_mesh_reflection and ngp_get_frame_mesh_reflection_ms read the primary's share only.
 * Stated limits: mirror direction only: roughness does not blur the reflection, and strength is the caller's handle on that. Without
 *   ngp_set_mesh_reflection_meshes (below) meshes do not appear in reflections: a ray cut by a mesh carries what the NeRF put in front of
 *   the hit, and black behind it. No environment map or
 *   sky fills the reflection where alpha_r < 1. The reflected NeRF is the captured one: the shadow and the ambient change of
 *   ngp_set_mesh_shadow_on_nerf / ngp_set_ambient_change_on_nerf are not applied to it. A surface inside the NeRF's own density reflects
 *   that density unless t_min skips it. The NeRF does not reflect the meshes. */
typedef struct ngp_mesh_reflection_desc {
	float strength;          /* the factor on the reflected radiance; finite, >= 0 (the bindings' True: 1). 0: the frame is the option-off frame */
	float min_transmittance; /* as in ngp_trace_nerf_rays (<= 0 selects 0.01); NaN refused (True: 0.01) */
	float t_min;             /* the NeRF is ignored within t_min of q along the mirror direction; finite, >= 0 (True: 0) */
} ngp_mesh_reflection_desc;
/* desc == NULL: off (the default) */
NGP_API int ngp_set_mesh_reflection(ngp_ctx* ctx, const ngp_mesh_reflection_desc* desc /* nullable: off */);
NGP_API int ngp_get_mesh_reflection(ngp_ctx* ctx, ngp_mesh_reflection_desc* out, int* enabled);
/* stage entry for tests and tools: per pixel of the LAST frame's LAST sample, in the frame's own pixel order (packed or not; on a
 * multi-device context the primary's tile-packed share), 12 floats: q (3), t_hit, r (3) as handed to the tracer before it is normalised,
 * 0, rgb_r (3), alpha_r; zeros where the pixel owns no ray. n_pixels must be that frame's extent. Refuses when the last frame traced no
 * reflection rays. */
NGP_API int ngp_get_frame_mesh_reflection(ngp_ctx* ctx, float* out /* n_pixels x 12 */, size_t n_pixels);
/* device time (HIP events) of the reflection rays' prep and trace in the last frame's last sample; 0 after a frame without them */
NGP_API int ngp_get_frame_mesh_reflection_ms(ngp_ctx* ctx, float* ms);

/* mesh reflection, the meshes in it: a mirror ray that a mesh cuts has its hit shaded by the mesh pass's own M5, composited behind the NeRF
 * along the ray. A sub-option of the mesh reflection: context state, off by default. It acts while ngp_set_mesh_reflection is on with
 * strength > 0 in a frame the reflection serves; every other frame ignores it. All values are float32, in this order, under
 * -ffp-contract=off.
 *
 * Who owns a hit: a pixel that owns a mirror ray (the rule above) whose t_hit is finite.
 * The hit: r^ = normalize3(r) as the reflection forms it for closest_hit; (mesh, tri) what closest_hit reports for that call;
 *   p2 = q + r^ t_hit; n2 = normalize3(cross(b - a, c - a)) of that triangle, the raw winding normal as the mesh trace leaves it, so the
 *   shade gets what the frames' own trace would have given it.
 * Its sun: ff2 = n2 turned against r^ (n2 where n2 . r^ < 0, else -n2); q2 = p2 + 1e-3 normalize3(ff2); shadow2 = 0 where a triangle of ANY
 *   mesh lies within MAX_DIST of q2 along the frames' shadow direction, else 1. This is the all-meshes rule of ngp_set_mesh_shadow_on_nerf,
 *   not the one-mesh rule of the frames' own shadow ray. ngp_set_sun_nerf_shadow does not reach the hit: the NeRF throws no shadow on a
 *   mirrored mesh.
 * Its colour: C2 = the mesh pass's shade at (p2, n2) viewed along r^ with shadow2: the frame's own ambient source (sky term, probe table(s),
 *   SH9 volume, visible volume) and the one material of the context. C2 carries no mirror ray of its own: one bounce only.
 * The pixel: L = rgb_r + fl(max(1 - alpha_r, 0) C2); color += fl(fl(F (.) L) strength), F the term above; added where alpha_r > 0 or the ray
 *   owns a hit. A ray without a hit (t_hit = +inf) keeps exactly the bits it has with the sub-option off; a hit with alpha_r = 0 gives L = C2.
 * Identities as bytes (the frame is that of the same options without the sub-option): the sub-option off; on with the reflection off, at
 *   strength 0, in NeRF mode, without meshes, or without a model; on in a scene where no mirror ray is cut.
 * Records: the 12-float record of ngp_get_frame_mesh_reflection does not change by a bit (it is the tracer's rgb_r and alpha_r); neither do
 *   depth, coverage, the NeRF pass, the sun-shadow record and ngp_get_render_stats.
 * Determinism: no atomics; frames are bit-identical from run to run. One kernel on the frame's stream between the reflection list's fill
 *   and its prep step, inside the time of ngp_get_frame_mesh_reflection_ms; nothing waits on the host.
 * Several devices: the flag travels to the peers with the geometry; ngp_get_frame_mesh_reflection_hits reads the primary's share only.
 * Stated limits: one bounce; mirror direction only; no sky where alpha_r < 1 and nothing is hit; no NeRF shadow on the mirrored hit; the hit is
 *   not ambient-changed by ngp_set_ambient_change_on_nerf; the NeRF still does not reflect the meshes. */
NGP_API int ngp_set_mesh_reflection_meshes(ngp_ctx* ctx, int on);
NGP_API int ngp_get_mesh_reflection_meshes(ngp_ctx* ctx, int* on);
/* stage entry for tests and tools: per pixel of the LAST frame's LAST sample, in the frame's own pixel order (as ngp_get_frame_mesh_reflection),
 * 8 floats: p2 (3), shadow2, C2 (3), 1; zeros where the pixel owns no hit. n_pixels must be that frame's extent. Refuses when the last frame
 * shaded no reflection hits. */
NGP_API int ngp_get_frame_mesh_reflection_hits(ngp_ctx* ctx, float* out /* n_pixels x 8 */, size_t n_pixels);
/* device time (HIP events) of the hit-shade kernel in the last frame's last sample; 0 after a frame without it */
NGP_API int ngp_get_frame_mesh_reflection_hits_ms(ngp_ctx* ctx, float* ms);

/* The six frame options together (ngp_set_sun_nerf_shadow, ngp_set_sun_disk, ngp_set_mesh_reflection, ngp_set_mesh_reflection_meshes,
 * ngp_set_mesh_shadow_on_nerf, ngp_set_ambient_change_on_nerf). Any set of them may be on; each keeps its own block's rule and these hold
 * between them, as bytes (tests/test_frame_options_gpu.py renders all 48 sets):
 *   Depth is the frame's with every option off.
 *   What a record depends on: ngp_get_frame_mesh_reflection on the reflection alone; ngp_get_frame_mesh_reflection_hits on the reflection and
 *     its sub-option; ngp_get_frame_ambient_change on the ambient change alone; ngp_get_frame_sun_disk on the disk alone;
 *     ngp_get_frame_sun_shadow on the sun shadow and on whether the disk is on; ngp_get_frame_mesh_shadow on the meshes' shadow and on whether
 *     the disk is on. No other option changes a bit of it, and a getter refuses after every frame that did not run its pass.
 *   The disk and the sun shadow: the shadow list's entry of a pixel that owns a disk is live where V > 0, whatever M4 said of it, and dead where
 *     V = 0; a live entry is traced from q along the sun's centre and the pixel's sun colour is scaled by fl(V T_s). The mirror ray does not
 *     look at V: its q, r and t_hit are the G-buffer's position and normal alone, and the mirrored hit's shadow2 is the central ray.
 *   The ambient change and the meshes' shadow, with or without the disk: the ratio scales the scratch first, then the shadow's kernel (hard or
 *     soft) composites it: the pixel is fl(fl(n g) f) + m k, f = fl(1 - fl(strength fl(count / K))) with the disk.
 *   Where the NeRF wrote nothing (n.w == 0) the pixel is the mesh pass's of the same set without the meshes' shadow and the ambient change; where
 *     the primary ray found no triangle the pixel is that of the same set without the sun shadow, the reflection and its sub-option.
 *   No state survives a frame: a set gives the same colour, depth and records whichever sets and resolutions were rendered before it. */

/* mesh materials: a mesh may own a material, the BRDF part of ngp_geometry_opts; a mesh without one is shaded with the context's
 * ngp_geometry_opts, as every mesh is by default. The sun and up directions stay the context's. Defaults of a material's fields, as a scene
 * file's "material" object fills the keys it lacks: basecolor (0.8, 0.8, 0.8), ambientcolor (0, 0, 0), metallic 0, subsurface 0, specular 1,
 * roughness 0.5, sheen 0, clearcoat 0, clearcoat_gloss 0.
 *
 * Which material a shade uses: M5 at a pixel uses the material of the mesh whose triangle the pixel's primary ray hit -- the mesh the mesh trace
 *   chose, and only where it found a triangle. A covered pixel without a triangle (the ray that enters no box and is shaded at the camera)
 *   uses the context's. The mirror term's F (ngp_set_mesh_reflection) uses the pixel's material. The mirrored hit's C2
 *   (ngp_set_mesh_reflection_meshes) uses the material of the mesh the mirror ray hit. Nothing else reads a material: hits, q, depth, shadow
 *   booleans, disk counts and ray lists never depend on one.
 * Lifetime: a material belongs to its mesh slot. ngp_clear_meshes and ngp_load_scene drop all of them; a mesh added by ngp_add_mesh or
 *   ngp_load_mesh_file has none; ngp_set_geometry_opts never touches them. ngp_load_scene gives a "Mesh" entry that carries a "material"
 *   object that material.
 * Refusals, each naming the field and leaving the state alone: a mesh index outside [0, ngp_n_meshes); a non-finite field. Both calls work
 *   on a host-only context.
 * Identities as bytes: while no mesh owns a material, every frame, depth and record is what it was before materials existed, and the frame
 *   launches those very kernels. With every mesh owning a copy of the context's material, colour and depth are those bytes too. With any
 *   materials, depth and every geometric record (ngp_get_frame_sun_shadow, _sun_disk, _mesh_shadow, _ambient_change, _mesh_reflection, and
 *   (p2, shadow2) of _mesh_reflection_hits) are the no-material frame's bytes.
 * Determinism: no atomics; frames are bit-identical from run to run. The device table (64 bytes a mesh) is uploaded by ngp_set_mesh_material and
 *   by the calls that change the mesh list, never inside a frame: ngp_render_device stays asynchronous.
 * Several devices: the materials travel to the peers with the geometry; ngp_get_frame_mesh_ids reads the primary's share only.
 * Stated limits: the SH9 volume's bounce and sun passes read no material: a mesh's albedo there is its own where it owns one
 *   (ngp_set_mesh_albedo, "mesh albedos"), else the call's; no per-triangle or per-OBJ-group materials, no textures, no MTL files; the sun and
 *   up directions stay per context. */
typedef struct ngp_mesh_material {
	float metallic, subsurface, specular, roughness, sheen, clearcoat, clearcoat_gloss;
	float basecolor[3], ambientcolor[3];
} ngp_mesh_material;
NGP_API int ngp_set_mesh_material(ngp_ctx* ctx, int mesh, const ngp_mesh_material* m /* nullable: back to the context's */);
/* out (nullable) receives the mesh's own material, or where it owns none the context's BRDF fields; own (nullable) receives 1 or 0 */
NGP_API int ngp_get_mesh_material(ngp_ctx* ctx, int mesh, ngp_mesh_material* out, int* own);
/* stage entry for tests and tools: per pixel of the LAST frame's LAST sample, in the frame's own pixel order (packed or not; on several devices
 * the primary's share), the mesh index of the primary hit, -1 for every other pixel. n_pixels must be that frame's extent. Refuses after a
 * frame that ran without materials. */
NGP_API int ngp_get_frame_mesh_ids(ngp_ctx* ctx, int32_t* out /* n_pixels */, size_t n_pixels);


/* --- training: Testbed::reset_network (src/testbed.cu:3820-4210), Testbed::train (:4364-4470),
 * Testbed::train_nerf / train_nerf_step (src/testbed_nerf.cu:2949-3431), training_prep_nerf (:3432-3446). The default
 * path of configs/nerf/base.json: no envmap, no camera / exposure / latent optimisation, no error-map sampling,
 * no depth supervision. */
enum ngp_loss_type { NGP_LOSS_L2 = 0, NGP_LOSS_L1, NGP_LOSS_MAPE, NGP_LOSS_SMAPE, NGP_LOSS_HUBER, NGP_LOSS_LOGL1, NGP_LOSS_RELATIVE_L2 }; /* ELossType, common.h:84-92 */
enum ngp_image_type { NGP_IMAGE_NONE = 0, NGP_IMAGE_BYTE = 1, NGP_IMAGE_HALF = 2, NGP_IMAGE_FLOAT = 3 };                                    /* EImageDataType */
typedef struct ngp_training_opts {
	uint32_t struct_size;
	int32_t loss_type;              /* m_nerf.training.loss_type; configs/nerf/base.json: Huber */
	int32_t random_bg_color;        /* nerf.h defaults: true */
	int32_t linear_colors;          /* false */
	int32_t snap_to_pixel_centers;  /* true */
	float near_distance;            /* 0.1 */
	float density_grid_decay;       /* 0.95 */
	int32_t train_network, train_encoding; /* m_train_network / m_train_encoding -> optimize_matrix_params / optimize_non_matrix_params */
	/* configs/nerf/base.json "optimizer": Ema{decay} > ExponentialDecay{decay_start, decay_interval, decay_base} > Adam */
	float learning_rate, beta1, beta2, epsilon, l2_reg;
	float ema_decay;                /* 0: no Ema, inference uses the training parameters */
	uint32_t decay_start, decay_interval;
	float decay_base;
	float background_color[3];      /* m_background_color.rgb() when !random_bg_color */
	int32_t color_space;            /* m_color_space: 0 Linear, 1 SRGB */
} ngp_training_opts;
typedef struct ngp_training_state {
	uint32_t struct_size;
	uint32_t training_step;                          /* m_training_step */
	uint32_t rays_per_batch;                         /* counters_rgb.rays_per_batch */
	uint32_t measured_batch_size;                    /* samples after compaction in the last step */
	uint32_t measured_batch_size_before_compaction;  /* samples marched in the last step */
	uint32_t n_rays_total;
	float loss;                                      /* m_loss_scalar.val(): refreshed every 16th step like Testbed::train */
	float learning_rate;                             /* Adam's rate after ExponentialDecay */
	uint64_t n_params, n_matrix_params;
} ngp_training_state;
/* Testbed::reset_network for configs/nerf/base.json: fresh random parameters (xavier-uniform matrices, grid in
 * +-1e-4, pcg32 seeded with `seed`; the reference's m_seed is 1337), an empty occupancy grid, training counters at 0.
 * The boxes and aabb_scale come from the loaded dataset (ngp_load_training_data) or, without one, aabb_scale 1. */
NGP_API int ngp_reset_network(ngp_ctx* ctx, uint32_t log2_hashmap_size, uint64_t seed);
NGP_API void ngp_default_training_opts(ngp_training_opts* opts);
NGP_API int ngp_set_training_opts(ngp_ctx* ctx, const ngp_training_opts* opts);
NGP_API int ngp_get_training_opts(const ngp_ctx* ctx, ngp_training_opts* opts);
/* NerfDataset::set_training_image (src/nerf_loader.cu:745-): pixels of training view `view`, RGBA, NGP_IMAGE_BYTE
 * (sRGB, straight alpha) or NGP_IMAGE_FLOAT (linear, premultiplied -- python_api.cu nerf.training.set_image);
 * width/height replace the view's resolution */
NGP_API int ngp_set_training_image(ngp_ctx* ctx, int view, int32_t width, int32_t height, const void* rgba, int32_t image_type);
/* Decode the dataset's image files into training images (the reference does this inside load_nerf with stb_image,
 * src/nerf_loader.cu:520-640): PNG and baseline JPEG files -- views whose file is missing or of another format (EXR,
 * progressive JPEG ...) stay without pixels and take no part in training. Fails when no view could be loaded. */
NGP_API int ngp_load_training_images(ngp_ctx* ctx, int32_t* n_loaded_out);
/* The decoder behind it, on its own (needs no device): PNG (8/16-bit, non-interlaced) and baseline JPEG -> RGBA8.
 * rgba_out may be NULL to query the size; error_out (nullable) receives the reason on failure. */
NGP_API int ngp_decode_image(const void* bytes, size_t n_bytes, int32_t* width, int32_t* height, uint8_t* rgba_out, size_t rgba_capacity, char* error_out, size_t error_capacity);
/* m_render_ground_truth (python_api.cu:490-491; CudaRenderBuffer::overlay_image at alpha 1, src/render_buffer.cu:344-414, called
 * from Testbed::render_frame_epilogue, src/testbed.cu:4979-4994): the training image of `view`, resampled (nearest) to
 * width x height around the screen centre, over background_rgba (sRGB values), times 2^exposure, in linear or sRGB output --
 * what scripts/run.py --test_transforms compares the render with (run.py:236-241). color_space: m_color_space (0 Linear,
 * 1 SRGB); fov_axis / zoom: m_fov_axis / m_zoom. Host float RGBA out. */
NGP_API int ngp_render_ground_truth(ngp_ctx* ctx, int view, int32_t width, int32_t height, const float* background_rgba, float exposure, int32_t color_space, int32_t to_srgb,
                                    int32_t fov_axis, float zoom, float* rgba_out);
/* n_steps x Testbed::train(batch_size): occupancy-grid refresh on training_prep_nerf's schedule, one train_nerf_step,
 * the optimizer, the counters; loss_out (nullable) receives the running loss. batch_size: a multiple of 128, 2^18 in the
 * reference's GUI and scripts/run.py */
NGP_API int ngp_train(ngp_ctx* ctx, uint32_t n_steps, uint32_t batch_size, float* loss_out);
NGP_API int ngp_get_training_state(const ngp_ctx* ctx, ngp_training_state* out);
/* The pieces of one step, for parity tests against the oracle. ngp_train_prepare_batch: sample generation + network +
 * loss for the current step (no parameter changes); the buffers (host pointers, nullable) receive ray_indices[n_rays],
 * numsteps[n_rays][2] (after compaction), coords_compacted[target][7], dloss fp16 [target][4], loss[n_rays];
 * counters3 = {samples marched, rays kept, samples after compaction}. ngp_train_gradients: the fused backward on that
 * batch, gradient of every parameter in snapshot order (loss-scaled by 128 like the reference). ngp_train_apply: the
 * optimizer step on the gradient currently held + the step bookkeeping. */
NGP_API int ngp_train_prepare_batch(ngp_ctx* ctx, uint32_t batch_size, uint32_t* counters3, uint32_t* ray_indices, uint32_t* numsteps, float* coords_compacted,
                                    uint16_t* dloss_fp16, float* loss);
NGP_API int ngp_train_gradients(ngp_ctx* ctx, uint32_t batch_size, float* grad_out /* n_params */);
NGP_API int ngp_train_apply(ngp_ctx* ctx);
/* current training parameters (fp32 master copy) and their Ema (fp16 -> fp32), n_params each, nullable */
NGP_API int ngp_get_training_params(ngp_ctx* ctx, float* params_out, float* ema_out);


/* --- marching cubes: Testbed::compute_marching_cubes_mesh / compute_and_save_marching_cubes_mesh (python_api.cu; scripts/run.py
 * --save_mesh). The reference's marching_cubes.cu is not part of this project's sources: what upstream instant-ngp does is marked
 * (upstream); the rest is this project's own contract.
 * Lattice: res3 = (rx, ry, rz), each in [2, 1024], at most 2^30 points. aabb6 = min xyz, max xyz in ngp space (NULL: the render aabb),
 * finite and max > min on every axis. Point (i, j, k) sits at p = R^T (aabb.min + (aabb.max - aabb.min) * (i, j, k) / (res - 1)), R the
 * render aabb's to_local (generate_grid_samples_nerf_uniform, upstream), and holds the ACTIVATED density network_to_density(logit,
 * density_activation) of the density head at warp_position(p, scene aabb); fp32, index i + rx (j + ry k). Grid models (every head the
 * loader serves) and Frequency / Identity models.
 * Vertices: a lattice point is inside when density > thresh (strictly); each lattice edge whose ends differ gets exactly one vertex at
 * t = (thresh - d0) / (d1 - d0) (fp32) along it, placed by the lattice formula at (i, j, k) + t e_axis. Vertex order: the linear index
 * of the edge's lower end (x fastest), then axis x < y < z; no atomics decide it, the output is bit-identical from run to run.
 * Triangles: a 256-case table generated by one stated rule (csrc/mc_table.h) whose face decisions depend on the face's corners alone,
 * so a smooth closed surface gives a watertight mesh; at most 5 per cell. Order: linear cell index (x fastest), then table order.
 * uint32 indices; the counter-clockwise normal points from the dense side to the empty side.
 * Normals: -grad sigma / |grad sigma| at the vertex from the density-gradient stage behind NGP_RENDER_NORMALS; (0, 0, 0) where the
 * gradient is zero or not finite. Upstream derives them from the mesh's 1-ring instead.
 * Colours: sigmoid of the rgb logits of the full network at the vertex, direction normalize(p - 0.5) (upstream
 * generate_nerf_network_inputs_from_positions' outward choice), through the ngp_network_inference path of the model.
 * Files (ngp_save_marching_cubes_mesh): by extension, .obj or .ply (anything else is refused); positions in dataset space
 * (p - offset) / scale per axis, no axis permutation (save_mesh(..., nerf_scale, nerf_offset), upstream).
 *   OBJ: "v x y z r g b" (positions %.9g, colours %.3f), "vn nx ny nz", "f a//a b//b c//c" (1-based).
 *   PLY: ASCII; x y z nx ny nz float, red green blue uchar, "property list uchar int vertex_index". Both keep the winding above
 *   (upstream's PLY writes the indices reversed).
 *   A mesh of a caller's lattice has neither: "v x y z" / "f a b c", and x y z alone in the PLY.
 * Refused with a message: a host-only context ("no HIP device"), no model, a resolution out of range, an empty or non-finite aabb,
 * a non-finite thresh. */
/* the lattice alone, host out[rx * ry * rz] (a stage entry for tests) */
NGP_API int ngp_density_on_grid(ngp_ctx* ctx, const uint32_t* res3, const float* aabb6, float* out);
/* marching cubes on a lattice the caller supplies (host density[rx * ry * rz], laid out as above); the mesh is kept in the context and has
 * no normals or colours */
NGP_API int ngp_marching_cubes(ngp_ctx* ctx, const uint32_t* res3, const float* aabb6, float thresh, const float* density, uint32_t* n_verts, uint32_t* n_tris);
/* the whole pipeline: lattice, marching cubes, normals, colours; the mesh is kept in the context */
NGP_API int ngp_compute_marching_cubes_mesh(ngp_ctx* ctx, const uint32_t* res3, const float* aabb6, float thresh, uint32_t* n_verts, uint32_t* n_tris);
/* the kept mesh, ngp space: V, N, C n_verts x 3 floats, F n_tris x 3; each pointer nullable. N or C of a caller-lattice mesh is refused. */
NGP_API int ngp_get_marching_cubes_mesh(ngp_ctx* ctx, float* V, float* N, float* C, uint32_t* F);
NGP_API int ngp_save_marching_cubes_mesh(ngp_ctx* ctx, const char* path);
/* device time (HIP events) of the last ngp_compute_marching_cubes_mesh, ms: lattice, marching cubes (count, scan, read-back of the two
 * totals, emit), normals + colours. No counterpart in the reference; tools/mc_rate.py reads it. */
NGP_API int ngp_get_marching_cubes_timings(ngp_ctx* ctx, float* ms3);

#ifdef __cplusplus
}
#endif
#endif
