"""ctypes binding of libngp_hip.so -- the C ABI declared in include/ngp_hip.h.

This is the only way Python reaches the renderer: there is no CPU fallback. Loading fails loudly when the
library has not been built (run the package's build.py / __graft_entry__.build()), and every compute call
fails loudly when no HIP device is present.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libngp_hip.so")

HEADER_PATH = os.path.join(HERE, "..", "include", "ngp_hip.h")


def header_exports():
    """Every entry point include/ngp_hip.h declares (NGP_API ... name(...))."""
    import re

    with open(HEADER_PATH) as f:
        return re.findall(r"NGP_API\s+[\w\s\*]+?\b(ngp_\w+)\s*\(", f.read())


EXPORTS = header_exports()


def material_albedo(material):
    """the diffuse albedo the SH9 volume's passes take from a material (a dict of set_mesh_material's keys): the base colour squared per
    channel, clamped to [0, 1], formed in float32 -- what the mesh pass hands the BRDF"""
    base = np.asarray(material.get("basecolor", (0.8, 0.8, 0.8)), np.float32)
    return tuple(float(x) for x in np.minimum(np.maximum(base * base, np.float32(0.0)), np.float32(1.0)))


class ModelDesc(C.Structure):
    _fields_ = [
        ("n_levels", C.c_uint32), ("n_features_per_level", C.c_uint32), ("log2_hashmap_size", C.c_uint32), ("base_resolution", C.c_uint32),
        ("per_level_scale", C.c_float),
        ("n_neurons", C.c_uint32), ("n_hidden_density", C.c_uint32), ("n_hidden_rgb", C.c_uint32), ("density_out_dims", C.c_uint32),
        ("rgb_activation", C.c_uint32), ("density_activation", C.c_uint32),
        ("params_fp16", C.c_void_p), ("n_params", C.c_uint64),
        ("density_grid_fp16", C.c_void_p), ("n_density_grid", C.c_uint64),
        ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
        ("render_aabb_min", C.c_float * 3), ("render_aabb_max", C.c_float * 3),
        ("render_aabb_to_local", C.c_float * 9),
        ("aabb_scale", C.c_uint32), ("cone_angle_constant", C.c_float), ("linear_colors", C.c_int32),
        ("pos_encoding", C.c_uint32), ("pos_n_frequencies", C.c_uint32), ("dir_encoding", C.c_uint32), ("dir_n_frequencies", C.c_uint32),
        ("mlp_alignment", C.c_uint32),
    ]


class Camera(C.Structure):
    _fields_ = [
        ("matrix", C.c_float * 12), ("width", C.c_int32), ("height", C.c_int32), ("focal_length", C.c_float * 2),
        ("screen_center", C.c_float * 2), ("spp_index", C.c_uint32), ("snap_to_pixel_centers", C.c_int32), ("near_distance", C.c_float),
        ("lens_mode", C.c_int32), ("lens_params", C.c_float * 7), ("aperture_size", C.c_float), ("focus_z", C.c_float),
        ("has_matrix1", C.c_int32), ("matrix1", C.c_float * 12), ("rolling_shutter", C.c_float * 4),
    ]


class RenderOpts(C.Structure):
    _fields_ = [
        ("render_mode", C.c_int32), ("min_transmittance", C.c_float), ("background", C.c_float * 4), ("exposure", C.c_float),
        ("to_srgb", C.c_int32), ("spp", C.c_int32), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("testbed_mode", C.c_int32), ("packed_output", C.c_int32), ("depth_scale", C.c_float), ("color_space", C.c_int32),
    ]


class SessionState(C.Structure):
    _fields_ = [
        ("valid", C.c_int32), ("background_color", C.c_float * 4), ("exposure", C.c_float), ("sun_dir", C.c_float * 3), ("up_dir", C.c_float * 3),
        ("camera_scale", C.c_float), ("aperture_size", C.c_float), ("autofocus_depth", C.c_float),
    ]


class GeometryOpts(C.Structure):
    _fields_ = [
        ("sun_dir", C.c_float * 3), ("up_dir", C.c_float * 3),
        ("metallic", C.c_float), ("subsurface", C.c_float), ("specular", C.c_float), ("roughness", C.c_float),
        ("sheen", C.c_float), ("clearcoat", C.c_float), ("clearcoat_gloss", C.c_float),
        ("basecolor", C.c_float * 3), ("ambientcolor", C.c_float * 3),
    ]


class MeshMaterial(C.Structure):
    _fields_ = GeometryOpts._fields_[2:]  # (ngp_mesh_material: the BRDF part of ngp_geometry_opts)


MATERIAL_DEFAULTS = dict(metallic=0.0, subsurface=0.0, specular=1.0, roughness=0.5, sheen=0.0, clearcoat=0.0, clearcoat_gloss=0.0, basecolor=(0.8, 0.8, 0.8),
                         ambientcolor=(0.0, 0.0, 0.0))


class ProbeDesc(C.Structure):
    _fields_ = [("mode", C.c_int32), ("n_theta", C.c_uint32), ("n_phi", C.c_uint32), ("n_origin", C.c_uint32), ("origin", C.c_float * 3),
                ("min_transmittance", C.c_float)]


class ProbeGridDesc(C.Structure):
    _fields_ = [("grid_x", C.c_uint32), ("grid_y", C.c_uint32), ("n_theta", C.c_uint32), ("n_phi", C.c_uint32), ("shell_radius", C.c_float),
                ("min_transmittance", C.c_float)]


class IrradianceTraceDesc(C.Structure):
    _fields_ = [("n_u", C.c_uint32), ("n_v", C.c_uint32), ("offset", C.c_float), ("min_transmittance", C.c_float), ("occlude_by_meshes", C.c_int32)]


MODE_NERF, MODE_GEOMETRY = 0, 1
RENDER_SHADE, RENDER_SHADE_ENVMAP, RENDER_AO, RENDER_POSITIONS, RENDER_DEPTH, RENDER_COST, RENDER_SHADE_GRID_ENVMAP, RENDER_NORMALS = 0, 1, 2, 3, 4, 5, 6, 7
RENDER_SHADE_IRRADIANCE_VOLUME = 8  # meshes lit by the SH9 irradiance volume (compute_irradiance_volume / set_irradiance_volume)
PROBE_CENTER, PROBE_CENTER_OUTWARD, PROBE_MULTI_CENTER = 0, 1, 2
BVH_NODE_DTYPE = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left_idx", "<i4"), ("right_idx", "<i4")])
TRIANGLE_DTYPE = np.dtype([("a", "<f4", 3), ("b", "<f4", 3), ("c", "<f4", 3)])


class IrradianceShDesc(C.Structure):
    _fields_ = [("n_u", C.c_uint32), ("n_v", C.c_uint32), ("min_transmittance", C.c_float), ("occlude_by_meshes", C.c_int32)]


class IrradianceVolumeDesc(C.Structure):
    _fields_ = [("res", C.c_uint32 * 3), ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("sh", IrradianceShDesc)]


class IrradianceVisibilityDesc(C.Structure):
    _fields_ = [("n_u", C.c_uint32), ("n_v", C.c_uint32), ("sharpness_log2", C.c_uint32), ("max_distance", C.c_float), ("normal_bias", C.c_float)]


class IrradianceBounceDesc(C.Structure):
    _fields_ = [("n_bounces", C.c_uint32), ("albedo", C.c_float * 3)]


class IrradianceSunDesc(C.Structure):
    _fields_ = [("direction", C.c_float * 3), ("radiance", C.c_float * 3), ("shadow_bias", C.c_float)]


class IrradianceSunNerfDesc(C.Structure):
    _fields_ = [("min_transmittance", C.c_float), ("t_min", C.c_float)]


class MeshShadowOnNerfDesc(C.Structure):
    _fields_ = [("strength", C.c_float), ("bias", C.c_float)]


class SunDiskDesc(C.Structure):
    _fields_ = [("angular_radius", C.c_float), ("n_rays", C.c_uint32)]


SUN_ANGULAR_RADIUS = 0.00465  # the real sun's, rad


class AmbientChangeDesc(C.Structure):
    _fields_ = [("min_irradiance", C.c_float), ("max_gain", C.c_float)]


class MeshReflectionDesc(C.Structure):
    _fields_ = [("strength", C.c_float), ("min_transmittance", C.c_float), ("t_min", C.c_float)]


# the frame options with a descriptor, by the name in ngp_set_<name> / ngp_get_<name>: the struct and what True takes, field by field
FRAME_OPTIONS = {
    "sun_nerf_shadow": (IrradianceSunNerfDesc, dict(min_transmittance=0.01, t_min=0.0)),
    "mesh_shadow_on_nerf": (MeshShadowOnNerfDesc, dict(strength=0.5, bias=1e-2)),
    "ambient_change_on_nerf": (AmbientChangeDesc, dict(min_irradiance=1e-3, max_gain=4.0)),
    "mesh_reflection": (MeshReflectionDesc, dict(strength=1.0, min_transmittance=0.01, t_min=0.0)),
    "sun_disk": (SunDiskDesc, dict(angular_radius=SUN_ANGULAR_RADIUS, n_rays=16)),
}


SUN_RADIANCE = tuple(float(np.float32(c) / np.float32(255.0) * np.float32(4.0)) for c in (255.0, 225.0, 195.0))  # the frames' suncol


class RenderStats(C.Structure):
    _fields_ = [
        ("n_rays", C.c_uint64), ("n_rays_alive_after_init", C.c_uint64), ("n_rays_hit", C.c_uint64), ("n_samples", C.c_uint64),
        ("kernel_ms", C.c_float), ("frame_ms", C.c_float), ("kernel_device_ms", C.c_float),
    ]


PAYLOAD_DTYPE = np.dtype([("origin", "<f4", 3), ("dir", "<f4", 3), ("t", "<f4"), ("max_weight", "<f4"), ("idx", "<u4"),
                          ("n_steps", "<u2"), ("alive", "u1"), ("pad", "u1")])

_lib = None


class TrainingOpts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("loss_type", C.c_int32), ("random_bg_color", C.c_int32), ("linear_colors", C.c_int32), ("snap_to_pixel_centers", C.c_int32),
        ("near_distance", C.c_float), ("density_grid_decay", C.c_float), ("train_network", C.c_int32), ("train_encoding", C.c_int32),
        ("learning_rate", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float), ("l2_reg", C.c_float),
        ("ema_decay", C.c_float), ("decay_start", C.c_uint32), ("decay_interval", C.c_uint32), ("decay_base", C.c_float),
        ("background_color", C.c_float * 3), ("color_space", C.c_int32),
    ]


class TrainingState(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("training_step", C.c_uint32), ("rays_per_batch", C.c_uint32), ("measured_batch_size", C.c_uint32),
        ("measured_batch_size_before_compaction", C.c_uint32), ("n_rays_total", C.c_uint32), ("loss", C.c_float), ("learning_rate", C.c_float),
        ("n_params", C.c_uint64), ("n_matrix_params", C.c_uint64),
    ]


LOSS_TYPES = {"L2": 0, "L1": 1, "MAPE": 2, "SMAPE": 3, "Huber": 4, "LogL1": 5, "RelativeL2": 6}
IMAGE_BYTE, IMAGE_FLOAT = 1, 3


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    LIB_PATH = os.environ.get("NGP_HIP_LIBRARY") or globals()["LIB_PATH"]  # e.g. the legacy-encode variant, libngp_hip_legacy.so
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build the HIP extension first (python __graft_entry__.py or the package's build.py). "
                           "There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, ip = C.c_void_p, C.c_int
    L.ngp_create.argtypes = [ip]; L.ngp_create.restype = vp
    L.ngp_create_multi.argtypes = [vp, ip]; L.ngp_create_multi.restype = vp
    L.ngp_n_devices.argtypes = [vp]
    L.ngp_get_device_render_stats.argtypes = [vp, ip, C.POINTER(RenderStats)]
    L.ngp_destroy.argtypes = [vp]; L.ngp_destroy.restype = None
    L.ngp_last_error.argtypes = [vp]; L.ngp_last_error.restype = C.c_char_p
    L.ngp_version.restype = C.c_char_p
    L.ngp_set_model.argtypes = [vp, C.POINTER(ModelDesc)]
    L.ngp_load_snapshot.argtypes = [vp, vp, C.c_size_t, ip]
    L.ngp_load_snapshot_file.argtypes = [vp, C.c_char_p]
    L.ngp_save_snapshot_file.argtypes = [vp, C.c_char_p, ip]
    L.ngp_get_model.argtypes = [vp, C.POINTER(ModelDesc)]
    L.ngp_update_density_grid.argtypes = [vp, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32]
    L.ngp_get_density_grid.argtypes = [vp, vp, C.c_uint64]
    L.ngp_set_cone_angle_constant.argtypes = [vp, C.c_float]
    L.ngp_set_envmap.argtypes = [vp, C.c_int32, C.c_int32, vp]
    L.ngp_set_render_aabb.argtypes = [vp, vp, vp, vp]
    L.ngp_get_snapshot_camera.argtypes = [vp, vp, vp, vp, vp, vp]
    L.ngp_get_session_state.argtypes = [vp, C.POINTER(SessionState)]
    L.ngp_set_session_state.argtypes = [vp, C.POINTER(SessionState), vp, vp, C.c_int32, vp, C.c_float]
    L.ngp_load_training_data.argtypes = [vp, C.c_char_p]
    L.ngp_n_training_views.argtypes = [vp]
    L.ngp_get_training_view.argtypes = [vp, ip, vp, vp, vp, vp]
    L.ngp_get_training_view_lens.argtypes = [vp, ip, vp, vp]
    L.ngp_get_dataset_info.argtypes = [vp, vp, vp, vp, vp]
    L.ngp_render.argtypes = [vp, C.POINTER(Camera), C.POINTER(RenderOpts), vp, vp]
    L.ngp_render_device.argtypes = [vp, C.POINTER(Camera), C.POINTER(RenderOpts), vp, vp, vp]
    L.ngp_host_alloc.argtypes = [C.c_size_t]; L.ngp_host_alloc.restype = vp
    L.ngp_host_free.argtypes = [vp]; L.ngp_host_free.restype = None
    L.ngp_packed_tiles.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.c_uint32]
    L.ngp_packed_tiles.restype = C.c_uint32
    L.ngp_get_render_stats.argtypes = [vp, C.POINTER(RenderStats)]
    L.ngp_get_mesh_pass_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_get_render_history.argtypes = [vp, ip, C.POINTER(RenderStats)]
    L.ngp_set_schedule.argtypes = [vp, vp, ip]
    if hasattr(L, "ngp_last_render_kernel"):  # (an older build loaded through NGP_HIP_LIBRARY for an A/B run lacks it)
        L.ngp_last_render_kernel.argtypes = [vp]; L.ngp_last_render_kernel.restype = C.c_char_p
    if hasattr(L, "ngp_get_culled_tiles"):  # (an older build loaded through NGP_HIP_LIBRARY for an A/B run lacks it)
        L.ngp_get_culled_tiles.argtypes = [vp, C.POINTER(C.c_uint64)]
    if hasattr(L, "ngp_get_profile_trace"):  # (diagnostic entry; an older build loaded through NGP_HIP_LIBRARY for an A/B run lacks it)
        L.ngp_get_profile_trace.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.ngp_grid_encode.argtypes = [vp, C.c_uint32, vp, vp]
    L.ngp_network_inference.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.ngp_density_gradient.argtypes = [vp, C.c_uint32, vp, vp]
    L.ngp_get_density_bitfield.argtypes = [vp, vp, vp]
    L.ngp_density_on_grid.argtypes = [vp, vp, vp, vp]
    L.ngp_marching_cubes.argtypes = [vp, vp, vp, C.c_float, vp, vp, vp]
    L.ngp_compute_marching_cubes_mesh.argtypes = [vp, vp, vp, C.c_float, vp, vp]
    L.ngp_get_marching_cubes_mesh.argtypes = [vp, vp, vp, vp, vp]
    L.ngp_save_marching_cubes_mesh.argtypes = [vp, C.c_char_p]
    L.ngp_get_marching_cubes_timings.argtypes = [vp, vp]
    L.ngp_init_rays.argtypes = [vp, C.POINTER(Camera), vp]
    L.ngp_load_scene.argtypes = [vp, C.c_char_p]
    L.ngp_add_mesh.argtypes = [vp, vp, C.c_uint32, vp]
    L.ngp_load_mesh_file.argtypes = [vp, C.c_char_p, vp]
    L.ngp_clear_meshes.argtypes = [vp]
    L.ngp_n_meshes.argtypes = [vp]
    L.ngp_get_mesh_info.argtypes = [vp, ip, vp, vp, vp]
    L.ngp_get_mesh_bvh.argtypes = [vp, ip, vp, vp]
    L.ngp_set_geometry_opts.argtypes = [vp, C.POINTER(GeometryOpts)]
    L.ngp_trace_mesh_rays.argtypes = [vp, C.c_uint32, vp, vp]
    L.ngp_set_mesh_material.argtypes = [vp, ip, C.POINTER(MeshMaterial)]
    L.ngp_get_mesh_material.argtypes = [vp, ip, C.POINTER(MeshMaterial), C.POINTER(C.c_int)]
    L.ngp_set_mesh_albedo.argtypes = [vp, ip, C.POINTER(C.c_float * 3)]
    L.ngp_get_mesh_albedo.argtypes = [vp, ip, C.POINTER(C.c_float * 3), C.POINTER(C.c_int)]
    L.ngp_get_frame_mesh_ids.argtypes = [vp, vp, C.c_size_t]
    L.ngp_compute_envmap.argtypes = [vp, C.POINTER(ProbeDesc), vp]
    L.ngp_get_envmap.argtypes = [vp, vp, vp, vp, vp]
    L.ngp_irradiance.argtypes = [vp, C.c_uint32, vp, vp]
    L.ngp_compute_envmap_grid.argtypes = [vp, C.POINTER(ProbeGridDesc), vp]
    L.ngp_get_envmap_grid.argtypes = [vp, C.POINTER(ProbeGridDesc), vp]
    L.ngp_irradiance_at.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.ngp_trace_nerf_rays.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_float, vp, vp]
    L.ngp_irradiance_rays.argtypes = [vp, C.c_uint32, vp, vp, C.POINTER(IrradianceTraceDesc), vp, vp, vp]
    L.ngp_irradiance_traced.argtypes = [vp, C.c_uint32, vp, vp, C.POINTER(IrradianceTraceDesc), vp]
    L.ngp_irradiance_sphere_rays.argtypes = [vp, C.c_uint32, vp, C.POINTER(IrradianceShDesc), vp, vp, vp]
    L.ngp_irradiance_sh_traced.argtypes = [vp, C.c_uint32, vp, C.POINTER(IrradianceShDesc), vp, vp]
    L.ngp_irradiance_sh_eval.argtypes = [C.c_uint32, vp, vp, vp]
    L.ngp_compute_irradiance_volume.argtypes = [vp, C.POINTER(IrradianceVolumeDesc)]
    L.ngp_get_irradiance_volume.argtypes = [vp, C.POINTER(IrradianceVolumeDesc), vp]
    L.ngp_set_irradiance_volume.argtypes = [vp, C.POINTER(IrradianceVolumeDesc), vp]
    L.ngp_clear_irradiance_volume.argtypes = [vp]
    L.ngp_irradiance_volume_at.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.ngp_irradiance_distance_maps.argtypes = [vp, C.c_uint32, vp, C.POINTER(IrradianceVisibilityDesc), vp]
    L.ngp_compute_irradiance_volume_visibility.argtypes = [vp, C.POINTER(IrradianceVisibilityDesc)]
    L.ngp_get_irradiance_volume_visibility.argtypes = [vp, C.POINTER(IrradianceVisibilityDesc), vp]
    L.ngp_set_irradiance_volume_visibility.argtypes = [vp, C.POINTER(IrradianceVisibilityDesc), vp]
    L.ngp_clear_irradiance_volume_visibility.argtypes = [vp]
    L.ngp_irradiance_volume_at_visible.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.ngp_compute_irradiance_volume_bounced.argtypes = [vp, C.POINTER(IrradianceVolumeDesc), C.POINTER(IrradianceBounceDesc), C.POINTER(IrradianceVisibilityDesc)]
    L.ngp_irradiance_sh_bounce.argtypes = [vp, C.c_uint32, vp, C.POINTER(IrradianceShDesc), vp, vp, C.c_int, vp, vp]
    L.ngp_get_irradiance_bounce_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_compute_irradiance_volume_sunlit.argtypes = [vp, C.POINTER(IrradianceVolumeDesc), C.POINTER(IrradianceBounceDesc), C.POINTER(IrradianceVisibilityDesc),
                                                       C.POINTER(IrradianceSunDesc)]
    L.ngp_irradiance_sh_sun.argtypes = [vp, C.c_uint32, vp, C.POINTER(IrradianceShDesc), C.POINTER(IrradianceSunDesc), vp, vp, vp, vp]
    L.ngp_get_irradiance_sun_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_compute_irradiance_volume_sunlit_shadowed.argtypes = [vp, C.POINTER(IrradianceVolumeDesc), C.POINTER(IrradianceBounceDesc), C.POINTER(IrradianceVisibilityDesc),
                                                                C.POINTER(IrradianceSunDesc), C.POINTER(IrradianceSunNerfDesc)]
    L.ngp_irradiance_sh_sun_shadowed.argtypes = [vp, C.c_uint32, vp, C.POINTER(IrradianceShDesc), C.POINTER(IrradianceSunDesc), vp, vp, C.POINTER(IrradianceSunNerfDesc), vp, vp, vp]
    L.ngp_get_irradiance_sun_shadow_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_set_sun_nerf_shadow.argtypes = [vp, C.POINTER(IrradianceSunNerfDesc)]
    L.ngp_get_sun_nerf_shadow.argtypes = [vp, C.POINTER(IrradianceSunNerfDesc), C.POINTER(C.c_int)]
    L.ngp_get_frame_sun_shadow.argtypes = [vp, vp, C.c_size_t]
    L.ngp_get_frame_sun_shadow_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_set_mesh_shadow_on_nerf.argtypes = [vp, C.POINTER(MeshShadowOnNerfDesc)]
    L.ngp_get_mesh_shadow_on_nerf.argtypes = [vp, C.POINTER(MeshShadowOnNerfDesc), C.POINTER(C.c_int)]
    L.ngp_get_frame_mesh_shadow.argtypes = [vp, vp, C.c_size_t]
    L.ngp_get_frame_mesh_shadow_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_set_sun_disk.argtypes = [vp, C.POINTER(SunDiskDesc)]
    L.ngp_get_sun_disk.argtypes = [vp, C.POINTER(SunDiskDesc), C.POINTER(C.c_int)]
    L.ngp_sun_disk_directions.argtypes = [vp, vp, C.c_uint32, vp]
    L.ngp_get_frame_sun_disk.argtypes = [vp, vp, C.c_size_t]
    L.ngp_get_frame_sun_disk_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_compute_reference_irradiance_volume.argtypes = [vp, C.POINTER(IrradianceVolumeDesc)]
    L.ngp_get_reference_irradiance_volume.argtypes = [vp, C.POINTER(IrradianceVolumeDesc), vp]
    L.ngp_set_reference_irradiance_volume.argtypes = [vp, C.POINTER(IrradianceVolumeDesc), vp]
    L.ngp_clear_reference_irradiance_volume.argtypes = [vp]
    L.ngp_set_ambient_change_on_nerf.argtypes = [vp, C.POINTER(AmbientChangeDesc)]
    L.ngp_get_ambient_change_on_nerf.argtypes = [vp, C.POINTER(AmbientChangeDesc), C.POINTER(C.c_int)]
    L.ngp_irradiance_volume_ratio.argtypes = [vp, C.c_uint32, vp, vp, C.POINTER(AmbientChangeDesc), vp]
    L.ngp_get_frame_ambient_change.argtypes = [vp, vp, C.c_size_t]
    L.ngp_get_frame_ambient_change_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_set_mesh_reflection.argtypes = [vp, C.POINTER(MeshReflectionDesc)]
    L.ngp_get_mesh_reflection.argtypes = [vp, C.POINTER(MeshReflectionDesc), C.POINTER(C.c_int)]
    L.ngp_get_frame_mesh_reflection.argtypes = [vp, vp, C.c_size_t]
    L.ngp_get_frame_mesh_reflection_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_set_mesh_reflection_meshes.argtypes = [vp, C.c_int]
    L.ngp_get_mesh_reflection_meshes.argtypes = [vp, C.POINTER(C.c_int)]
    L.ngp_get_frame_mesh_reflection_hits.argtypes = [vp, vp, C.c_size_t]
    L.ngp_get_frame_mesh_reflection_hits_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ngp_reset_network.argtypes = [vp, C.c_uint32, C.c_uint64]
    L.ngp_default_training_opts.argtypes = [C.POINTER(TrainingOpts)]; L.ngp_default_training_opts.restype = None
    L.ngp_set_training_opts.argtypes = [vp, C.POINTER(TrainingOpts)]
    L.ngp_get_training_opts.argtypes = [vp, C.POINTER(TrainingOpts)]
    L.ngp_set_training_image.argtypes = [vp, ip, C.c_int32, C.c_int32, vp, C.c_int32]
    L.ngp_train.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.ngp_load_training_images.argtypes = [vp, vp]
    L.ngp_render_ground_truth.argtypes = [vp, ip, C.c_int32, C.c_int32, vp, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_float, vp]
    L.ngp_decode_image.argtypes = [vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, C.c_size_t]
    L.ngp_get_training_state.argtypes = [vp, C.POINTER(TrainingState)]
    L.ngp_train_prepare_batch.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.ngp_train_gradients.argtypes = [vp, C.c_uint32, vp]
    L.ngp_train_apply.argtypes = [vp]
    L.ngp_get_training_params.argtypes = [vp, vp, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


LENS_PERSPECTIVE, LENS_OPENCV, LENS_FTHETA, LENS_LATLONG, LENS_OPENCV_FISHEYE, LENS_EQUIRECTANGULAR = range(6)


def host_image(shape):
    """float32 array in page-locked memory from ngp_host_alloc; the buffer returns to the pool when the array is collected"""
    import weakref

    L = load_library()
    count = int(np.prod(shape))
    p = L.ngp_host_alloc(count * 4)
    if not p:
        raise MemoryError("ngp_host_alloc failed")
    buf = (C.c_float * count).from_address(p)
    weakref.finalize(buf, L.ngp_host_free, p)
    return np.ctypeslib.as_array(buf).reshape(shape)


def decode_image(data):
    """PNG / baseline JPEG bytes -> (H, W, 4) uint8 through the library's decoder."""
    L = load_library()
    w, h = C.c_int32(0), C.c_int32(0)
    err = C.create_string_buffer(256)
    if L.ngp_decode_image(data, len(data), C.byref(w), C.byref(h), None, 0, err, 256) != 0:
        raise RuntimeError(err.value.decode())
    out = np.zeros((h.value, w.value, 4), np.uint8)
    if L.ngp_decode_image(data, len(data), C.byref(w), C.byref(h), _p(out), out.size, err, 256) != 0:
        raise RuntimeError(err.value.decode())
    return out


def make_camera(matrix_3x4, width, height, focal_length, screen_center=(0.5, 0.5), spp_index=0, snap=True, near=0.0, lens_mode=0, lens_params=(), aperture_size=0.0, focus_z=1.0,
                matrix1_3x4=None, rolling_shutter=(0.0, 0.0, 0.0, 1.0)):
    cam = Camera()
    mat = np.asarray(matrix_3x4, np.float32)
    assert mat.shape == (3, 4)
    for c in range(4):
        for r in range(3):
            cam.matrix[c * 3 + r] = mat[r, c]
    cam.width, cam.height = int(width), int(height)
    cam.focal_length[0], cam.focal_length[1] = focal_length
    cam.screen_center[0], cam.screen_center[1] = screen_center
    cam.spp_index = spp_index
    cam.snap_to_pixel_centers = 1 if snap else 0
    cam.near_distance = near
    cam.lens_mode = lens_mode
    for i, q in enumerate(lens_params):
        cam.lens_params[i] = q
    cam.aperture_size, cam.focus_z = aperture_size, focus_z
    if matrix1_3x4 is not None:  # the camera at the end of the frame's interval (camera_matrix1) + rolling shutter
        m1 = np.asarray(matrix1_3x4, np.float32)
        cam.has_matrix1 = 1
        for c in range(4):
            for r in range(3):
                cam.matrix1[c * 3 + r] = m1[r, c]
        for i in range(4):
            cam.rolling_shutter[i] = rolling_shutter[i]
    return cam


def make_opts(min_transmittance=0.01, background=(0.0, 0.0, 0.0, 1.0), exposure=0.0, to_srgb=False, spp=1, shard_index=0, shard_count=1,
              testbed_mode=MODE_NERF, render_mode=RENDER_SHADE, packed_output=False, depth_scale=0.0, color_space=0):
    o = RenderOpts()
    o.render_mode = render_mode
    o.min_transmittance = min_transmittance
    for i in range(4):
        o.background[i] = background[i]
    o.exposure = exposure
    o.to_srgb = int(to_srgb)
    o.spp = spp
    o.shard_index, o.shard_count = shard_index, shard_count
    o.testbed_mode = testbed_mode
    o.packed_output = int(packed_output)
    o.depth_scale = depth_scale
    o.color_space = color_space
    return o


def irradiance_sh_eval(sh, normals):
    """E(n) of SH9 probe records (n, 28) at normals (n, 3), normalised by the library: (n, 3). Host code; no context, no device."""
    sh = np.ascontiguousarray(sh, np.float32).reshape(-1, 28)
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if sh.shape[0] != nrm.shape[0]:
        raise ValueError("records (n, 28) and normals (n, 3)")
    out = np.zeros((sh.shape[0], 3), np.float32)
    rc = load_library().ngp_irradiance_sh_eval(sh.shape[0], _p(sh), _p(nrm), _p(out))
    if rc != 0:
        raise RuntimeError("ngp_irradiance_sh_eval: " + ("a normal is zero or not finite" if rc == -1 else "null argument"))
    return out


class Context:
    """One ngp_ctx. Errors from the C ABI become RuntimeError (like the reference's exceptions through pybind11)."""

    def __init__(self, device=0, devices=None):
        """device: one HIP ordinal (-1: host-only). devices: a list of ordinals -> ngp_create_multi (the first is the primary)."""
        self.L = load_library()
        if devices is not None:
            arr = np.asarray(devices, np.int32)
            self.h = self.L.ngp_create_multi(_p(arr), arr.size)
        else:
            self.h = self.L.ngp_create(device)
        if not self.h:
            raise RuntimeError("ngp_create failed: no HIP device available (libngp_hip has no CPU fallback), or NGP_TUNE was refused (the library names the knob on stderr)")

    def n_devices(self):
        return self.L.ngp_n_devices(self.h)

    def device_render_stats(self, index):
        st = RenderStats()
        self._check(self.L.ngp_get_device_render_stats(self.h, index, C.byref(st)))
        return {k: getattr(st, k) for k, _ in RenderStats._fields_}

    def close(self):
        if getattr(self, "h", None):
            self.L.ngp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.ngp_last_error(self.h).decode(errors="replace"))

    def set_schedule(self, *knobs):
        """refill_min, skip_steps, go_min, max_stall, k_busy, k_drain, block_jumps, share (ngp_set_schedule: validated)"""
        a = np.asarray(knobs, np.int32)
        self._check(self.L.ngp_set_schedule(self.h, _p(a), a.size))

    def profile_trace(self):
        """Wave timelines of the last frame (diagnostic build: NGP_PROFILE_SECTIONS + NGP_PROFILE_TRACE): (n_working_waves, headers [W, 16], records [W, I, 16])"""
        cw, ci = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        self._check(self.L.ngp_get_profile_trace(self.h, None, 0, _p(cw), _p(ci)))
        w, it = int(cw[0]), int(ci[0])
        buf = np.zeros(16 + w * 16 + w * it * 16, np.uint32)
        self._check(self.L.ngp_get_profile_trace(self.h, _p(buf), buf.size, None, None))
        return int(buf[0]), buf[16:16 + w * 16].reshape(w, 16), buf[16 + w * 16:].reshape(w, it, 16)

    # ---------------------------------------------------------------- model
    def set_model(self, scene):
        d = ModelDesc()
        enc = scene["encoding"]
        if enc.get("otype") in ("Frequency", "Identity"):  # configs/nerf/frequency.json, none.json
            if enc["otype"] == "Identity":
                d.pos_encoding = 2
            else:
                d.pos_encoding, d.pos_n_frequencies = 1, enc["n_frequencies"]
            de = scene.get("dir_encoding", {})
            if de.get("otype") == "Frequency":
                d.dir_encoding, d.dir_n_frequencies = 1, de["n_frequencies"]
            elif de.get("otype") == "Identity":
                d.dir_encoding = 2
            if scene["network"].get("otype", "FullyFusedMLP") != scene["rgb_network"].get("otype", "FullyFusedMLP"):
                raise ValueError("Frequency encodings: the density and the rgb network must be of the same otype")
        else:
            d.n_levels, d.n_features_per_level = enc["n_levels"], enc["n_features_per_level"]
            d.log2_hashmap_size, d.base_resolution = enc["log2_hashmap_size"], enc["base_resolution"]
            d.per_level_scale = enc["per_level_scale"]
        # the rgb network's alignment (nerf_network.h:83): 8 for CutlassMLP (linear.json, base_0layer.json, frequency.json)
        d.mlp_alignment = 8 if scene["rgb_network"].get("otype", "FullyFusedMLP") == "CutlassMLP" else 16
        d.n_neurons = scene["network"]["n_neurons"]
        d.n_hidden_density = scene["network"]["n_hidden_layers"]
        d.n_hidden_rgb = scene["rgb_network"]["n_hidden_layers"]
        d.density_out_dims = scene["network"].get("n_output_dims", 16)
        d.rgb_activation = scene.get("rgb_activation", 2)
        d.density_activation = scene.get("density_activation", 3)
        params = np.ascontiguousarray(scene["params"], np.uint16)
        grid = np.ascontiguousarray(np.asarray(scene["density_grid"]).astype(np.float16)).view(np.uint16)
        d.params_fp16, d.n_params = params.ctypes.data, params.size
        d.density_grid_fp16, d.n_density_grid = grid.ctypes.data, grid.size
        for i in range(3):
            d.aabb_min[i], d.aabb_max[i] = scene["aabb"][0][i], scene["aabb"][1][i]
            d.render_aabb_min[i], d.render_aabb_max[i] = scene["render_aabb"][0][i], scene["render_aabb"][1][i]
        r2l = np.asarray(scene.get("render_aabb_to_local", np.eye(3)), np.float32)
        for c in range(3):
            for r in range(3):
                d.render_aabb_to_local[c * 3 + r] = r2l[r, c]
        d.aabb_scale = scene["aabb_scale"]
        d.cone_angle_constant = scene["cone_angle_constant"]
        d.linear_colors = int(scene.get("linear_colors", False))
        self._check(self.L.ngp_set_model(self.h, C.byref(d)))

    def load_snapshot_bytes(self, data, compressed=False):
        buf = np.frombuffer(data, np.uint8)
        self._check(self.L.ngp_load_snapshot(self.h, _p(buf), buf.size, int(compressed)))

    def load_snapshot_file(self, path):
        self._check(self.L.ngp_load_snapshot_file(self.h, os.fsencode(path)))

    def save_snapshot_file(self, path, compress=True):
        self._check(self.L.ngp_save_snapshot_file(self.h, os.fsencode(path), int(compress)))

    def get_model(self):
        d = ModelDesc()
        self._check(self.L.ngp_get_model(self.h, C.byref(d)))
        return d

    def get_scene(self):
        """The loaded model as the dict set_model takes (and the oracle's make_model): what a snapshot left behind, copied out of the context"""
        from . import scene as S

        d = self.get_model()
        if d.pos_encoding != 0:
            raise RuntimeError("get_scene: grid models only")
        params = np.ctypeslib.as_array(C.cast(d.params_fp16, C.POINTER(C.c_uint16)), shape=(int(d.n_params),)).copy()
        grid = np.ctypeslib.as_array(C.cast(d.density_grid_fp16, C.POINTER(C.c_uint16)), shape=(int(d.n_density_grid),)).copy().view(np.float16)
        r2l = np.array([[d.render_aabb_to_local[c * 3 + r] for c in range(3)] for r in range(3)], np.float32)
        return {
            "encoding": {"otype": "HashGrid", "n_levels": d.n_levels, "n_features_per_level": d.n_features_per_level, "log2_hashmap_size": d.log2_hashmap_size,
                         "base_resolution": d.base_resolution, "per_level_scale": float(d.per_level_scale)},
            "network": {"otype": "CutlassMLP" if d.n_hidden_density == 0 else "FullyFusedMLP", "n_neurons": d.n_neurons, "n_hidden_layers": d.n_hidden_density, "n_output_dims": d.density_out_dims},
            "rgb_network": {"otype": "CutlassMLP" if d.mlp_alignment == 8 else "FullyFusedMLP", "n_neurons": d.n_neurons, "n_hidden_layers": d.n_hidden_rgb},
            "rgb_activation": d.rgb_activation, "density_activation": d.density_activation,
            "params": params, "density_grid": grid,
            "aabb": (tuple(d.aabb_min), tuple(d.aabb_max)), "render_aabb": (tuple(d.render_aabb_min), tuple(d.render_aabb_max)), "render_aabb_to_local": r2l,
            "aabb_scale": d.aabb_scale, "max_cascade": S.max_cascade_for(d.aabb_scale), "cone_angle_constant": float(d.cone_angle_constant), "linear_colors": bool(d.linear_colors),
        }

    def session_state(self):
        st = SessionState()
        self._check(self.L.ngp_get_session_state(self.h, C.byref(st)))
        return st

    def set_session_state(self, st, matrix_3x4=None, relative_focal_length=(1.0, 1.0), fov_axis=1, screen_center=(0.5, 0.5), zoom=1.0):
        m = None if matrix_3x4 is None else np.ascontiguousarray(np.asarray(matrix_3x4, np.float32).T.reshape(-1))
        rfl = np.asarray(relative_focal_length, np.float32); sc = np.asarray(screen_center, np.float32)
        self._check(self.L.ngp_set_session_state(self.h, C.byref(st), _p(m) if m is not None else None, _p(rfl), fov_axis, _p(sc), zoom))

    def snapshot_camera(self):
        m = np.zeros(12, np.float32); rfl = np.zeros(2, np.float32); sc = np.zeros(2, np.float32)
        ax = C.c_int32(0); zoom = C.c_float(0)
        if self.L.ngp_get_snapshot_camera(self.h, _p(m), _p(rfl), C.addressof(ax), _p(sc), C.addressof(zoom)) != 0:
            return None
        return {"matrix": m.reshape(4, 3).T.copy(), "relative_focal_length": rfl, "fov_axis": ax.value, "screen_center": sc, "zoom": zoom.value}

    # ---------------------------------------------------------------- data
    def load_training_data(self, path):
        self._check(self.L.ngp_load_training_data(self.h, os.fsencode(path)))

    def n_training_views(self):
        return self.L.ngp_n_training_views(self.h)

    def training_view(self, i):
        m = np.zeros(12, np.float32); res = np.zeros(2, np.int32); fl = np.zeros(2, np.float32); pp = np.zeros(2, np.float32)
        if self.L.ngp_get_training_view(self.h, i, _p(m), _p(res), _p(fl), _p(pp)) != 0:
            raise IndexError(i)
        mode = C.c_int32(0); lp = np.zeros(7, np.float32)
        self.L.ngp_get_training_view_lens(self.h, i, C.addressof(mode), _p(lp))
        return {"matrix": m.reshape(4, 3).T.copy(), "resolution": res, "focal_length": fl, "principal_point": pp, "lens_mode": mode.value, "lens_params": lp}

    def dataset_info(self):
        a = C.c_int32(0); s = C.c_float(0); off = np.zeros(3, np.float32); hdr = C.c_int32(0)
        self._check(self.L.ngp_get_dataset_info(self.h, C.addressof(a), C.addressof(s), _p(off), C.addressof(hdr)))
        return {"aabb_scale": a.value, "scale": s.value, "offset": off, "is_hdr": bool(hdr.value)}

    # ---------------------------------------------------------------- render
    def render(self, cam, opts=None, want_depth=False):
        opts = opts or make_opts()
        if not (0 < cam.width <= 65536 and 0 < cam.height <= 65536):  # (the library refuses it: no image to allocate for the call)
            self._check(self.L.ngp_render(self.h, C.byref(cam), C.byref(opts), None, None))
        rgba = np.zeros((cam.height, cam.width, 4), np.float32)
        depth = np.zeros((cam.height, cam.width), np.float32) if want_depth else None
        self._check(self.L.ngp_render(self.h, C.byref(cam), C.byref(opts), _p(rgba), _p(depth) if want_depth else None))
        return (rgba, depth) if want_depth else rgba

    def render_pinned(self, cam, opts=None):
        """ngp_render into a page-locked buffer from the library's pool (what pyngp's Testbed.render does): one DMA, no staging"""
        opts = opts or make_opts()
        rgba = host_image((cam.height, cam.width, 4))
        self._check(self.L.ngp_render(self.h, C.byref(cam), C.byref(opts), _p(rgba), None))
        return rgba

    def render_device(self, cam, opts, d_rgba_ptr, d_depth_ptr=None, stream=None):
        self._check(self.L.ngp_render_device(self.h, C.byref(cam), C.byref(opts), d_rgba_ptr, d_depth_ptr, stream))

    def mesh_pass_ms(self):
        """device time of the last frame's mesh pass (its last sample), from HIP events on its stream"""
        ms = C.c_float(0)
        self._check(self.L.ngp_get_mesh_pass_ms(self.h, C.byref(ms)))
        return ms.value

    def render_stats(self):
        st = RenderStats()
        self._check(self.L.ngp_get_render_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in RenderStats._fields_}

    def last_render_kernel(self):
        """Name of the kernel the last frame ran ("render_nerf_fused_unit_plain", ..., "wide"; ngp_last_render_kernel)"""
        return self.L.ngp_last_render_kernel(self.h).decode()

    def culled_tiles(self):
        """8 x 8 camera tiles the last frame's unit render kernel dropped right after ray setup (ngp_get_culled_tiles; csrc/tile_probe.h)"""
        n = C.c_uint64(0)
        self._check(self.L.ngp_get_culled_tiles(self.h, C.byref(n)))
        return int(n.value)

    def render_history(self, n):
        arr = (RenderStats * n)()
        self._check(self.L.ngp_get_render_history(self.h, n, arr))
        return [{k: getattr(st, k) for k, _ in RenderStats._fields_} for st in arr]

    # ---------------------------------------------------------------- geometry mode
    def add_mesh(self, triangles, center=(0.0, 0.0, 0.0)):
        v = np.ascontiguousarray(triangles, np.float32).reshape(-1)
        c = np.asarray(center, np.float32)
        self._check(self.L.ngp_add_mesh(self.h, _p(v), v.size // 9, _p(c)))

    def load_mesh_file(self, path, center=(0.0, 0.0, 0.0)):
        c = np.asarray(center, np.float32)
        self._check(self.L.ngp_load_mesh_file(self.h, os.fsencode(path), _p(c)))

    def load_scene(self, path):
        self._check(self.L.ngp_load_scene(self.h, os.fsencode(path)))

    def clear_meshes(self):
        self._check(self.L.ngp_clear_meshes(self.h))

    def n_meshes(self):
        return self.L.ngp_n_meshes(self.h)

    def mesh_info(self, mesh=-1):
        nt, nn = C.c_uint32(0), C.c_uint32(0)
        bb = np.zeros(6, np.float32)
        if self.L.ngp_get_mesh_info(self.h, mesh, C.addressof(nt), C.addressof(nn), _p(bb)) != 0:
            raise IndexError(mesh)
        return {"n_tris": nt.value, "n_nodes": nn.value, "aabb": (bb[:3].copy(), bb[3:].copy())}

    def mesh_bvh(self, mesh):
        info = self.mesh_info(mesh)
        nodes = np.zeros(info["n_nodes"], BVH_NODE_DTYPE)
        tris = np.zeros(info["n_tris"], TRIANGLE_DTYPE)
        if self.L.ngp_get_mesh_bvh(self.h, mesh, _p(nodes), _p(tris)) != 0:
            raise IndexError(mesh)
        return nodes, tris

    def set_geometry_opts(self, sun_dir=(1.0, 1.0, 1.0), up_dir=(0.0, 1.0, 0.0), metallic=0.0, subsurface=0.0, specular=1.0, roughness=0.5,
                          sheen=0.0, clearcoat=0.0, clearcoat_gloss=0.0, basecolor=(0.8, 0.8, 0.8), ambientcolor=(0.0, 0.0, 0.0)):
        o = GeometryOpts()
        for i in range(3):
            o.sun_dir[i], o.up_dir[i], o.basecolor[i], o.ambientcolor[i] = sun_dir[i], up_dir[i], basecolor[i], ambientcolor[i]
        o.metallic, o.subsurface, o.specular, o.roughness = metallic, subsurface, specular, roughness
        o.sheen, o.clearcoat, o.clearcoat_gloss = sheen, clearcoat, clearcoat_gloss
        if self.L.ngp_set_geometry_opts(self.h, C.byref(o)) != 0:
            raise RuntimeError("ngp_set_geometry_opts failed")

    def set_mesh_material(self, mesh, material=None):
        """give mesh its own material: a dict with set_geometry_opts' BRDF keywords (metallic, subsurface, specular, roughness, sheen, clearcoat,
        clearcoat_gloss, basecolor, ambientcolor; a missing one takes that function's default), or None: back to the context's"""
        if material is None:
            self._check(self.L.ngp_set_mesh_material(self.h, int(mesh), None))
            return
        unknown = set(material) - set(MATERIAL_DEFAULTS)
        if unknown:
            raise ValueError("mesh material: unknown key(s) %s" % sorted(unknown))
        v = dict(MATERIAL_DEFAULTS, **material)
        m = MeshMaterial()
        for k in ("metallic", "subsurface", "specular", "roughness", "sheen", "clearcoat", "clearcoat_gloss"):
            setattr(m, k, v[k])
        for i in range(3):
            m.basecolor[i], m.ambientcolor[i] = v["basecolor"][i], v["ambientcolor"][i]
        self._check(self.L.ngp_set_mesh_material(self.h, int(mesh), C.byref(m)))

    def mesh_material(self, mesh):
        """the mesh's own material as a dict of set_mesh_material's keys, or None where it is shaded with the context's"""
        m, own = MeshMaterial(), C.c_int(0)
        self._check(self.L.ngp_get_mesh_material(self.h, int(mesh), C.byref(m), C.byref(own)))
        if not own.value:
            return None
        return {k: (tuple(getattr(m, k)) if k in ("basecolor", "ambientcolor") else getattr(m, k)) for k in MATERIAL_DEFAULTS}

    def set_mesh_albedo(self, mesh, rgb=None):
        """give mesh its own albedo in the SH9 volume's bounce and sun passes: three channels in [0, 1] (one number: all three), or None: back
        to the call's albedo"""
        if rgb is None:
            self._check(self.L.ngp_set_mesh_albedo(self.h, int(mesh), None))
            return
        a = (C.c_float * 3)(*[float(x) for x in np.broadcast_to(np.asarray(rgb, np.float32), (3,))])
        self._check(self.L.ngp_set_mesh_albedo(self.h, int(mesh), C.byref(a)))

    def mesh_albedo(self, mesh):
        """the mesh's own albedo as a tuple of three floats, or None where the volume's passes use the call's"""
        a, own = (C.c_float * 3)(), C.c_int(0)
        self._check(self.L.ngp_get_mesh_albedo(self.h, int(mesh), C.byref(a), C.byref(own)))
        return tuple(a) if own.value else None

    def frame_mesh_ids(self, n_pixels):
        """(n_pixels,) int32: per pixel of the last frame's last sample, in the frame's pixel order, the mesh its primary ray hit, -1 for every
        other pixel; refuses after a frame that ran without materials. On a multi-device context the primary's tile-packed share."""
        out = np.zeros(int(n_pixels), np.int32)
        self._check(self.L.ngp_get_frame_mesh_ids(self.h, _p(out), int(n_pixels)))
        return out

    def trace_mesh_rays(self, positions, directions):
        p = np.ascontiguousarray(positions, np.float32).copy()
        d = np.ascontiguousarray(directions, np.float32).copy()
        self._check(self.L.ngp_trace_mesh_rays(self.h, p.shape[0], _p(p), _p(d)))
        return p, d

    # ---------------------------------------------------------------- irradiance probes
    def compute_envmap(self, mode=PROBE_CENTER, n_theta=32, n_phi=16, n_origin=1, origin=(0.0, 0.0, 0.0), min_transmittance=0.01):
        d = ProbeDesc()
        d.mode, d.n_theta, d.n_phi, d.n_origin, d.min_transmittance = mode, n_theta, n_phi, n_origin, min_transmittance
        for i in range(3):
            d.origin[i] = origin[i]
        env = np.zeros((n_phi, n_theta, 4), np.float32)
        self._check(self.L.ngp_compute_envmap(self.h, C.byref(d), _p(env)))
        return env

    def get_envmap(self):
        nt, nph = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.ngp_get_envmap(self.h, C.addressof(nt), C.addressof(nph), None, None))
        env = np.zeros((nph.value, nt.value, 4), np.float32)
        irr = np.zeros((nph.value, nt.value, 4), np.float32)
        self._check(self.L.ngp_get_envmap(self.h, None, None, _p(env), _p(irr)))
        return env, irr

    def irradiance(self, normals):
        nrm = np.ascontiguousarray(normals, np.float32)
        out = np.zeros((nrm.shape[0], 3), np.float32)
        self._check(self.L.ngp_irradiance(self.h, nrm.shape[0], _p(nrm), _p(out)))
        return out

    def compute_envmap_grid(self, grid_x=4, grid_y=4, n_theta=32, n_phi=16, shell_radius=1.0, min_transmittance=0.01):
        """Testbed::computeEnvmapGrid: (grid_x * grid_y, n_phi, n_theta, 4) probe textures, all traced in one launch"""
        d = ProbeGridDesc()
        d.grid_x, d.grid_y, d.n_theta, d.n_phi, d.shell_radius, d.min_transmittance = grid_x, grid_y, n_theta, n_phi, shell_radius, min_transmittance
        env = np.zeros((grid_x * grid_y, n_phi, n_theta, 4), np.float32)
        self._check(self.L.ngp_compute_envmap_grid(self.h, C.byref(d), _p(env)))
        return env

    def get_envmap_grid(self):
        """(desc, shell positions (G, 3), textures (G, n_phi, n_theta, 4), irradiance tables (G, n_phi, n_theta, 4))"""
        d = ProbeGridDesc()
        self._check(self.L.ngp_get_envmap_grid(self.h, C.byref(d), None))
        g = d.grid_x * d.grid_y
        org = np.zeros((g, 3), np.float32)
        self._check(self.L.ngp_get_envmap_grid(self.h, C.byref(d), _p(org)))
        env = np.zeros((g, d.n_phi, d.n_theta, 4), np.float32)
        irr = np.zeros((g, d.n_phi, d.n_theta, 4), np.float32)
        self._check(self.L.ngp_get_envmap(self.h, None, None, _p(env), _p(irr)))
        return d, org, env, irr

    def irradiance_at(self, positions, normals):
        pos = np.ascontiguousarray(positions, np.float32)
        nrm = np.ascontiguousarray(normals, np.float32)
        out = np.zeros((nrm.shape[0], 3), np.float32)
        self._check(self.L.ngp_irradiance_at(self.h, nrm.shape[0], _p(pos), _p(nrm), _p(out)))
        return out

    # ---------------------------------------------------------------- traced irradiance (contract: include/ngp_hip.h)
    def trace_nerf_rays(self, origins, directions, t_range=None, min_transmittance=0.01):
        """the caller's rays (ngp space, n x 3 each; t_range None or n x 2 (t_min, t_max)) through the NeRF: (rgba n x 4, depth n)"""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        if d.shape != o.shape:
            raise ValueError("origins and directions: n x 3 each")
        t = None if t_range is None else np.ascontiguousarray(t_range, np.float32).reshape(o.shape[0], 2)
        rgba = np.zeros((o.shape[0], 4), np.float32)
        depth = np.zeros(o.shape[0], np.float32)
        self._check(self.L.ngp_trace_nerf_rays(self.h, o.shape[0], _p(o), _p(d), _p(t) if t is not None else None, min_transmittance, _p(rgba), _p(depth)))
        return rgba, depth

    @staticmethod
    def _irradiance_args(positions, normals, n_u, n_v, offset, occlude_by_meshes, min_transmittance):
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if p.shape != n.shape:
            raise ValueError("positions and normals: n x 3 each")
        d = IrradianceTraceDesc()
        d.n_u, d.n_v, d.offset, d.min_transmittance, d.occlude_by_meshes = n_u, n_v, offset, min_transmittance, int(bool(occlude_by_meshes))
        return p, n, d

    def irradiance_rays(self, positions, normals, n_u=16, n_v=16, offset=1e-4, occlude_by_meshes=True, min_transmittance=0.01):
        """the generator's hemisphere rays: (origins (n, K, 3), directions (n, K, 3), t_max (n, K)), K = n_u n_v, k = u + n_u v"""
        p, n, d = self._irradiance_args(positions, normals, n_u, n_v, offset, occlude_by_meshes, min_transmittance)
        k = int(n_u) * int(n_v)
        o = np.zeros((p.shape[0], k, 3), np.float32)
        dr = np.zeros((p.shape[0], k, 3), np.float32)
        t = np.zeros((p.shape[0], k), np.float32)
        self._check(self.L.ngp_irradiance_rays(self.h, p.shape[0], _p(p), _p(n), C.byref(d), _p(o), _p(dr), _p(t)))
        return o, dr, t

    def irradiance_traced(self, positions, normals, n_u=16, n_v=16, offset=1e-4, occlude_by_meshes=True, min_transmittance=0.01):
        """E(p, n) traced at the points: (n, 4) = rgb irradiance, fraction of rays no mesh blocks"""
        p, n, d = self._irradiance_args(positions, normals, n_u, n_v, offset, occlude_by_meshes, min_transmittance)
        out = np.zeros((p.shape[0], 4), np.float32)
        self._check(self.L.ngp_irradiance_traced(self.h, p.shape[0], _p(p), _p(n), C.byref(d), _p(out)))
        return out

    # ---------------------------------------------------------------- SH9 irradiance volumes (contract: include/ngp_hip.h)
    @staticmethod
    def _sh_desc(n_u, n_v, occlude_by_meshes, min_transmittance):
        d = IrradianceShDesc()
        d.n_u, d.n_v, d.min_transmittance, d.occlude_by_meshes = n_u, n_v, min_transmittance, int(bool(occlude_by_meshes))
        return d

    @staticmethod
    def _volume_desc(resolution, aabb, sh):
        d = IrradianceVolumeDesc()
        for i in range(3):
            d.res[i], d.aabb_min[i], d.aabb_max[i] = resolution[i], aabb[0][i], aabb[1][i]
        d.sh = sh
        return d

    def irradiance_sphere_rays(self, positions, n_u=32, n_v=32, occlude_by_meshes=True, min_transmittance=0.01):
        """the sphere rays of the probes at `positions`: (origins (n, K, 3), directions (n, K, 3), t_max (n, K)), K = n_u n_v, k = u + n_u v"""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        d = self._sh_desc(n_u, n_v, occlude_by_meshes, min_transmittance)
        k = int(n_u) * int(n_v)
        o = np.zeros((p.shape[0], k, 3), np.float32)
        dr = np.zeros((p.shape[0], k, 3), np.float32)
        t = np.zeros((p.shape[0], k), np.float32)
        self._check(self.L.ngp_irradiance_sphere_rays(self.h, p.shape[0], _p(p), C.byref(d), _p(o), _p(dr), _p(t)))
        return o, dr, t

    def irradiance_sh_traced(self, positions, n_u=32, n_v=32, occlude_by_meshes=True, min_transmittance=0.01, return_rays=False):
        """SH9 probe records traced at `positions`: (n, 28); with return_rays also every ray's rgba as traced, (n, K, 4)"""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        d = self._sh_desc(n_u, n_v, occlude_by_meshes, min_transmittance)
        sh = np.zeros((p.shape[0], 28), np.float32)
        rays = np.zeros((p.shape[0], int(n_u) * int(n_v), 4), np.float32) if return_rays else None
        self._check(self.L.ngp_irradiance_sh_traced(self.h, p.shape[0], _p(p), C.byref(d), _p(sh), _p(rays) if return_rays else None))
        return (sh, rays) if return_rays else sh

    def compute_irradiance_volume(self, resolution, aabb, n_u=32, n_v=32, occlude_by_meshes=True, min_transmittance=0.01, bounces=0, albedo=None, visibility=None,
                                  sun=None, sun_nerf_shadow=None):
        """trace a lattice of resolution = (rx, ry, rz) probes over aabb = (min, max); the volume stays on the device (get_irradiance_volume).
        bounces > 0: that many passes of diffuse interreflection off the meshes, of colour albedo (three channels in [0, 1], or one number for
        all three; None: the default base colour 0.8 squared, in float32); visibility: None, or the keywords of compute_irradiance_volume_visibility
        as a dict: the distance maps are computed first, the bounces look the volume up through them, and they stay in the context.
        sun: None, or the sun whose first bounce off the meshes joins the records ahead of the passes (also with bounces = 0): a dict with
        direction and optionally radiance (default: the frames' sun colour) and shadow_bias (1e-3), or a tuple in that order.
        sun_nerf_shadow: None, or the NeRF's density in front of that sun: True (min_transmittance 0.01, t_min 0), or a dict or a tuple of
        min_transmittance and t_min (without a sun no pass runs)"""
        d = self._volume_desc(resolution, aabb, self._sh_desc(n_u, n_v, occlude_by_meshes, min_transmittance))
        ns = self._sun_nerf_desc(sun_nerf_shadow)
        if sun is not None or ns is not None:
            b = self._bounce_desc(bounces, np.float32(0.8) * np.float32(0.8) if albedo is None else albedo)
            v = None if visibility is None else self._visibility_desc(**dict(dict(n_u=16, n_v=16, sharpness_log2=5, max_distance=0.0, normal_bias=0.0), **visibility))
            s = None if sun is None else self._sun_desc(sun)
            if ns is not None:
                self._check(self.L.ngp_compute_irradiance_volume_sunlit_shadowed(self.h, C.byref(d), C.byref(b), C.byref(v) if v is not None else None,
                                                                                 C.byref(s) if s is not None else None, C.byref(ns)))
                return
            self._check(self.L.ngp_compute_irradiance_volume_sunlit(self.h, C.byref(d), C.byref(b), C.byref(v) if v is not None else None, C.byref(s)))
            return
        if not bounces:
            if albedo is not None or visibility is not None:
                raise ValueError("albedo and visibility belong to bounces > 0")
            self._check(self.L.ngp_compute_irradiance_volume(self.h, C.byref(d)))
            return
        b = self._bounce_desc(bounces, np.float32(0.8) * np.float32(0.8) if albedo is None else albedo)
        v = None if visibility is None else self._visibility_desc(**dict(dict(n_u=16, n_v=16, sharpness_log2=5, max_distance=0.0, normal_bias=0.0), **visibility))
        self._check(self.L.ngp_compute_irradiance_volume_bounced(self.h, C.byref(d), C.byref(b), C.byref(v) if v is not None else None))

    @staticmethod
    def _bounce_desc(bounces, albedo):
        b = IrradianceBounceDesc()
        b.n_bounces = bounces
        b.albedo[:] = [float(x) for x in np.broadcast_to(np.asarray(albedo, np.float32), (3,))]
        return b

    @staticmethod
    def _sun_desc(sun):
        if isinstance(sun, IrradianceSunDesc):
            return sun
        if isinstance(sun, dict):
            extra = set(sun) - {"direction", "radiance", "shadow_bias"}
            if extra or "direction" not in sun:
                raise ValueError("sun: direction, and optionally radiance and shadow_bias")
            sun = (sun["direction"], sun.get("radiance", SUN_RADIANCE), sun.get("shadow_bias", 1e-3))
        sun = tuple(sun)
        if not 1 <= len(sun) <= 3 or np.ndim(sun[0]) != 1:
            raise ValueError("sun: (direction, radiance, shadow_bias)")
        sun = sun + (SUN_RADIANCE, 1e-3)[len(sun) - 1:]
        s = IrradianceSunDesc()
        s.direction[:] = [float(x) for x in np.asarray(sun[0], np.float32).reshape(3)]
        s.radiance[:] = [float(x) for x in np.broadcast_to(np.asarray(sun[1], np.float32), (3,))]
        s.shadow_bias = float(sun[2])
        return s

    @staticmethod
    def _sun_nerf_desc(shadow):
        """None and False: none; True: the defaults; a dict or a tuple of min_transmittance and t_min"""
        if shadow is None or shadow is False:
            return None
        if isinstance(shadow, IrradianceSunNerfDesc):
            return shadow
        if shadow is True:
            shadow = {}
        if isinstance(shadow, dict):
            if set(shadow) - {"min_transmittance", "t_min"}:
                raise ValueError("sun_nerf_shadow: min_transmittance and t_min")
            shadow = (shadow.get("min_transmittance", 0.01), shadow.get("t_min", 0.0))
        shadow = tuple(shadow)
        if not 1 <= len(shadow) <= 2:
            raise ValueError("sun_nerf_shadow: (min_transmittance, t_min)")
        shadow = shadow + (0.0,)[len(shadow) - 1:]
        ns = IrradianceSunNerfDesc()
        ns.min_transmittance, ns.t_min = float(shadow[0]), float(shadow[1])
        return ns

    def irradiance_sh_sun(self, positions, sun, albedo, n_u=32, n_v=32, alpha=None, occlude_by_meshes=True, return_rays=False, nerf_shadow=None, return_shadow=False):
        """one sun pass at the probes at `positions` (no model, no volume): the records R_sun (n, 28) of the sun's first bounce off the meshes,
        float 27 the unblocked fraction; with return_rays also every ray's (B rgb, t of the primary hit or inf), (n, K, 4). sun: as
        compute_irradiance_volume takes it; alpha: None or the rays' NeRF alpha (n, K). nerf_shadow: as compute_irradiance_volume's
        sun_nerf_shadow; the pass then needs a model, the rays are B', and return_shadow adds every ray's (q xyz, alpha_s), (n, K, 4), zeros
        where there is no shadow ray. The results come in the order records, rays, shadow."""
        ns = self._sun_nerf_desc(nerf_shadow)
        if return_shadow and ns is None:
            raise ValueError("return_shadow belongs to nerf_shadow")
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        k = int(n_u) * int(n_v)
        d = self._sh_desc(n_u, n_v, occlude_by_meshes, 0.01)
        s = self._sun_desc(sun)
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(albedo, np.float32), (3,)))
        a = None if alpha is None else np.ascontiguousarray(alpha, np.float32)
        if a is not None and a.size != p.shape[0] * k:
            raise ValueError("alpha: n x K values")
        sh = np.zeros((p.shape[0], 28), np.float32)
        rays = np.zeros((p.shape[0], k, 4), np.float32) if return_rays else None
        if ns is not None:
            shadow = np.zeros((p.shape[0], k, 4), np.float32) if return_shadow else None
            self._check(self.L.ngp_irradiance_sh_sun_shadowed(self.h, p.shape[0], _p(p), C.byref(d), C.byref(s), _p(al), _p(a) if a is not None else None, C.byref(ns),
                                                              _p(rays) if return_rays else None, _p(shadow) if return_shadow else None, _p(sh)))
            out = (sh,) + ((rays,) if return_rays else ()) + ((shadow,) if return_shadow else ())
            return out if len(out) > 1 else sh
        self._check(self.L.ngp_irradiance_sh_sun(self.h, p.shape[0], _p(p), C.byref(d), C.byref(s), _p(al), _p(a) if a is not None else None, _p(sh),
                                                 _p(rays) if return_rays else None))
        return (sh, rays) if return_rays else sh

    def irradiance_sun_ms(self):
        """device time of the last sun pass (compute_irradiance_volume with a sun, irradiance_sh_sun), ms"""
        ms = C.c_float(0)
        self._check(self.L.ngp_get_irradiance_sun_ms(self.h, C.byref(ms)))
        return ms.value

    def irradiance_sun_shadow_ms(self):
        """device time of the shadow rays' prep and trace in the last sun pass, ms; 0 after a pass without a NeRF shadow"""
        ms = C.c_float(0)
        self._check(self.L.ngp_get_irradiance_sun_shadow_ms(self.h, C.byref(ms)))
        return ms.value

    def _frame_record(self, fn, n_pixels, stride):
        """(n_pixels, stride): the record an optional pass of the last frame left, through its getter fn"""
        out = np.zeros((int(n_pixels), stride), np.float32)
        self._check(fn(self.h, _p(out), int(n_pixels)))
        return out

    def _frame_pass_ms(self, fn):
        """device time of an optional pass in the last frame's last sample, ms, through its getter fn"""
        ms = C.c_float(0)
        self._check(fn(self.h, C.byref(ms)))
        return ms.value

    @staticmethod
    def _option_desc(name, value, check=None):
        """the descriptor of the frame option `name` (FRAME_OPTIONS) from what its setter takes: None for None and False, the defaults for
        True, a dict over the defaults; check (optional) sees the values before they are converted"""
        struct, defaults = FRAME_OPTIONS[name]
        if value is None or value is False:
            return None
        if value is True:
            value = {}
        if not isinstance(value, dict) or set(value) - set(defaults):
            keys = list(defaults)
            raise ValueError("%s: True, False, None or a dict of %s and %s" % (name, ", ".join(keys[:-1]), keys[-1]))
        values = dict(defaults, **value)
        if check is not None:
            check(values)
        d = struct()
        for k, v in values.items():
            setattr(d, k, type(defaults[k])(v))
        return d

    def _set_option(self, name, d):
        self._check(getattr(self.L, "ngp_set_" + name)(self.h, C.byref(d) if d is not None else None))

    def _option_dict(self, name):
        """None while the frame option `name` is off, else its descriptor as set, a dict in the fields' order"""
        struct, defaults = FRAME_OPTIONS[name]
        d, on = struct(), C.c_int(0)
        self._check(getattr(self.L, "ngp_get_" + name)(self.h, C.byref(d), C.byref(on)))
        return {k: getattr(d, k) for k in defaults} if on.value else None

    def set_sun_nerf_shadow(self, shadow=True):
        """the NeRF's density in front of the frames' sun on mesh pixels (Geometry frames with meshes and a model): None or False switches it
        off (the default), True takes min_transmittance 0.01 and t_min 0, a dict or a tuple gives min_transmittance and t_min"""
        self._set_option("sun_nerf_shadow", self._sun_nerf_desc(shadow))

    def sun_nerf_shadow(self):
        """None while the option is off, else dict(min_transmittance=, t_min=) as set"""
        return self._option_dict("sun_nerf_shadow")

    def frame_sun_shadow(self, n_pixels):
        """(n_pixels, 4): per pixel of the last frame's last sample, in the frame's pixel order, (q xyz, alpha_s) of its shadow ray through the
        NeRF; zeros where the pixel had none. On a multi-device context the primary's tile-packed share."""
        return self._frame_record(self.L.ngp_get_frame_sun_shadow, n_pixels, 4)

    def frame_sun_shadow_ms(self):
        """device time of the shadow rays' prep and trace in the last frame's last sample, ms; 0 after a frame without them"""
        return self._frame_pass_ms(self.L.ngp_get_frame_sun_shadow_ms)

    def set_mesh_shadow_on_nerf(self, shadow=True):
        """the meshes in front of the sun on the NeRF (Geometry frames with meshes and a model, the four shade modes): None or False switches
        it off (the default), True takes strength 0.5 and bias 1e-2, a dict gives strength and bias"""
        self._set_option("mesh_shadow_on_nerf", self._option_desc("mesh_shadow_on_nerf", shadow))

    def mesh_shadow_on_nerf(self):
        """None while the option is off, else dict(strength=, bias=) as set"""
        return self._option_dict("mesh_shadow_on_nerf")

    def frame_mesh_shadow(self, n_pixels):
        """(n_pixels, 4): per pixel of the last frame's last sample, in the frame's pixel order, (p xyz, 2 blocked / 1 open) of the NeRF's
        surface point under the meshes' shadow; zeros where the pixel owns none. On a multi-device context the primary's tile-packed share."""
        return self._frame_record(self.L.ngp_get_frame_mesh_shadow, n_pixels, 4)

    def frame_mesh_shadow_ms(self):
        """device time of the mesh shadow kernel in the last frame's last sample, ms; 0 after a frame without it"""
        return self._frame_pass_ms(self.L.ngp_get_frame_mesh_shadow_ms)

    # ---------------------------------------------------------------- the meshes' change of the ambient light on the NeRF (include/ngp_hip.h, "ambient")
    def set_ambient_change_on_nerf(self, change=True):
        """scale every NeRF pixel that owns a surface point by E_after / E_before there (Geometry frames with meshes and a model, the four
        shade modes; needs the irradiance volume and the reference volume): None or False switches it off (the default), True takes
        min_irradiance 1e-3 and max_gain 4, a dict gives them"""
        self._set_option("ambient_change_on_nerf", self._option_desc("ambient_change_on_nerf", change))

    def ambient_change_on_nerf(self):
        """None while the option is off, else dict(min_irradiance=, max_gain=) as set"""
        return self._option_dict("ambient_change_on_nerf")

    def compute_reference_irradiance_volume(self, resolution, aabb, n_u=32, n_v=32, min_transmittance=0.01):
        """trace the reference volume, the scene before the meshes: V_0 over the lattice with the meshes occluding nothing, no bounces, no
        sun; it stays on the device (reference_irradiance_volume) and the context's own volume is untouched"""
        d = self._volume_desc(resolution, aabb, self._sh_desc(n_u, n_v, False, min_transmittance))
        self._check(self.L.ngp_compute_reference_irradiance_volume(self.h, C.byref(d)))

    def set_reference_irradiance_volume(self, sh, aabb, n_u=0, n_v=0, min_transmittance=0.01):
        """a caller's own reference records (rz, ry, rx, 28) over aabb = (min, max)"""
        sh = np.ascontiguousarray(sh, np.float32)
        if sh.ndim != 4 or sh.shape[3] != 28:
            raise ValueError("records: (rz, ry, rx, 28)")
        d = self._volume_desc(sh.shape[2::-1], aabb, self._sh_desc(n_u, n_v, False, min_transmittance))
        self._check(self.L.ngp_set_reference_irradiance_volume(self.h, C.byref(d), _p(sh)))

    def reference_irradiance_volume(self):
        """(desc, records (rz, ry, rx, 28)) of the reference volume"""
        d = IrradianceVolumeDesc()
        self._check(self.L.ngp_get_reference_irradiance_volume(self.h, C.byref(d), None))
        sh = np.zeros((d.res[2], d.res[1], d.res[0], 28), np.float32)
        self._check(self.L.ngp_get_reference_irradiance_volume(self.h, C.byref(d), _p(sh)))
        return d, sh

    def clear_reference_irradiance_volume(self):
        self._check(self.L.ngp_clear_reference_irradiance_volume(self.h))

    def irradiance_volume_ratio(self, positions, normals, min_irradiance=1e-3, max_gain=4.0):
        """(n, 4) = g rgb, state (1 no estimate, 2 scaled): E_after / E_before per channel, the context's volume over its reference volume"""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if p.shape != n.shape:
            raise ValueError("positions and normals: n x 3 each")
        d = self._option_desc("ambient_change_on_nerf", dict(min_irradiance=min_irradiance, max_gain=max_gain))
        out = np.zeros((p.shape[0], 4), np.float32)
        self._check(self.L.ngp_irradiance_volume_ratio(self.h, p.shape[0], _p(p), _p(n), C.byref(d), _p(out)))
        return out

    def frame_ambient_change(self, n_pixels):
        """(n_pixels, 12): per pixel of the last frame's last sample, in the frame's pixel order: p (3), state (0 not an owner, 1 no estimate,
        2 scaled), N (3), W_after, g (3), W_before. On a multi-device context the primary's tile-packed share."""
        return self._frame_record(self.L.ngp_get_frame_ambient_change, n_pixels, 12)

    def frame_ambient_change_ms(self):
        """device time of the normals and ratio kernels in the last frame's last sample, ms; 0 after a frame without them"""
        return self._frame_pass_ms(self.L.ngp_get_frame_ambient_change_ms)

    # ---------------------------------------------------------------- the NeRF mirrored in the meshes (include/ngp_hip.h, "mesh reflection")
    def set_mesh_reflection(self, reflection=True):
        """one reflection ray a mesh pixel through the NeRF (Geometry frames with meshes and a model, the four shade modes): None or False
        switches it off (the default), True takes strength 1, min_transmittance 0.01 and t_min 0, a dict gives them"""
        self._set_option("mesh_reflection", self._option_desc("mesh_reflection", reflection))

    def mesh_reflection(self):
        """None while the option is off, else dict(strength=, min_transmittance=, t_min=) as set"""
        return self._option_dict("mesh_reflection")

    def frame_mesh_reflection(self, n_pixels):
        """(n_pixels, 12): per pixel of the last frame's last sample, in the frame's pixel order: q (3), t_hit, r (3) before the tracer
        normalises it, 0, rgb_r (3), alpha_r; zeros where the pixel owns no ray. On a multi-device context the primary's tile-packed share."""
        return self._frame_record(self.L.ngp_get_frame_mesh_reflection, n_pixels, 12)

    def frame_mesh_reflection_ms(self):
        """device time of the reflection rays' prep and trace in the last frame's last sample, ms; 0 after a frame without them"""
        return self._frame_pass_ms(self.L.ngp_get_frame_mesh_reflection_ms)

    def set_mesh_reflection_meshes(self, on=True):
        """with set_mesh_reflection on: a mirror ray that a mesh cuts has its hit shaded by the mesh pass's own shade, composited behind the
        NeRF along the ray (off by default)"""
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError("mesh_reflection_meshes: True or False")
        self._check(self.L.ngp_set_mesh_reflection_meshes(self.h, 1 if on else 0))

    def mesh_reflection_meshes(self):
        on = C.c_int(0)
        self._check(self.L.ngp_get_mesh_reflection_meshes(self.h, C.byref(on)))
        return bool(on.value)

    def frame_mesh_reflection_hits(self, n_pixels):
        """(n_pixels, 8): per pixel of the last frame's last sample, in the frame's pixel order: p2 (3), shadow2, C2 (3), 1; zeros where the
        pixel's mirror ray is not cut by a mesh. On a multi-device context the primary's tile-packed share."""
        return self._frame_record(self.L.ngp_get_frame_mesh_reflection_hits, n_pixels, 8)

    def frame_mesh_reflection_hits_ms(self):
        """device time of the hit-shade kernel in the last frame's last sample, ms; 0 after a frame without it"""
        return self._frame_pass_ms(self.L.ngp_get_frame_mesh_reflection_hits_ms)

    def set_sun_disk(self, disk=True):
        """the sun's disk (Geometry frames with meshes): K shadow rays a pixel over the disk against all meshes, on mesh pixels and, with
        set_mesh_shadow_on_nerf, on NeRF pixels. None or False switches it off (the default), True takes the real sun's 0.00465 rad and 16
        rays, a dict gives angular_radius and n_rays (1, 2, 4, 8 or 16)"""
        def whole_n_rays(values):  # (before int() would round it or the struct's uint32 wrap it)
            if int(values["n_rays"]) != values["n_rays"] or not 0 <= values["n_rays"] < 2 ** 32:
                raise ValueError("sun_disk: n_rays must be 1, 2, 4, 8 or 16")

        self._set_option("sun_disk", self._option_desc("sun_disk", disk, whole_n_rays))

    def sun_disk(self):
        """None while the option is off, else dict(angular_radius=, n_rays=) as set"""
        return self._option_dict("sun_disk")

    def sun_disk_directions(self, sun_dir, spp_index=0):
        """(n_rays, 3) float32: the shadow directions the frame's sample of spp index `spp_index` uses under sun_dir (host arithmetic)"""
        on = self.sun_disk()
        if on is None:
            raise RuntimeError("the sun has no disk: call set_sun_disk first")
        sd = np.ascontiguousarray(sun_dir, np.float32).reshape(3)
        out = np.zeros((on["n_rays"], 3), np.float32)
        self._check(self.L.ngp_sun_disk_directions(self.h, _p(sd), int(spp_index), _p(out)))
        return out

    def frame_sun_disk(self, n_pixels):
        """(n_pixels, 4): per pixel of the last frame's last sample, in the frame's pixel order, (q xyz, 1 + the blocked rays' count) of the
        mesh pixel's disk; zeros where the pixel owns none. On a multi-device context the primary's tile-packed share."""
        return self._frame_record(self.L.ngp_get_frame_sun_disk, n_pixels, 4)

    def frame_sun_disk_ms(self):
        """device time of the sun disk kernel in the last frame's last sample, ms; refused after a frame without it"""
        return self._frame_pass_ms(self.L.ngp_get_frame_sun_disk_ms)

    def irradiance_sh_bounce(self, positions, albedo, n_u=32, n_v=32, alpha=None, visible=False, occlude_by_meshes=True, return_rays=False):
        """one bounce pass at the probes at `positions` from the held volume (visible: through its visible lookup): the records R (n, 28) the pass
        adds, float 27 the unblocked fraction; with return_rays also every ray's (B rgb, t of the hit or inf), (n, K, 4). alpha: None or the
        rays' NeRF alpha (n, K)"""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        k = int(n_u) * int(n_v)
        d = self._sh_desc(n_u, n_v, occlude_by_meshes, 0.01)
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(albedo, np.float32), (3,)))
        a = None if alpha is None else np.ascontiguousarray(alpha, np.float32)
        if a is not None and a.size != p.shape[0] * k:
            raise ValueError("alpha: n x K values")
        sh = np.zeros((p.shape[0], 28), np.float32)
        rays = np.zeros((p.shape[0], k, 4), np.float32) if return_rays else None
        self._check(self.L.ngp_irradiance_sh_bounce(self.h, p.shape[0], _p(p), C.byref(d), _p(al), _p(a) if a is not None else None, int(bool(visible)), _p(sh),
                                                    _p(rays) if return_rays else None))
        return (sh, rays) if return_rays else sh

    def irradiance_bounce_ms(self):
        """device time of the last bounce pass (compute_irradiance_volume with bounces, irradiance_sh_bounce), ms"""
        ms = C.c_float(0)
        self._check(self.L.ngp_get_irradiance_bounce_ms(self.h, C.byref(ms)))
        return ms.value

    def get_irradiance_volume(self):
        """(desc, records (rz, ry, rx, 28))"""
        d = IrradianceVolumeDesc()
        self._check(self.L.ngp_get_irradiance_volume(self.h, C.byref(d), None))
        sh = np.zeros((d.res[2], d.res[1], d.res[0], 28), np.float32)
        self._check(self.L.ngp_get_irradiance_volume(self.h, C.byref(d), _p(sh)))
        return d, sh

    def set_irradiance_volume(self, sh, aabb, n_u=0, n_v=0, occlude_by_meshes=True, min_transmittance=0.01):
        """a caller's own records (rz, ry, rx, 28) over aabb = (min, max); n_u ... only describe how they were made"""
        sh = np.ascontiguousarray(sh, np.float32)
        if sh.ndim != 4 or sh.shape[3] != 28:
            raise ValueError("records: (rz, ry, rx, 28)")
        d = self._volume_desc(sh.shape[2::-1], aabb, self._sh_desc(n_u, n_v, occlude_by_meshes, min_transmittance))
        self._check(self.L.ngp_set_irradiance_volume(self.h, C.byref(d), _p(sh)))

    def clear_irradiance_volume(self):
        self._check(self.L.ngp_clear_irradiance_volume(self.h))

    def irradiance_volume_at(self, positions, normals, visible=False):
        """E(p, n) read from the volume: (n, 4) = rgb irradiance, weight of the live probes around the point; visible: every probe weighted
        by its visibility from the point (needs compute_irradiance_volume_visibility or set_irradiance_volume_visibility)"""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if p.shape != n.shape:
            raise ValueError("positions and normals: n x 3 each")
        out = np.zeros((p.shape[0], 4), np.float32)
        f = self.L.ngp_irradiance_volume_at_visible if visible else self.L.ngp_irradiance_volume_at
        self._check(f(self.h, p.shape[0], _p(p), _p(n), _p(out)))
        return out

    # ---------------------------------------------------------------- probe visibility (contract: include/ngp_hip.h)
    @staticmethod
    def _visibility_desc(n_u, n_v, sharpness_log2, max_distance, normal_bias):
        d = IrradianceVisibilityDesc()
        d.n_u, d.n_v, d.sharpness_log2, d.max_distance, d.normal_bias = n_u, n_v, sharpness_log2, max_distance, normal_bias
        return d

    def irradiance_distance_maps(self, positions, n_u=16, n_v=16, sharpness_log2=5, max_distance=1.0):
        """the distance maps of probes at `positions`: (n, 64, 2) = mean and mean squared distance to the nearest mesh per octahedral texel"""
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        d = self._visibility_desc(n_u, n_v, sharpness_log2, max_distance, 0.0)
        maps = np.zeros((p.shape[0], 64, 2), np.float32)
        self._check(self.L.ngp_irradiance_distance_maps(self.h, p.shape[0], _p(p), C.byref(d), _p(maps)))
        return maps

    def compute_irradiance_volume_visibility(self, n_u=16, n_v=16, sharpness_log2=5, max_distance=0.0, normal_bias=0.0):
        """distance maps for the probes of the held volume; they stay on the device (get_irradiance_volume_visibility). max_distance <= 0:
        1.5 x the diagonal of a lattice cell"""
        d = self._visibility_desc(n_u, n_v, sharpness_log2, max_distance, normal_bias)
        self._check(self.L.ngp_compute_irradiance_volume_visibility(self.h, C.byref(d)))

    def get_irradiance_volume_visibility(self):
        """(desc, maps (rz, ry, rx, 64, 2)); desc.max_distance is the D in use"""
        v = IrradianceVolumeDesc()
        self._check(self.L.ngp_get_irradiance_volume(self.h, C.byref(v), None))
        d = IrradianceVisibilityDesc()
        maps = np.zeros((v.res[2], v.res[1], v.res[0], 64, 2), np.float32)
        self._check(self.L.ngp_get_irradiance_volume_visibility(self.h, C.byref(d), _p(maps)))
        return d, maps

    def set_irradiance_volume_visibility(self, maps, max_distance, sharpness_log2=5, normal_bias=0.0, n_u=0, n_v=0):
        """a caller's own maps (rz, ry, rx, 64, 2) for the held volume's probes; n_u, n_v only describe how they were made"""
        maps = np.ascontiguousarray(maps, np.float32)
        if maps.ndim != 5 or maps.shape[3:] != (64, 2):
            raise ValueError("maps: (rz, ry, rx, 64, 2)")
        v = IrradianceVolumeDesc()
        self._check(self.L.ngp_get_irradiance_volume(self.h, C.byref(v), None))
        if maps.shape[:3] != (v.res[2], v.res[1], v.res[0]):
            raise ValueError("maps: the held volume has (rz, ry, rx) = (%d, %d, %d)" % (v.res[2], v.res[1], v.res[0]))
        d = self._visibility_desc(n_u, n_v, sharpness_log2, max_distance, normal_bias)
        self._check(self.L.ngp_set_irradiance_volume_visibility(self.h, C.byref(d), _p(maps)))

    def clear_irradiance_volume_visibility(self):
        self._check(self.L.ngp_clear_irradiance_volume_visibility(self.h))

    # ---------------------------------------------------------------- stages
    def grid_encode(self, pos01):
        pos01 = np.ascontiguousarray(pos01, np.float32)
        d = self.get_model()  # a Frequency position encoding (pos_encoding 1) is as wide as its padded 3 * 2 * n_frequencies
        al = d.mlp_alignment or 16
        width = (6 * d.pos_n_frequencies + al - 1) // al * al if d.pos_encoding == 1 else (3 + al - 1) // al * al if d.pos_encoding == 2 else 32
        out = np.zeros((pos01.shape[0], width), np.uint16)
        self._check(self.L.ngp_grid_encode(self.h, pos01.shape[0], _p(pos01), _p(out)))
        return out.view(np.float16)

    def density_gradient(self, pos01):
        """d density logit / d position (what ERenderMode::Normals composites): n x 3 floats"""
        pos01 = np.ascontiguousarray(pos01, np.float32)
        out = np.zeros((pos01.shape[0], 3), np.float32)
        self._check(self.L.ngp_density_gradient(self.h, pos01.shape[0], _p(pos01), _p(out)))
        return out

    def network(self, pos01, dir01):
        pos01 = np.ascontiguousarray(pos01, np.float32)
        dir01 = np.ascontiguousarray(dir01, np.float32)
        out = np.zeros((pos01.shape[0], 4), np.uint16)
        self._check(self.L.ngp_network_inference(self.h, pos01.shape[0], _p(pos01), _p(dir01), _p(out)))
        return out.view(np.float16)

    # ---- marching cubes (contract: include/ngp_hip.h). res: one int or three; aabb: None (the render aabb) or (min3, max3) in ngp space
    @staticmethod
    def _mc_args(res, aabb):
        r = np.asarray([res] * 3 if np.isscalar(res) else res, np.uint32)
        if r.shape != (3,):
            raise ValueError("resolution: one value or three")
        a = None if aabb is None else np.ascontiguousarray(np.asarray(aabb, np.float32).reshape(6))
        return r, a

    def density_on_grid(self, res, aabb=None):
        """the activated density on the lattice: float32 (rz, ry, rx)"""
        r, a = self._mc_args(res, aabb)
        out = np.zeros((int(r[2]), int(r[1]), int(r[0])), np.float32)
        self._check(self.L.ngp_density_on_grid(self.h, _p(r), _p(a) if a is not None else None, _p(out)))
        return out

    def _mc_mesh(self, nv, nt, attrs):
        V = np.zeros((nv, 3), np.float32)
        F = np.zeros((nt, 3), np.uint32)
        N = np.zeros((nv, 3), np.float32) if attrs else None
        Cc = np.zeros((nv, 3), np.float32) if attrs else None
        self._check(self.L.ngp_get_marching_cubes_mesh(self.h, _p(V), _p(N) if attrs else None, _p(Cc) if attrs else None, _p(F)))
        return {"V": V, "N": N, "C": Cc, "F": F}

    def marching_cubes(self, density, thresh, aabb=None):
        """marching cubes on a caller's lattice (float32 (rz, ry, rx)): {"V", "F"} in ngp space"""
        d = np.ascontiguousarray(density, np.float32)
        r, a = self._mc_args(d.shape[::-1], aabb)
        nv, nt = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.ngp_marching_cubes(self.h, _p(r), _p(a) if a is not None else None, float(thresh), _p(d), C.addressof(nv), C.addressof(nt)))
        m = self._mc_mesh(nv.value, nt.value, False)
        return {"V": m["V"], "F": m["F"]}

    def compute_marching_cubes_mesh(self, res=256, aabb=None, thresh=2.5):
        """lattice + marching cubes + normals + colours: {"V", "N", "C", "F"} in ngp space"""
        r, a = self._mc_args(res, aabb)
        nv, nt = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.ngp_compute_marching_cubes_mesh(self.h, _p(r), _p(a) if a is not None else None, float(thresh), C.addressof(nv), C.addressof(nt)))
        return self._mc_mesh(nv.value, nt.value, True)

    def save_marching_cubes_mesh(self, path):
        self._check(self.L.ngp_save_marching_cubes_mesh(self.h, os.fsencode(path)))

    def marching_cubes_timings(self):
        """device ms of the last compute_marching_cubes_mesh: lattice, marching cubes, normals + colours"""
        ms = np.zeros(3, np.float32)
        self._check(self.L.ngp_get_marching_cubes_timings(self.h, _p(ms)))
        return [float(x) for x in ms]

    def density_bitfield(self):
        bf = np.zeros(128 ** 3 // 8 * 8, np.uint8)
        mean = C.c_float(0)
        self._check(self.L.ngp_get_density_bitfield(self.h, _p(bf), C.addressof(mean)))
        return bf, mean.value

    def set_render_aabb(self, lo, hi, to_local=None):
        lo = np.asarray(lo, np.float32); hi = np.asarray(hi, np.float32)
        r = None if to_local is None else np.ascontiguousarray(np.asarray(to_local, np.float32).T.reshape(-1))  # column-major
        self._check(self.L.ngp_set_render_aabb(self.h, _p(lo), _p(hi), _p(r) if r is not None else None))

    def set_envmap(self, rgba=None):
        """(H, W, 4) lat-long radiance behind the NeRF (m_envmap); None removes it"""
        if rgba is None:
            self._check(self.L.ngp_set_envmap(self.h, 0, 0, None))
            return
        env = np.ascontiguousarray(rgba, np.float32)
        self._check(self.L.ngp_set_envmap(self.h, env.shape[1], env.shape[0], _p(env)))

    def set_cone_angle_constant(self, value):
        self._check(self.L.ngp_set_cone_angle_constant(self.h, value))

    def update_density_grid(self, decay=0.95, n_uniform=0, n_nonuniform=0, n_iterations=1):
        """Testbed::update_density_grid_nerf: refresh the occupancy grid from the density network (0/0 = training_prep_nerf's schedule)."""
        self._check(self.L.ngp_update_density_grid(self.h, decay, n_uniform, n_nonuniform, n_iterations))

    def density_grid(self, max_cascade):
        out = np.zeros(128 ** 3 * (max_cascade + 1), np.float32)
        self._check(self.L.ngp_get_density_grid(self.h, _p(out), out.size))
        return out

    def init_rays(self, cam):
        pl = np.zeros(cam.width * cam.height, PAYLOAD_DTYPE)
        self._check(self.L.ngp_init_rays(self.h, C.byref(cam), _p(pl)))
        return pl

    # ------------------------------------------------------------- training
    def reset_network(self, log2_hashmap_size=19, seed=1337):
        self._check(self.L.ngp_reset_network(self.h, log2_hashmap_size, seed))

    def training_opts(self):
        o = TrainingOpts()
        self._check(self.L.ngp_get_training_opts(self.h, C.byref(o)))
        return o

    def set_training_opts(self, **kw):
        o = self.training_opts()
        for k, v in kw.items():
            if k == "background_color":
                o.background_color = (C.c_float * 3)(*v)
            elif k == "loss_type" and isinstance(v, str):
                o.loss_type = LOSS_TYPES[v]
            else:
                if not hasattr(o, k):
                    raise AttributeError(k)
                setattr(o, k, v)
        self._check(self.L.ngp_set_training_opts(self.h, C.byref(o)))

    def set_training_image(self, view, img):
        """img: (H, W, 4) uint8 (sRGB, straight alpha) or float32 (linear, premultiplied)."""
        if img.dtype == np.uint8:
            a, t = np.ascontiguousarray(img), IMAGE_BYTE
        else:
            a, t = np.ascontiguousarray(img, np.float32), IMAGE_FLOAT
        assert a.ndim == 3 and a.shape[2] == 4
        self._check(self.L.ngp_set_training_image(self.h, view, a.shape[1], a.shape[0], _p(a), t))

    def load_training_images(self):
        n = C.c_int32(0)
        self._check(self.L.ngp_load_training_images(self.h, C.byref(n)))
        return n.value

    def render_ground_truth(self, view, width, height, background=(0.0, 0.0, 0.0, 1.0), exposure=0.0, color_space=1, to_srgb=False, fov_axis=1, zoom=1.0):
        bg = np.asarray(background, np.float32)
        out = np.zeros((height, width, 4), np.float32)
        self._check(self.L.ngp_render_ground_truth(self.h, view, width, height, _p(bg), exposure, color_space, int(to_srgb), fov_axis, zoom, _p(out)))
        return out

    def train(self, n_steps=1, batch_size=1 << 18):
        loss = C.c_float(0)
        self._check(self.L.ngp_train(self.h, n_steps, batch_size, C.byref(loss)))
        return loss.value

    def training_state(self):
        st = TrainingState()
        self._check(self.L.ngp_get_training_state(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in TrainingState._fields_ if k != "struct_size"}

    def train_prepare_batch(self, batch_size):
        n_rays = self.training_state()["rays_per_batch"]
        counters = np.zeros(3, np.uint32)
        ray_indices = np.zeros(n_rays, np.uint32)
        numsteps = np.zeros((n_rays, 2), np.uint32)
        coords = np.zeros((batch_size, 7), np.float32)
        dloss = np.zeros((batch_size, 4), np.float16)
        loss = np.zeros(n_rays, np.float32)
        self._check(self.L.ngp_train_prepare_batch(self.h, batch_size, _p(counters), _p(ray_indices), _p(numsteps), _p(coords), _p(dloss), _p(loss)))
        return {"counters": counters, "ray_indices": ray_indices, "numsteps": numsteps, "coords": coords, "dloss": dloss, "loss": loss, "n_rays": n_rays}

    def train_gradients(self, batch_size):
        n = self.training_state()["n_params"] or self.get_model().n_params
        g = np.zeros(int(n), np.float32)
        self._check(self.L.ngp_train_gradients(self.h, batch_size, _p(g)))
        return g

    def train_apply(self):
        self._check(self.L.ngp_train_apply(self.h))

    def training_params(self):
        n = int(self.get_model().n_params)
        w, e = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self._check(self.L.ngp_get_training_params(self.h, _p(w), _p(e)))
        return w, e
