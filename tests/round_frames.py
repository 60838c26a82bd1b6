"""Child process of tests/test_round_gpu.py: renders the frames of that test with the library NGP_HIP_LIBRARY names and prints one
record per frame: digests of rgba and depth, the four counters and the kernel that ran. Not a test module."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
PKG = "surface-irradiance-estimation-from-neural-radiance-fields_amd"
DEFAULT_SCHEDULE = (64, 4, 32, 1, 1, 4, 1, 1)
EXACT_MARCH = (64, 4, 32, 1, 1, 4, 0, 1)
COUNTERS = ("n_rays", "n_rays_alive_after_init", "n_rays_hit", "n_samples")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    import torch  # torch bundles its own HIP runtime: it has to initialise first

    import model_fixtures

    native, synthetic, scene = (importlib.import_module(PKG + "." + m) for m in ("native", "synthetic", "scene"))
    torch.zeros(1, device="cuda")
    ctx = native.Context(0)
    out = {}

    def frame(name, w, h, az=45.0, el=30.0, radius=4.03, aperture_size=0.0, **opts):
        cam = native.make_camera(scene.orbit_camera(az, el, radius), w, h, scene.focal_from_fov_x(w, 0.6911), aperture_size=aperture_size, focus_z=1.3)
        rgba, depth = ctx.render(cam, native.make_opts(**opts), want_depth=True)
        st = ctx.render_stats()
        out[name] = dict(rgba=sha(rgba), depth=sha(depth), nonzero=int(np.count_nonzero(rgba[..., :3])), kernel=ctx.last_render_kernel(), **{k: int(st[k]) for k in COUNTERS})

    # the frame list of tests/test_netsec_gpu.py: the benchmark's model
    model = synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19)
    ctx.set_model(model)
    for sched_name, sched in (("default", DEFAULT_SCHEDULE), ("exact_march", EXACT_MARCH)):
        ctx.set_schedule(*sched)
        frame(sched_name + "/plain", 320, 180)
        frame(sched_name + "/plain_inside", 256, 144, az=20.0, el=10.0, radius=0.5)
        frame(sched_name + "/depth_of_field", 320, 180, az=200.0, aperture_size=0.05)
        frame(sched_name + "/share8", 320, 180, shard_index=3, shard_count=8)
    ctx.set_schedule(*DEFAULT_SCHEDULE)
    frame("default/1080p", 1920, 1080, az=135.0)
    frame("default/1080p_depth_of_field", 1920, 1080, az=135.0, aperture_size=0.02)
    wide_box = dict(model)
    wide_box["render_aabb"] = ((-0.25, -0.25, -0.25), (1.25, 1.25, 1.25))
    ctx.set_model(wide_box)
    frame("wide_box/plain", 320, 180)
    frame("wide_box/depth_of_field", 320, 180, az=200.0, aperture_size=0.05)

    # the other kernels that read the occupancy summaries
    unit = synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=15)  # conftest.scene_unit
    ctx.set_model(unit)
    frame("kernels/normals", 160, 90, az=70.0, render_mode=native.RENDER_NORMALS)
    rng = np.random.default_rng(12)
    o = rng.normal(size=(4096, 3))
    ray_o = (0.5 + 2.0 * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    d = rng.uniform(0.2, 0.8, (4096, 3)) - ray_o
    ray_d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rgba, depth = ctx.trace_nerf_rays(ray_o, ray_d)  # trace_probe_fused
    out["kernels/probe_rays"] = dict(rgba=sha(rgba), depth=sha(depth), nonzero=int(np.count_nonzero(rgba[..., :3])), kernel="trace_probe_fused")
    big = synthetic.make_scene(aabb_scale=4, seed=99, log2_hashmap_size=16, pls_rule="upstream")  # conftest.scene_big
    ctx.set_model(big)
    frame("kernels/c5_plain", 256, 144)
    frame("kernels/c5", 256, 144, az=200.0, aperture_size=0.05)
    ctx.set_schedule(*EXACT_MARCH)  # the reference's climb through the cascades, one cell at a time
    frame("kernels/c5_plain_exact_march", 256, 144)
    ctx.set_schedule(*DEFAULT_SCHEDULE)
    ctx.set_model(model_fixtures.beyond_the_grid(big))  # 8 cascades, rays that start outside the occupancy grid
    frame("kernels/generic", 256, 144)
    fsc = synthetic.make_scene(aabb_scale=1, seed=7, cfg=scene.frequency_network_config())  # configs/nerf/frequency.json: wide_kernels.hip
    ctx.set_model(fsc)
    frame("kernels/wide", 96, 54)

    # a training occupancy refresh rebuilds the bitfield on the device: the derived tables have to follow it
    ctx.set_model(unit)
    frame("refresh/before", 256, 144)
    ctx.update_density_grid(decay=0.95, n_iterations=3)
    frame("refresh/after", 256, 144)
    frame("refresh/after_inside", 256, 144, az=20.0, el=10.0, radius=0.5)
    ctx.close()
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
