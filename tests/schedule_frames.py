"""Child process of tests/test_schedule_gpu.py: renders every frame of FRAMES under every schedule of SCHEDULES with ONE context and
prints one record per (schedule, frame): digests of rgba and depth, the counters, the kernel that ran, and how many pixels differ from
the same frame under the first schedule of the group (the anchor). Not a test module; run it as `python tests/schedule_frames.py`.

With --env-route the schedule comes from NGP_TUNE (read at context creation) and set_schedule is never called: the frames of ENV_FRAMES
under that one schedule."""
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

# refill_min, skip_steps, go_min, max_stall, k_busy, k_drain, block_jumps, share (include/ngp_hip.h: ngp_set_schedule)
KNOBS = ("refill_min", "skip_steps", "go_min", "max_stall", "k_busy", "k_drain", "block_jumps", "share")
RANGE = ((16, 64), (1, 64), (1, 64), (0, 64), (1, 8), (1, 8), (0, 1), (0, 1))  # validate_schedule (csrc/ngp_render.cpp)
ANCHOR = (64, 1, 1, 0, 1, 1, 1, 0)
DEFAULT = (64, 4, 32, 1, 1, 4, 1, 1)
ALL_LOW = (16, 1, 1, 0, 1, 1, 1, 0)
ALL_HIGH = (64, 64, 64, 64, 8, 8, 1, 1)
MIXED = (16, 64, 64, 0, 8, 1, 1, 1)


def one_knob_schedules():
    """each knob but block_jumps alone at its lowest and its highest allowed value, the others at their defaults: 14 tuples, of which
    refill_min = 64, k_busy = 1 and share = 1 ARE the default schedule"""
    out = []
    for i in (0, 1, 2, 3, 4, 5, 7):
        for v in RANGE[i]:
            out.append(DEFAULT[:i] + (v,) + DEFAULT[i + 1:])
    return out


def _unique(seq):
    return tuple(dict.fromkeys(seq))


def _exact(s):
    return s[:6] + (0,) + s[7:]


# block_jumps changes sample sets, so schedules are compared inside their group only; a group's first schedule is its anchor
SCHEDULES = {
    "jumps": _unique((ANCHOR, DEFAULT) + tuple(one_knob_schedules()) + (ALL_LOW, ALL_HIGH, MIXED)),  # 2 + 14 - 3 duplicates of DEFAULT + 3 = 16
    "exact": tuple(_exact(s) for s in (ANCHOR, DEFAULT, ALL_LOW, ALL_HIGH, MIXED)),
}

UNIT_PLAIN, UNIT = "render_nerf_fused_unit_plain", "render_nerf_fused_unit"
# (model, frame, kernel). Models are set in this order; every frame of a model is rendered under every schedule before the next model.
FRAMES = (
    ("unit", "pinhole", UNIT_PLAIN), ("unit", "inside", UNIT_PLAIN), ("unit", "share8", UNIT_PLAIN), ("unit", "packed", UNIT_PLAIN),
    ("unit", "odd_101x67", UNIT_PLAIN), ("unit", "8x8", UNIT_PLAIN), ("unit", "1x1", UNIT_PLAIN), ("unit", "spp4", UNIT_PLAIN),
    ("unit", "depth_of_field", UNIT), ("unit", "depth_of_field_envmap", UNIT), ("unit", "normals", "render_nerf_fused_normals"),
    ("unit", "hybrid", UNIT_PLAIN), ("unit", "probe_envmap", "trace_probe_fused"), ("unit", "probe_rays", "trace_probe_fused"),
    ("big", "pinhole", "render_nerf_fused_c5_plain"), ("big", "depth_of_field", "render_nerf_fused_c5"),
    ("big_beyond_grid", "pinhole", "render_nerf_fused"),
    ("rgb_1layer", "pinhole", "render_nerf_fused_mid0"), ("rgb_3layer", "pinhole", "render_nerf_fused_mid2"),
    ("rgb_0layer", "pinhole", "render_nerf_fused_lin_rgb"), ("linear", "pinhole", "render_nerf_fused_lin"),
)
ENV_FRAMES = (("unit", "pinhole"), ("unit", "inside"))
PROBE_FRAMES = ("probe_envmap", "probe_rays")  # no camera frame: no render counters, and the kernel is not chosen by launch_render_nerf


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main(env_route):
    import torch  # torch bundles its own HIP runtime: it has to initialise first

    import model_fixtures

    native, synthetic, scene, meshio = (importlib.import_module(PKG + "." + m) for m in ("native", "synthetic", "scene", "meshio"))
    torch.zeros(1, device="cuda")
    ctx = native.Context(0)
    models = {
        "unit": lambda: synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=15),  # conftest.scene_unit
        "big": lambda: synthetic.make_scene(aabb_scale=4, seed=99, log2_hashmap_size=16, pls_rule="upstream"),  # conftest.scene_big
        "big_beyond_grid": lambda: model_fixtures.beyond_the_grid(synthetic.make_scene(aabb_scale=4, seed=99, log2_hashmap_size=16, pls_rule="upstream")),
        "rgb_1layer": lambda: model_fixtures.rgb_head_scene(1), "rgb_3layer": lambda: model_fixtures.rgb_head_scene(3),
        "rgb_0layer": lambda: model_fixtures.linear_head_scene(1), "linear": lambda: model_fixtures.linear_head_scene(0),
    }
    rng = np.random.default_rng(12)
    env = np.zeros((16, 32, 4), np.float32)
    env[..., :3] = rng.uniform(0, 1, (16, 32, 3))
    env[..., 3] = rng.uniform(0.5, 1.0, (16, 32))
    env[..., :3] *= env[..., 3:4]
    # the probe kernel's own rays: from a sphere around the object towards points inside it
    n = 4096
    o = rng.normal(size=(n, 3))
    ray_o = (0.5 + 2.0 * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    d = rng.uniform(0.2, 0.8, (n, 3)) - ray_o
    ray_d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    meshes = ((meshio.icosphere(3), (0.55, -0.1, 0.0)), (meshio.torus(32, 16), (-0.3, 0.25, 0.4)))  # the hybrid frame's (caller rays would stop at them)

    def camera(w, h, az=45.0, el=30.0, radius=4.03, **kw):
        return native.make_camera(scene.orbit_camera(az, el, radius), w, h, scene.focal_from_fov_x(w, 0.6911), **kw)

    def render(frame):
        """-> rgba, depth (probe frames: what stands for them), counters or None"""
        if frame == "probe_envmap":
            e = ctx.compute_envmap(n_theta=64, n_phi=32)
            return e, ctx.get_envmap()[1], None  # (second array: the irradiance map convolved from it)
        if frame == "probe_rays":
            rgba, depth = ctx.trace_nerf_rays(ray_o, ray_d)
            return rgba, depth, None
        if frame == "packed":  # tile-packed output stays on the device
            cam, opts = camera(320, 180), native.make_opts(packed_output=True)
            m = native.load_library().ngp_packed_tiles(320, 180, 0, 1) * 64
            rgba, depth = torch.zeros((m, 4), device="cuda"), torch.zeros((m,), device="cuda")
            ctx.render_device(cam, opts, rgba.data_ptr(), depth.data_ptr(), None)
            torch.cuda.synchronize()
            rgba, depth = rgba.cpu().numpy(), depth.cpu().numpy()
        else:
            cam, opts = {
                "pinhole": lambda: (camera(256, 144), native.make_opts()),
                "inside": lambda: (camera(256, 144, az=20.0, el=10.0, radius=0.5), native.make_opts()),  # a camera inside the object
                "share8": lambda: (camera(320, 180), native.make_opts(shard_index=3, shard_count=8)),  # an interleaved 1/8 share
                "odd_101x67": lambda: (camera(101, 67, az=300.0), native.make_opts()),
                "8x8": lambda: (camera(8, 8), native.make_opts()),
                "1x1": lambda: (camera(1, 1), native.make_opts()),
                "spp4": lambda: (camera(200, 112, az=300.0, snap=False), native.make_opts(spp=4)),
                "depth_of_field": lambda: (camera(256, 144, az=200.0, aperture_size=0.05, focus_z=1.3), native.make_opts()),
                "depth_of_field_envmap": lambda: (camera(256, 144, az=200.0, aperture_size=0.05, focus_z=1.3), native.make_opts()),
                "normals": lambda: (camera(160, 90, az=70.0), native.make_opts(render_mode=native.RENDER_NORMALS)),
                "hybrid": lambda: (native.make_camera(scene.orbit_camera(60.0, 25.0, 5.5), 160, 90, scene.focal_from_fov_x(160, 0.8)), native.make_opts(testbed_mode=native.MODE_GEOMETRY)),
            }[frame]()
            if frame == "depth_of_field_envmap":
                ctx.set_envmap(env)
            if frame == "hybrid":
                for tris, centre in meshes:
                    ctx.add_mesh(tris, centre)
            try:
                rgba, depth = ctx.render(cam, opts, want_depth=True)
            finally:
                ctx.set_envmap(None)
                ctx.clear_meshes()
        st = ctx.render_stats()
        return rgba, depth, {k: int(st[k]) for k in ("n_rays", "n_rays_alive_after_init", "n_rays_hit", "n_samples")}

    records = []

    def run(group, sched, model, frame, anchors):
        print("SCHED %s FRAME %s/%s" % (",".join(map(str, sched)), model, frame), flush=True)
        rgba, depth, counters = render(frame)
        rec = dict(group=group, schedule=list(sched), model=model, frame=frame, rgba=sha(rgba), depth=sha(depth), nonzero=int(np.count_nonzero(rgba[..., :3])),
                   kernel="trace_probe_fused" if frame in PROBE_FRAMES else ctx.last_render_kernel())
        if counters:
            rec.update(counters)
        a = anchors.setdefault((group, model, frame), (rgba, depth))
        # the pixels that differ from the anchor's (none, if the knobs are what the header says): how many, and the first few
        for name, got, ref in (("rgba", rgba, a[0]), ("depth", depth, a[1])):
            diff = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32)  # bits, not values: -0.0 and NaN count
            if name == "rgba":
                diff = diff.any(-1)
            rec["diff_" + name] = int(np.count_nonzero(diff))
            rec["diff_" + name + "_first"] = [list(map(int, ix)) for ix in np.argwhere(diff)[:8]]
        records.append(rec)

    anchors = {}
    if env_route:
        sched = tuple(int(v) for v in os.environ["NGP_TUNE"].split(","))
        ctx.set_model(models["unit"]())
        for model, frame in ENV_FRAMES:
            run("env", sched, model, frame, anchors)
    else:
        for model in dict.fromkeys(m for m, _, _ in FRAMES):
            ctx.set_model(models[model]())
            for group, scheds in SCHEDULES.items():
                for sched in scheds:
                    ctx.set_schedule(*sched)
                    for m, frame, _ in FRAMES:
                        if m == model:
                            run(group, sched, model, frame, anchors)
    ctx.close()
    print("RECORDS " + json.dumps(records))


if __name__ == "__main__":
    main("--env-route" in sys.argv)
