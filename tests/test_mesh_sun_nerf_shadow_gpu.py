"""The NeRF in front of the frames' sun on the GPU (include/ngp_hip.h, "sun: the NeRF in front of the frames' sun"): the identities the
contract promises as bytes (which pin the split mesh pass to the fused one for every ambient source), the per-pixel record against the
ray-list tracer, the float64 reference and the oracle, the colour against the reference rendered with the recorded factor, and the
structure around it: determinism, samples, shards, devices, statistics, streams, refusals and bindings. Tolerances: TIE_EPS and the
float32 form's own deviation for q (test_irradiance_sun_shadow_gpu.py's rule), test_caller_rays_match_oracle's bound for alpha,
mesh_volume_cases' colour rule for the frame; none comes from the code under test. The measured figures are in DESIGN 3.15."""
import json
import subprocess

import numpy as np
import pytest

from conftest import pkg

import mesh_cases as mc
import mesh_reference as mref
import mesh_sun_nerf_shadow_cases as sc
import mesh_volume_cases as mv
import model_fixtures
from test_mesh_sun_nerf_shadow_cpu import oracle_alpha_s

pytestmark = pytest.mark.gpu

W, H = sc.WIDTH, sc.HEIGHT
INF = np.float32(np.inf)
NERF = (0.01, 0.0)   # min_transmittance, t_min
FAR = (0.01, 100.0)  # every shadow ray starts beyond the box
ALPHA_BOUND = 1e-2   # test_caller_rays_match_oracle's for scene_unit
VOLUME_BOX = (np.float32([-0.1, -0.2, -0.1]), np.float32([1.1, 0.7, 1.1]))
RICH = dict(ambientcolor=mv.SKY_AMBIENT, up_dir=(1.0, 0.0, 0.0), metallic=0.3, clearcoat=0.5, sheen=0.5)  # every term of the BRDF and the sky at work


def _load(c, scene):
    c.clear_meshes()
    for tris, center in scene:
        c.add_mesh(tris, center)


def _opts(native, mode=None, **kw):
    return native.make_opts(**dict(dict(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0), render_mode=native.RENDER_SHADE if mode is None else mode), **kw))


def _cam(native, w=W, h=H, **kw):
    return native.make_camera(sc.CAMERA, w, h, sc.FOCAL, **kw)


def _render(c, native, shadow, cam=None, **kw):
    c.set_sun_nerf_shadow(shadow)
    try:
        return c.render(cam or _cam(native), _opts(native, **kw), want_depth=True)
    finally:
        c.set_sun_nerf_shadow(None)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF over the floor, the default geometry options (sun (1, 1, 1))"""
    c = native.Context(0)
    c.set_model(scene_unit)
    _load(c, sc.scene())
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare(gpu_ctx, native):
    """the floor alone"""
    c = native.Context(0)
    _load(c, sc.scene())
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames(hybrid, bare, native):
    """the frames most tests compare: option off, option on with its record and statistics, the meshes alone"""
    off = _render(hybrid, native, None)
    off_stats = hybrid.render_stats()
    hybrid.set_sun_nerf_shadow(NERF)
    on = hybrid.render(_cam(native), _opts(native), want_depth=True)
    record = hybrid.frame_sun_shadow(W * H).reshape(H, W, 4)
    on_stats, shadow_ms, mesh_ms = hybrid.render_stats(), hybrid.frame_sun_shadow_ms(), hybrid.mesh_pass_ms()
    hybrid.set_sun_nerf_shadow(None)
    return dict(off=off, on=on, record=record, off_stats=off_stats, on_stats=on_stats, shadow_ms=shadow_ms, mesh_ms=mesh_ms, bare=_render(bare, native, None))


# ------------------------------------------------------------------------------------------------------- identities as bytes
def test_identities_as_bytes(hybrid, bare, frames, native, scene_unit):
    """option off after on, a t_min beyond the box, NeRF mode, a context of meshes alone and a model without density: each is the
    option-off frame, colour and depth"""
    off = frames["off"]
    assert (off[0][..., 3] > 0).sum() > 500 and not _same(frames["on"], off)
    assert _same(_render(hybrid, native, None), off)                      # off after on
    assert _same(_render(hybrid, native, FAR), off)                       # t_min = 100
    assert hybrid.sun_nerf_shadow() is None
    nerf_mode = dict(testbed_mode=native.MODE_NERF)
    assert _same(_render(hybrid, native, NERF, **nerf_mode), _render(hybrid, native, None, **nerf_mode))
    assert _same(_render(bare, native, NERF), frames["bare"])             # no model: no trace
    with pytest.raises(RuntimeError, match="traced no sun shadow rays"):
        bare.frame_sun_shadow(W * H)
    hybrid.clear_meshes()
    try:
        assert _same(_render(hybrid, native, NERF), _render(hybrid, native, None))  # Geometry mode without meshes
    finally:
        _load(hybrid, sc.scene())
    empty = native.Context(0)
    try:
        empty.set_model(dict(scene_unit, density_grid=np.zeros_like(scene_unit["density_grid"])))
        _load(empty, sc.scene())
        empty.set_geometry_opts()
        a, b = _render(empty, native, NERF), _render(empty, native, None)
        assert _same(a, b) and (a[0][..., 3] > 0).sum() > 500
    finally:
        empty.close()


@pytest.mark.parametrize("mode", ["Shade", "ShadeEnvMap", "ShadeGridEnvMap", "ShadeIrradianceVolume", "ShadeIrradianceVolumeVisible"])
def test_deferred_pass_is_the_fused_pass(mode, hybrid, native):
    """with every shadow ray beyond the box T_s = 1, and the frame of the split pass is the fused pass's as bytes: for each source of
    ambient light, with geometry options that put every term of the BRDF to work"""
    hybrid.set_geometry_opts(**RICH)
    try:
        if mode == "ShadeEnvMap":
            hybrid.compute_envmap(n_theta=16, n_phi=8)
        elif mode == "ShadeGridEnvMap":
            hybrid.compute_envmap_grid(2, 2, 16, 8)
        elif mode.startswith("ShadeIrradianceVolume"):
            hybrid.compute_irradiance_volume((3, 2, 3), VOLUME_BOX, 8, 8, occlude_by_meshes=False)
            if mode.endswith("Visible"):
                hybrid.compute_irradiance_volume_visibility(n_u=8, n_v=8, sharpness_log2=4, max_distance=0.0, normal_bias=0.01)
        kw = dict(mode={"Shade": native.RENDER_SHADE, "ShadeEnvMap": native.RENDER_SHADE_ENVMAP, "ShadeGridEnvMap": native.RENDER_SHADE_GRID_ENVMAP}.get(mode, native.RENDER_SHADE_IRRADIANCE_VOLUME))
        off, far, on = _render(hybrid, native, None, **kw), _render(hybrid, native, FAR, **kw), _render(hybrid, native, NERF, **kw)
        lit = off[0][..., :3].max(-1) > 1e-3
        print("\n%s: %d pixels with colour, largest %.3g; the shadow changes %d" % (mode, lit.sum(), off[0][..., :3].max(), (np.abs(on[0] - off[0]).max(-1) > 0).sum()))
        assert lit.sum() > 500 and np.unique(off[0][..., 0]).size > 100
        assert _same(far, off)
        assert not _same(on, off) and on[1].tobytes() == off[1].tobytes()
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.set_geometry_opts()


@pytest.mark.parametrize("lens", ["aperture", "fisheye"])
def test_deferred_pass_is_the_fused_pass_through_every_lens(lens, hybrid, bare, native):
    """test_deferred_pass_is_the_fused_pass where the primary ray is more than a pinhole's and the pixel map more than whole tiles: a thin
    lens (aperture_size > 0, a positive focus_z) and an OpenCV fisheye, 52 x 36 (a multiple of neither 8 nor 16), whole and as three
    tile-packed shards put together as in test_shards_and_packed_shards_cover_the_frame. With every shadow ray beyond the box the split
    pass's frame is the fused pass's as bytes, colour and depth, in both layouts. The comparison must not be one of empty frames: a primary ray
    has to find a triangle at a quarter of the pixels at least. They are counted in the frame of the meshes alone through the same camera,
    where no NeRF writes a depth: a depth of 0.01 or more, below MAX_DEPTH (a ray that chooses no mesh ends where it starts, at a depth
    under 1e-6, test_nerf_mesh_shadow_gpu.py's `behind`). mesh_reference.trace on these cameras' rays at pixel centres gives 782 of 1872
    for the fisheye and 808 to 817 for the thin lens, over draws of the point on the lens disk, its rim included; the pinhole's 812."""
    import torch

    w, h, world = 52, 36, 3
    kw = {"aperture": dict(aperture_size=0.05, focus_z=1.5), "fisheye": dict(lens_mode=native.LENS_OPENCV_FISHEYE, lens_params=(0.05, -0.01, 0.003, -0.0005))}[lens]
    cam = _cam(native, w=w, h=h, **kw)
    tile, slot = _tiles(w, h)
    src = (tile // world) * 64 + slot
    got = {}
    hybrid.set_geometry_opts(**RICH)
    try:
        for name, shadow in (("off", None), ("far", FAR)):
            hybrid.set_sun_nerf_shadow(shadow)
            full, full_depth = hybrid.render(cam, _opts(native), want_depth=True)
            packed, packed_depth = np.zeros_like(full), np.zeros_like(full_depth)
            for r in range(world):
                mine = tile % world == r
                n = native.load_library().ngp_packed_tiles(w, h, r, world) * 64
                rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
                dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
                hybrid.render_device(cam, _opts(native, shard_index=r, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
                torch.cuda.synchronize()
                packed[mine], packed_depth[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]]
            got[name] = (full, full_depth), (packed, packed_depth)
    finally:
        hybrid.set_sun_nerf_shadow(None)
        hybrid.set_geometry_opts()
    (off, off_packed), (far, far_packed) = got["off"], got["far"]
    mesh_depth = _render(bare, native, None, cam=cam)[1]
    hit = (mesh_depth >= np.float32(0.01)) & (mesh_depth < mref.MAX_DEPTH)
    assert hit.sum() >= w * h // 4, "%s: a triangle at %d of %d pixels" % (lens, hit.sum(), w * h)
    assert np.all(off[0][hit, 3] > 0) and np.unique(off[0][hit, 0]).size > 100  # the hybrid frame's mesh pixels: covered, and shaded
    assert _same(far, off) and _same(far_packed, off_packed)
    assert _same(off_packed, off)


# ---------------------------------------------------------------------------------------------------------------- the record
def test_record_matches_tracer_reference_and_oracle(hybrid, frames, native, oracle, scene_unit):
    """(a) alpha_s is ngp_trace_nerf_rays' alpha of (q_out, s^, (t_min, inf)) as bytes, for two descriptors; (b) q = 0 and alpha_s = 0
    exactly where the reference has no shadow ray (safe pixels); (c) |q - q64| <= TIE_EPS + GPU_FACTOR x the float32 form's deviation;
    (d) |alpha_s - the oracle's alpha on the reference's q| < 1e-2 on safe pixels; (e) the case's shares of blocked and open rays hold on
    the GPU's own alpha_s"""
    fr = sc.frame()
    s_hat = sc.s_hat()
    for nerf in (NERF, (0.05, 0.25)):
        hybrid.set_sun_nerf_shadow(nerf)
        try:
            hybrid.render(_cam(native), _opts(native))
            rec = hybrid.frame_sun_shadow(W * H).reshape(H, W, 4)
        finally:
            hybrid.set_sun_nerf_shadow(None)
        q, a = rec[..., :3], rec[..., 3]
        has = np.any(q != 0, axis=-1)
        assert np.isfinite(rec).all() and np.all(a[~has] == 0)
        n = int(has.sum())
        traced, _ = hybrid.trace_nerf_rays(q[has], np.tile(s_hat, (n, 1)), np.tile(np.float32([nerf[1], INF]), (n, 1)), nerf[0])
        assert a[has].tobytes() == traced[:, 3].tobytes() and (a > 0.9).any()   # (a)
        safe = ~fr["unsafe"]
        assert np.array_equal(has[safe], fr["has_ray"][safe])                   # (b)
    rec = frames["record"]
    q, a = rec[..., :3], rec[..., 3]
    has = np.any(q != 0, axis=-1)
    m = safe & fr["has_ray"]
    dq = np.abs(q.astype(np.float64) - fr["q"])[m].max()
    allow = mref.TIE_EPS + mc.GPU_FACTOR * fr["q_dev"]
    da = np.abs(a - oracle_alpha_s(oracle, scene_unit))[m].max()
    blocked, open_ = float((a[has] > 0.9).mean()), float((a[has] == 0).mean())
    print("\n%d pixels with a shadow ray (safe %d), alpha_s > 0.9: %d, = 0: %d, between: %d; |dq| %.2e (allowed %.2e, of it the float32 form x %g: %.2e); |dalpha| against the oracle %.2e"
          % (has.sum(), m.sum(), (a[has] > 0.9).sum(), (a[has] == 0).sum(), ((a[has] > 0) & (a[has] <= 0.9)).sum(), dq, allow, mc.GPU_FACTOR, mc.GPU_FACTOR * fr["q_dev"], da))
    assert (fr["unsafe"] & fr["covered"]).sum() <= mc.UNSAFE_CAP * fr["covered"].sum()
    assert dq <= allow, (dq, allow)                                             # (c)
    assert da < ALPHA_BOUND, da                                                 # (d)
    assert has.sum() >= sc.MIN_RAYS and blocked >= sc.BLOCKED_SHARE and open_ >= sc.OPEN_SHARE, (has.sum(), blocked, open_)  # (e)


# ---------------------------------------------------------------------------------------------------------------- the colour
def test_colour_is_the_reference_with_the_recorded_factor(frames):
    """Clear pixels: the option-off hybrid frame equals the frame of the meshes alone as bytes, so the NeRF pass added nothing there. On
    clear, safe pixels the option-on frame is the float64 reference rendered with factor = max(1 - alpha_s, 0), alpha_s from the record,
    within GPU_FACTOR x ORACLE_DEV_FRAME["defaults"][1] x max(1, |rgb_ref|). Everywhere: depth as the off frame's; pixels without a shadow
    ray or with alpha_s = 0 as the off frame's, as bytes; no pixel brighter than off; and at least one pixel darker by more than ten times
    the tolerance, which is what fails without the option."""
    (off, off_depth), (on, on_depth), (bare, bare_depth) = frames["off"], frames["on"], frames["bare"]
    rec = frames["record"]
    a = rec[..., 3]
    has = np.any(rec[..., :3] != 0, axis=-1)
    clear = np.all(off.view(np.uint32) == bare.view(np.uint32), axis=-1) & (off_depth.view(np.uint32) == bare_depth.view(np.uint32))
    fr = sc.frame(sc.factor_of(a))
    want = fr["rgba"][..., :3]
    bound = sc.frame_bound(want)
    m = clear & ~fr["unsafe"] & fr["covered"]
    ratio = np.abs(on[..., :3].astype(np.float64) - want)[m] / bound[m]
    n_blocked, n_open = int((m & has & (a > 0.9)).sum()), int((m & has & (a == 0)).sum())
    tol = sc.frame_bound(off[..., :3].astype(np.float64))
    brighter = (on[..., :3].astype(np.float64) - off[..., :3]) / tol
    darker = (off[..., :3].astype(np.float64) - on[..., :3]) / tol
    print("\nclear pixels %d (safe and covered %d; with alpha_s > 0.9: %d, = 0: %d); largest colour deviation / bound %.3f; brightest gain / tolerance %.3g; largest loss / tolerance %.3g (%.3g absolute)"
          % (clear.sum(), m.sum(), n_blocked, n_open, ratio.max(), brighter.max(), darker.max(), (off[..., :3] - on[..., :3]).max()))
    assert n_blocked >= 20 and n_open >= 20
    assert np.array_equal(on[..., 3][m], fr["rgba"][..., 3][m])
    assert ratio.max() <= 1.0, ratio.max()
    assert on_depth.tobytes() == off_depth.tobytes()
    same = ~has | (a == 0)
    assert on[same].tobytes() == off[same].tobytes()
    assert brighter.max() <= 1.0
    assert darker.max() > 10.0


# ----------------------------------------------------------------------------------------------------------------- structure
def test_two_runs_statistics_and_times(hybrid, frames, native):
    """a second run is the first as bytes, record included; the frame's statistics are its NeRF pass's alone; the shadow trace's time lies
    inside the mesh pass's and is 0 after a frame without it"""
    hybrid.set_sun_nerf_shadow(NERF)
    try:
        again = hybrid.render(_cam(native), _opts(native), want_depth=True)
        assert _same(again, frames["on"]) and hybrid.frame_sun_shadow(W * H).tobytes() == frames["record"].tobytes()
        with pytest.raises(RuntimeError, match="n_pixels"):
            hybrid.frame_sun_shadow(W * H - 1)
    finally:
        hybrid.set_sun_nerf_shadow(None)
    on, off = frames["on_stats"], frames["off_stats"]
    print("\nstatistics on %s\n           off %s\nshadow prep + trace %.3f ms of a mesh pass of %.3f ms" % (on, off, frames["shadow_ms"], frames["mesh_ms"]))
    for k in ("n_rays", "n_rays_alive_after_init", "n_rays_hit", "n_samples"):
        assert on[k] == off[k], k
    assert off["n_samples"] > 0
    assert 0 < frames["shadow_ms"] <= frames["mesh_ms"]
    _render(hybrid, native, None)
    assert hybrid.frame_sun_shadow_ms() == 0
    with pytest.raises(RuntimeError, match="traced no sun shadow rays"):
        hybrid.frame_sun_shadow(W * H)


def test_two_samples_per_pixel(hybrid, native):
    """2 spp with jittered samples: every sample is traced at its own pixel offset and the record is the last sample's, which is the record
    of the one-sample frame of that sample index; with every shadow ray beyond the box the frame is the option-off frame as bytes"""
    cam = _cam(native, snap=False)
    off = _render(hybrid, native, None, cam=cam, spp=2)
    assert _same(_render(hybrid, native, FAR, cam=cam, spp=2), off)
    hybrid.set_sun_nerf_shadow(NERF)
    try:
        on = hybrid.render(cam, _opts(native, spp=2), want_depth=True)
        rec2 = hybrid.frame_sun_shadow(W * H)
        hybrid.render(_cam(native, snap=False, spp_index=1), _opts(native))
        rec_last = hybrid.frame_sun_shadow(W * H)
        hybrid.render(cam, _opts(native))
        rec_first = hybrid.frame_sun_shadow(W * H)
    finally:
        hybrid.set_sun_nerf_shadow(None)
    assert rec2.tobytes() == rec_last.tobytes() and rec2.tobytes() != rec_first.tobytes()
    assert not _same(on, off) and on[1].tobytes() == off[1].tobytes() and np.all(on[0] <= off[0])
    n = np.any(rec2[:, :3] != 0, axis=-1)
    traced, _ = hybrid.trace_nerf_rays(rec2[n, :3], np.tile(sc.s_hat(), (int(n.sum()), 1)), np.tile(np.float32([0.0, INF]), (int(n.sum()), 1)), 0.01)
    assert rec2[n, 3].tobytes() == traced[:, 3].tobytes() and n.sum() >= sc.MIN_RAYS


def _tiles(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // 8) * ((w + 7) // 8) + xs // 8, (xs % 8) + 8 * (ys % 8)


def test_shards_and_packed_shards_cover_the_frame(hybrid, native):
    """three shards in image layout and tile-packed (60 x 44: partial tiles on both axes) against the whole frame: colour, depth and the
    record, as bytes"""
    import torch

    w, h, world = 60, 44, 3
    cam = _cam(native, w=w, h=h)
    tile, slot = _tiles(w, h)
    hybrid.set_sun_nerf_shadow(NERF)
    try:
        full, full_depth = hybrid.render(cam, _opts(native), want_depth=True)
        full_rec = hybrid.frame_sun_shadow(w * h).reshape(h, w, 4)
        assert (full_rec[..., 3] > 0.9).sum() > 20 and (full[..., 3] == 1).sum() > 500
        total, total_depth, total_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        packed, packed_depth, packed_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        for r in range(world):
            mine = tile % world == r
            part, part_depth = hybrid.render(cam, _opts(native, shard_index=r, shard_count=world), want_depth=True)
            rec = hybrid.frame_sun_shadow(w * h).reshape(h, w, 4)
            assert not np.any(part[~mine]) and not np.any(rec[~mine])
            total[mine], total_depth[mine], total_rec[mine] = part[mine], part_depth[mine], rec[mine]
            n = native.load_library().ngp_packed_tiles(w, h, r, world) * 64
            rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
            hybrid.render_device(cam, _opts(native, shard_index=r, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
            rec = hybrid.frame_sun_shadow(n)  # (synchronises the context's stream)
            src = (tile // world) * 64 + slot
            packed[mine], packed_depth[mine], packed_rec[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]], rec[src[mine]]
    finally:
        hybrid.set_sun_nerf_shadow(None)
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes() and total_rec.tobytes() == full_rec.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes() and packed_rec.tobytes() == full_rec.tobytes()


def test_two_devices_render_the_one_device_frame(frames, native, scene_unit):
    """a context of two devices (the same ordinal twice): the option reaches the replica with the geometry, each device traces its share,
    the frame is the one-device frame as bytes; the record is the primary's tile-packed share"""
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        _load(multi, sc.scene())
        multi.set_geometry_opts()
        assert _same(_render(multi, native, None), frames["off"])
        multi.set_sun_nerf_shadow(NERF)
        two = multi.render(_cam(native), _opts(native), want_depth=True)
        assert _same(two, frames["on"])
        n = native.load_library().ngp_packed_tiles(W, H, 0, 2) * 64
        rec = multi.frame_sun_shadow(n)
        tile, slot = _tiles(W, H)
        mine = tile % 2 == 0
        assert rec[((tile // 2) * 64 + slot)[mine]].tobytes() == frames["record"][mine].tobytes()
        st = multi.render_stats()
        for k in ("n_rays", "n_rays_hit", "n_samples"):
            assert st[k] == frames["off_stats"][k], k
        multi.set_sun_nerf_shadow(None)
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), frames["off"])  # and off reaches it too
    finally:
        multi.close()


def test_frame_on_a_callers_stream(hybrid, frames, native):
    """ngp_render_device on a caller's stream, then the caller's own synchronise: the same bytes"""
    import torch

    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    hybrid.set_sun_nerf_shadow(NERF)
    try:
        hybrid.render_device(_cam(native), _opts(native), rgba.data_ptr(), dep.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert rgba.cpu().numpy().tobytes() == frames["on"][0].tobytes() and dep.cpu().numpy().tobytes() == frames["on"][1].tobytes()
        assert hybrid.frame_sun_shadow(W * H).tobytes() == frames["record"].tobytes()
    finally:
        hybrid.set_sun_nerf_shadow(None)
    assert _same(_render(hybrid, native, None), frames["off"])  # (back on the context's own stream)


def test_refusal_for_a_model_the_tracer_does_not_serve(native):
    """configs/nerf/base_1layer.json: refused when the frame is rendered, with the tracer's message, naming the option; the same context
    renders with the option off, and in NeRF mode with it on"""
    c = native.Context(0)
    try:
        c.set_model(model_fixtures.rgb_head_scene(1))
        _load(c, sc.scene())
        c.set_geometry_opts()
        off = _render(c, native, None)
        c.set_sun_nerf_shadow(NERF)
        with pytest.raises(RuntimeError, match=r"sun_nerf_shadow frames \(ngp_set_sun_nerf_shadow\) are built for the configs/nerf/base.json rgb head"):
            c.render(_cam(native), _opts(native))
        c.render(_cam(native), _opts(native, testbed_mode=native.MODE_NERF))
        assert c.frame_sun_shadow_ms() == 0
        assert _same(_render(c, native, None), off) and (off[0][..., 3] > 0).sum() > 500
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------------------ bindings
def _write_scene(tmp_path, hybrid):
    """the floor as an .obj file, the unit NeRF as a snapshot, and the scene file that names them"""
    mi = pkg("meshio")
    entries = []
    for i, (tris, center) in enumerate(sc.scene()):
        mi.save_obj(str(tmp_path / ("floor%d.obj" % i)), tris)
        entries.append({"center": [float(x) for x in center], "path": "floor%d.obj" % i, "type": "Mesh"})
    hybrid.save_snapshot_file(str(tmp_path / "unit.ingp"))
    entries.append({"center": [0, 0, 0], "path": "unit.ingp", "type": "Nerf"})
    path = tmp_path / "floor_geometry_scene.json"  # (the Testbed takes a scene file for a Geometry scene by the word in its name)
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def _testbed(pyngp, scene, camera=True):
    tb = pyngp.Testbed()
    tb.load_training_data(scene)
    assert tb.mode == pyngp.TestbedMode.Geometry
    tb.background_color = [0.0, 0.0, 0.0, 0.0]
    tb.render_mode = pyngp.RenderMode.Shade
    if camera:  # (else the default camera, the command line's)
        tb.snap_to_pixel_centers = True
        tb.sun_dir = [1.0, 1.0, 1.0]
        tb.fov_axis = 0
        tb.relative_focal_length = [sc.FOCAL[0] / W, sc.FOCAL[1] / W]
        tb.camera_matrix = sc.CAMERA
    return tb


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    """testbed.sun_nerf_shadow (with its two parameters) gives the native frame as bytes, and --sun_nerf_shadow writes the frame the
    property gives, to the 8 bits of the file"""
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    scene = _write_scene(tmp_path, hybrid)
    cam = _cam(native)
    tb = _testbed(pyngp, scene)
    assert tb.sun_nerf_shadow is False and tb.sun_nerf_shadow_min_transmittance == np.float32(0.01) and tb.sun_nerf_shadow_t_min == 0.0
    off = tb.render(W, H, 1, True)
    tb.sun_nerf_shadow = True
    on = tb.render(W, H, 1, True)
    tb.sun_nerf_shadow_min_transmittance, tb.sun_nerf_shadow_t_min = 0.05, 0.25
    own = tb.render(W, H, 1, True)
    tb.sun_nerf_shadow = False
    assert tb.render(W, H, 1, True).tobytes() == off.tobytes()
    del tb
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        assert c.render(cam, _opts(native)).tobytes() == off.tobytes()
        c.set_sun_nerf_shadow(True)
        assert c.render(cam, _opts(native)).tobytes() == on.tobytes()
        c.set_sun_nerf_shadow(dict(min_transmittance=0.05, t_min=0.25))
        assert c.render(cam, _opts(native)).tobytes() == own.tobytes()
    finally:
        c.close()
    changed = np.abs(on - off).max(-1) > 0
    print("\npyngp: sun_nerf_shadow changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(on - off).max()))
    assert (on[..., 3] > 0).sum() > 500 and changed.sum() > 100 and on.tobytes() != own.tobytes()
    # the command line writes the frame of the default camera: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit)
    shots = {}
    for shadow in (False, True):
        tb = _testbed(pyngp, scene, camera=False)
        tb.sun_nerf_shadow = shadow
        shots[shadow] = tb.render(W, H, 1, True)
        del tb

    def as_png(frame):
        a = np.clip(frame[..., 3:4], 0, 1)
        v = np.clip(np.where(a > 0, frame[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
        srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
        return np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)

    expect = {k: as_png(v) for k, v in shots.items()}
    print("command line: the flag changes %d of %d pixels of the file" % ((expect[True] != expect[False]).any(-1).sum(), W * H))
    assert (expect[True] != expect[False]).any(-1).sum() > 20
    exe = pkg("build").build_main()
    for shadow in (True, False):
        out = tmp_path / ("shot%d.png" % shadow)
        r = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "Shade", "--width", str(W), "--height", str(H), "--screenshot", str(out)]
                           + (["--sun_nerf_shadow", "--sun_nerf_shadow_t_min", "0"] if shadow else []), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        png = np.asarray(Image.open(out)).astype(np.int64)
        assert png.shape == (H, W, 4) and np.abs(png - expect[shadow]).max() <= 1 and (png != expect[shadow]).mean() < 0.01, (shadow, np.abs(png - expect[shadow]).max(), (png != expect[shadow]).mean())
        assert (png[..., 3] > 0).sum() > 100
