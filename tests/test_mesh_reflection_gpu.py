"""The NeRF mirrored in the meshes on the GPU (include/ngp_hip.h, "mesh reflection"): the identities the contract promises as bytes, the
per-pixel record against the ray-list tracer, the float64 reference and the oracle, the colour against the reference rendered with the
recorded radiance, and the structure around it: determinism, samples, shards, devices, statistics, streams, refusals and bindings.
Tolerances: TIE_EPS and the float32 form's own deviation for q and r (test_mesh_sun_nerf_shadow_gpu.py's rule), mesh_cases.position_tolerance
on the float32 form's deviation for t_hit, test_caller_rays_match_oracle's bound for alpha and rgb, mesh_sun_nerf_shadow_cases' colour rule for
the frame; none comes from the code under test. The measured figures are in DESIGN 3.18."""
import json
import subprocess

import numpy as np
import pytest

from conftest import pkg

import mesh_cases as mc
import mesh_reference as mref
import mesh_reflection_cases as rc
import mesh_volume_cases as mv
import model_fixtures
from test_mesh_reflection_cpu import oracle_reflection

pytestmark = pytest.mark.gpu

W, H = rc.WIDTH, rc.HEIGHT
INF = np.float32(np.inf)
ON = dict(strength=1.0, min_transmittance=0.01, t_min=0.0)
OWN = dict(strength=0.5, min_transmittance=0.05, t_min=0.25)
FAR = dict(strength=1.0, min_transmittance=0.01, t_min=100.0)  # every ray starts beyond the box (its diagonal is 15.6)
SUN_NERF, SUN_FAR = (0.01, 0.0), (0.01, 100.0)
TRACE_BOUND = 1e-2  # test_caller_rays_match_oracle's for scene_unit, alpha and rgb alike
VOLUME_BOX = (np.float32([-0.1, -0.2, -0.1]), np.float32([1.1, 0.7, 1.1]))
RICH = dict(ambientcolor=mv.SKY_AMBIENT, up_dir=(1.0, 0.0, 0.0), metallic=0.3, clearcoat=0.5, sheen=0.5)  # every term of the BRDF and the sky at work


def _load(c, scene):
    c.clear_meshes()
    for tris, center in scene:
        c.add_mesh(tris, center)


def _opts(native, mode=None, **kw):
    return native.make_opts(**dict(dict(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0), render_mode=native.RENDER_SHADE if mode is None else mode), **kw))


def _cam(native, w=W, h=H, **kw):
    return native.make_camera(rc.CAMERA, w, h, rc.FOCAL, **kw)


def _render(c, native, reflection, cam=None, sun=None, **kw):
    c.set_mesh_reflection(reflection)
    c.set_sun_nerf_shadow(sun)
    try:
        return c.render(cam or _cam(native), _opts(native, **kw), want_depth=True)
    finally:
        c.set_mesh_reflection(None)
        c.set_sun_nerf_shadow(None)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _record(c, n=W * H):
    return c.frame_mesh_reflection(n)


def _split(rec):
    """(q, t_hit, r, rgba, owns) of a record (..., 12); a pixel owns a ray where r is not zero"""
    return rec[..., 0:3], rec[..., 3], rec[..., 4:7], rec[..., 8:12], np.any(rec[..., 4:7] != 0, axis=-1)


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF over the floor (case A), the default geometry options (sun (1, 1, 1))"""
    c = native.Context(0)
    c.set_model(scene_unit)
    _load(c, rc.scene("A"))
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare(gpu_ctx, native):
    """the floor alone"""
    c = native.Context(0)
    _load(c, rc.scene("A"))
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames(hybrid, bare, native):
    """the frames most tests compare: option off, option on with its record and statistics, the meshes alone"""
    off = _render(hybrid, native, None)
    off_stats = hybrid.render_stats()
    hybrid.set_mesh_reflection(ON)
    on = hybrid.render(_cam(native), _opts(native), want_depth=True)
    record = _record(hybrid).reshape(H, W, 12)
    on_stats, trace_ms, mesh_ms = hybrid.render_stats(), hybrid.frame_mesh_reflection_ms(), hybrid.mesh_pass_ms()
    hybrid.set_mesh_reflection(None)
    return dict(off=off, on=on, record=record, off_stats=off_stats, on_stats=on_stats, trace_ms=trace_ms, mesh_ms=mesh_ms, bare=_render(bare, native, None))


# ------------------------------------------------------------------------------------------------------- identities as bytes
def test_identities_as_bytes(hybrid, bare, frames, native, scene_unit):
    """option off after on, strength 0 (no trace is run), a t_min beyond the box, NeRF mode, a context of meshes alone, Geometry mode without
    meshes and a model without density: each is the option-off frame, colour and depth"""
    off = frames["off"]
    assert (off[0][..., 3] > 0).sum() > 500 and not _same(frames["on"], off)
    assert _same(_render(hybrid, native, None), off)                      # off after on
    assert _same(_render(hybrid, native, FAR), off)                       # t_min = 100
    assert hybrid.mesh_reflection() is None
    hybrid.set_mesh_reflection(dict(strength=0.0))
    try:
        assert _same(hybrid.render(_cam(native), _opts(native), want_depth=True), off)  # strength 0 ...
        assert hybrid.frame_mesh_reflection_ms() == 0
        with pytest.raises(RuntimeError, match="traced no reflection rays"):            # ... and no trace was run
            _record(hybrid)
    finally:
        hybrid.set_mesh_reflection(None)
    nerf_mode = dict(testbed_mode=native.MODE_NERF)
    assert _same(_render(hybrid, native, ON, **nerf_mode), _render(hybrid, native, None, **nerf_mode))
    assert _same(_render(bare, native, ON), frames["bare"])               # no model: no trace
    with pytest.raises(RuntimeError, match="traced no reflection rays"):
        _record(bare)
    hybrid.clear_meshes()
    try:
        assert _same(_render(hybrid, native, ON), _render(hybrid, native, None))  # Geometry mode without meshes
    finally:
        _load(hybrid, rc.scene("A"))
    empty = native.Context(0)
    try:
        empty.set_model(dict(scene_unit, density_grid=np.zeros_like(scene_unit["density_grid"])))
        _load(empty, rc.scene("A"))
        empty.set_geometry_opts()
        a, b = _render(empty, native, ON), _render(empty, native, None)
        assert _same(a, b) and (a[0][..., 3] > 0).sum() > 500
    finally:
        empty.close()


@pytest.mark.parametrize("mode", ["Shade", "ShadeEnvMap", "ShadeGridEnvMap", "ShadeIrradianceVolume", "ShadeIrradianceVolumeVisible"])
def test_far_rays_leave_every_ambient_source_alone(mode, hybrid, native):
    """with every mirror ray beyond the box alpha_r = 0, and the frame of the split pass without a shadow trace is the fused pass's as bytes:
    for each source of ambient light, with geometry options that put every term of the BRDF to work; with the rays traced the frame changes
    and its depth does not"""
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
        off, far, on = _render(hybrid, native, None, **kw), _render(hybrid, native, FAR, **kw), _render(hybrid, native, ON, **kw)
        lit = off[0][..., :3].max(-1) > 1e-3
        print("\n%s: %d pixels with colour, largest %.3g; the reflection changes %d" % (mode, lit.sum(), off[0][..., :3].max(), (np.abs(on[0] - off[0]).max(-1) > 0).sum()))
        assert lit.sum() > 500 and np.unique(off[0][..., 0]).size > 100
        assert _same(far, off)
        assert not _same(on, off) and on[1].tobytes() == off[1].tobytes()
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.set_geometry_opts()


def test_with_the_sun_shadow_on_each_option_keeps_its_record_and_identities(hybrid, frames, native):
    """both options on: the sun-shadow record is that of the frame with the sun shadow alone and the reflection record that of the frame with
    the reflection alone, as bytes; with the other option's rays beyond the box each frame is the single-option frame as bytes"""
    sun_only = _render(hybrid, native, None, sun=SUN_NERF)
    hybrid.set_sun_nerf_shadow(SUN_NERF)
    try:
        hybrid.render(_cam(native), _opts(native))
        sun_rec = hybrid.frame_sun_shadow(W * H)
        with pytest.raises(RuntimeError, match="traced no reflection rays"):
            _record(hybrid)
        hybrid.set_mesh_reflection(ON)
        both = hybrid.render(_cam(native), _opts(native), want_depth=True)
        assert hybrid.frame_sun_shadow(W * H).tobytes() == sun_rec.tobytes() and (sun_rec[:, 3] > 0.9).sum() > 20
        assert _record(hybrid).tobytes() == frames["record"].tobytes()
        assert 0 < hybrid.frame_mesh_reflection_ms() and 0 < hybrid.frame_sun_shadow_ms()
        assert hybrid.frame_mesh_reflection_ms() + hybrid.frame_sun_shadow_ms() <= hybrid.mesh_pass_ms()
    finally:
        hybrid.set_mesh_reflection(None)
        hybrid.set_sun_nerf_shadow(None)
    assert not _same(both, sun_only) and not _same(both, frames["on"]) and both[1].tobytes() == frames["off"][1].tobytes()
    assert _same(_render(hybrid, native, FAR, sun=SUN_NERF), sun_only)            # the sun-shadow frame identity holds under the option
    assert _same(_render(hybrid, native, ON, sun=SUN_FAR), frames["on"])          # and this option's under the sun shadow
    assert _same(_render(hybrid, native, FAR, sun=SUN_FAR), frames["off"])
    hybrid.set_mesh_reflection(ON)                                              # reflection alone: no shadow trace is run
    try:
        hybrid.render(_cam(native), _opts(native))
        assert hybrid.frame_sun_shadow_ms() == 0
        with pytest.raises(RuntimeError, match="traced no sun shadow rays"):
            hybrid.frame_sun_shadow(W * H)
    finally:
        hybrid.set_mesh_reflection(None)


# ---------------------------------------------------------------------------------------------------------------- the record
def test_record_matches_tracer_reference_and_oracle(hybrid, frames, native, oracle, scene_unit):
    """case A. (a) (rgb_r, alpha_r) is ngp_trace_nerf_rays' rgba of the recorded (q, r, (t_min, t_hit)) as bytes, for two descriptors; (b) a
    pixel owns a ray exactly where the reference's does (safe pixels), and the record is zero elsewhere; (c) |q - q64| and |r - r64| <=
    TIE_EPS + GPU_FACTOR x the float32 form's deviation; (d) no ray is cut: t_hit = inf; (e) |alpha_r - the oracle's| and |rgb_r - the
    oracle's| < 1e-2 on safe pixels; (f) the case's shares of full and empty rays hold on the GPU's own alpha_r"""
    fr = rc.frame("A")
    safe = ~fr["unsafe"] & ~fr["t_unsafe"]
    for desc in (ON, OWN):
        hybrid.set_mesh_reflection(desc)
        try:
            hybrid.render(_cam(native), _opts(native))
            rec = _record(hybrid).reshape(H, W, 12)
        finally:
            hybrid.set_mesh_reflection(None)
        q, t_hit, r, rgba, owns = _split(rec)
        assert not np.isnan(rec).any() and not np.any(rec[~owns]) and np.all(rec[..., 7] == 0)
        n = int(owns.sum())
        t = np.stack([np.full(n, desc["t_min"], np.float32), t_hit[owns]], 1)
        traced, _ = hybrid.trace_nerf_rays(q[owns], r[owns], t, desc["min_transmittance"])
        assert rgba[owns].tobytes() == traced.tobytes() and (rgba[..., 3] > 0.9).any()   # (a)
        assert np.array_equal(owns[safe], fr["owns"][safe])                                # (b)
    assert not np.array_equal(rec, frames["record"])  # (the second descriptor traces other rays)
    q, t_hit, r, rgba, owns = _split(frames["record"])
    m = safe & fr["owns"]
    dq, dr = np.abs(q.astype(np.float64) - fr["rq"])[m].max(), np.abs(r.astype(np.float64) - fr["r"])[m].max()
    allow_q, allow_r = mref.TIE_EPS + mc.GPU_FACTOR * fr["rq_dev"], mref.TIE_EPS + mc.GPU_FACTOR * fr["r_dev"]
    want = oracle_reflection(oracle, scene_unit, "A")
    da, dc = np.abs(rgba[..., 3] - want[..., 3])[m].max(), np.abs(rgba[..., :3] - want[..., :3])[m].max()
    a = rgba[..., 3][owns]
    print("\n%d pixels own a ray (safe %d), alpha_r > 0.9: %d, = 0: %d, between: %d; |dq| %.2e (allowed %.2e), |dr| %.2e (allowed %.2e); against the oracle |dalpha| %.2e, |drgb| %.2e"
          % (owns.sum(), m.sum(), (a > 0.9).sum(), (a == 0).sum(), ((a > 0) & (a <= 0.9)).sum(), dq, allow_q, dr, allow_r, da, dc))
    assert (fr["unsafe"] & fr["covered"]).sum() <= mc.UNSAFE_CAP * fr["covered"].sum()
    assert dq <= allow_q and dr <= allow_r, (dq, allow_q, dr, allow_r)                     # (c)
    assert np.all(np.isinf(t_hit[owns]))                                                   # (d)
    assert da < TRACE_BOUND and dc < TRACE_BOUND, (da, dc)                                 # (e)
    assert owns.sum() >= rc.MIN_RAYS and (a > 0.9).mean() >= rc.FULL_SHARE and (a == 0).mean() >= rc.EMPTY_SHARE  # (f)


def test_a_mesh_in_the_way_cuts_the_ray(native, oracle, scene_unit):
    """case B. The rays the reference finds cut have a finite t_hit within mesh_cases.position_tolerance of the reference's (the deviation:
    the float32 form's own), every other owner's is inf; the record is the tracer's rgba of (q, r, (0, t_hit)) as bytes; a cut ray's alpha_r
    is at most that of the same ray traced uncut, and strictly less on at least 50 of the rays whose uncut alpha_r the oracle puts above 0.9;
    a covered pixel whose primary ray found no triangle owns no ray"""
    fr = rc.frame("B")
    c = native.Context(0)
    try:
        c.set_model(scene_unit)
        _load(c, rc.scene("B"))
        c.set_geometry_opts()
        off = _render(c, native, None)
        c.set_mesh_reflection(ON)
        on = c.render(_cam(native), _opts(native), want_depth=True)
        rec = _record(c).reshape(H, W, 12)
        q, t_hit, r, rgba, owns = _split(rec)
        n = int(owns.sum())
        traced, _ = c.trace_nerf_rays(q[owns], r[owns], np.stack([np.zeros(n, np.float32), t_hit[owns]], 1), 0.01)
        uncut, _ = c.trace_nerf_rays(q[owns], r[owns], np.tile(np.float32([0.0, INF]), (n, 1)), 0.01)
    finally:
        c.close()
    safe = ~fr["unsafe"] & ~fr["t_unsafe"]
    assert np.array_equal(owns[safe], fr["owns"][safe]) and (fr["covered"] & ~fr["owns"]).sum() > 500 and not np.any(rec[~owns])
    assert on[1].tobytes() == off[1].tobytes() and (off[0][..., 3] == 1).all()  # covered everywhere, by a triangle or not
    assert rgba[owns].tobytes() == traced.tobytes()
    cut_ref = fr["owns"] & np.isfinite(fr["t_hit"])
    cut = owns & np.isfinite(t_hit)
    m = safe & fr["owns"]
    assert np.array_equal(cut[m], cut_ref[m]) and np.all(t_hit[owns & ~cut] == INF)
    mc_ = m & cut_ref
    dt = np.abs(t_hit[mc_].astype(np.float64) - fr["t_hit"][mc_])
    tol = mc.position_tolerance(fr["t_dev"], fr["t_hit"][mc_])
    full = np.zeros((H, W, 4), np.float32)
    full[owns] = uncut
    a, a_uncut = rgba[..., 3], full[..., 3]
    named = mc_ & (oracle_reflection(oracle, scene_unit, "B")[..., 3] > 0.9)
    less = named & (a < a_uncut)
    print("\n%d owners, %d cut (safe %d); |dt_hit| / tolerance %.3f (largest |dt_hit| %.2e); cut rays whose uncut alpha_r the oracle puts above 0.9: %d, of them strictly less: %d (alpha_r at most %.3f)"
          % (owns.sum(), cut.sum(), mc_.sum(), (dt / tol).max(), dt.max(), named.sum(), less.sum(), a[less].max() if less.any() else 0))
    assert mc_.sum() >= rc.MIN_CUT and named.sum() >= rc.MIN_CUT_FULL
    assert np.all(dt <= tol), (dt / tol).max()
    assert np.all(a[cut] <= a_uncut[cut]) and np.all(rgba[..., :3][cut] <= full[..., :3][cut])
    assert less.sum() >= rc.MIN_CUT_FULL, less.sum()
    assert rgba[owns & ~cut].tobytes() == full[owns & ~cut].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the colour
def test_colour_is_the_reference_with_the_recorded_radiance(hybrid, frames, native):
    """Clear pixels: the option-off hybrid frame equals the frame of the meshes alone as bytes, so the NeRF pass added nothing there. On
    clear, safe pixels the option-on frame is the float64 reference rendered with the recorded (rgb_r, alpha_r), within GPU_FACTOR x
    ORACLE_DEV_FRAME["defaults"][1] x max(1, |rgb_ref|). Everywhere: depth as the off frame's; pixels without a ray or with alpha_r = 0 as
    the off frame's, as bytes; no pixel darker than off; and at least one pixel brighter by more than ten times the tolerance, which is what
    fails without the option. Then the term alone under a tinted metal: on - off against the reference's added term, within a rounding of
    the sum plus GPU_FACTOR x the float32 form's own deviation of the term."""
    (off, off_depth), (on, on_depth), (bare, bare_depth) = frames["off"], frames["on"], frames["bare"]
    q, t_hit, r, rgba, owns = _split(frames["record"])
    a = rgba[..., 3]
    clear = np.all(off.view(np.uint32) == bare.view(np.uint32), axis=-1) & (off_depth.view(np.uint32) == bare_depth.view(np.uint32))
    fr = rc.frame("A", rgba)
    want = fr["rgba"][..., :3]
    bound = rc.frame_bound(want)
    m = clear & ~fr["unsafe"] & fr["covered"]
    ratio = np.abs(on[..., :3].astype(np.float64) - want)[m] / bound[m]
    n_full, n_empty = int((m & owns & (a > 0.9)).sum()), int((m & owns & (a == 0)).sum())
    tol = rc.frame_bound(off[..., :3].astype(np.float64))
    brighter = (on[..., :3].astype(np.float64) - off[..., :3]) / tol
    darker = (off[..., :3].astype(np.float64) - on[..., :3]) / tol
    print("\nclear pixels %d (safe and covered %d; owners with alpha_r > 0.9: %d, = 0: %d); largest colour deviation / bound %.3f; largest gain / tolerance %.3g (%.3g absolute); largest loss / tolerance %.3g"
          % (clear.sum(), m.sum(), n_full, n_empty, ratio.max(), brighter.max(), (on[..., :3] - off[..., :3]).max(), darker.max()))
    assert n_full >= 20 and n_empty >= 20
    assert np.array_equal(on[..., 3][m], fr["rgba"][..., 3][m])
    assert ratio.max() <= 1.0, ratio.max()
    assert on_depth.tobytes() == off_depth.tobytes()
    same = ~owns | (a == 0)
    assert on[same].tobytes() == off[same].tobytes()
    assert darker.max() <= 0.0
    assert brighter.max() > 10.0
    # a tinted metal at half strength: F carries the base colour
    metal = dict(metallic=0.7, specular=0.5, basecolor=(0.9, 0.5, 0.1))
    hybrid.set_geometry_opts(**metal)
    try:
        m_off = _render(hybrid, native, None)
        hybrid.set_mesh_reflection(dict(strength=0.5))
        m_on = hybrid.render(_cam(native), _opts(native), want_depth=True)
        m_rgba = _split(_record(hybrid).reshape(H, W, 12))[3]
    finally:
        hybrid.set_mesh_reflection(None)
        hybrid.set_geometry_opts()
    assert m_rgba.tobytes() == rgba.tobytes()  # the rays are the geometry's, not the material's
    mf = rc.frame("A", m_rgba, strength=0.5, **metal)
    term = m_on[0][..., :3].astype(np.float64) - m_off[0][..., :3]
    dev32 = np.abs(mf["added32"].astype(np.float64) - mf["added"])[m].max()
    allow = 2.0 ** -24 * np.maximum(1.0, np.abs(m_on[0][..., :3])) + mc.GPU_FACTOR * dev32
    t_ratio = (np.abs(term - mf["added"]) / allow)[m]
    print("tinted metal: largest added term %.3g, |term - reference| / allowance %.3f (the float32 form deviates by %.2e)" % (mf["added"][m].max(), t_ratio.max(), dev32))
    assert t_ratio.max() <= 1.0 and mf["added"][m].max() > 0.05
    tint = mf["F"][m & owns]
    assert np.all(tint[:, 0] > tint[:, 1]) and np.all(tint[:, 1] > tint[:, 2])  # (the reference's F is red over green over blue: the metal's own colour)


# ----------------------------------------------------------------------------------------------------------------- structure
def test_two_runs_statistics_and_times(hybrid, frames, native):
    """a second run is the first as bytes, record included; the frame's statistics are its NeRF pass's alone; the reflection trace's time
    lies inside the mesh pass's and is 0 after a frame without it"""
    hybrid.set_mesh_reflection(ON)
    try:
        again = hybrid.render(_cam(native), _opts(native), want_depth=True)
        assert _same(again, frames["on"]) and _record(hybrid).tobytes() == frames["record"].tobytes()
        with pytest.raises(RuntimeError, match="n_pixels"):
            _record(hybrid, W * H - 1)
    finally:
        hybrid.set_mesh_reflection(None)
    on, off = frames["on_stats"], frames["off_stats"]
    print("\nstatistics on %s\n           off %s\nreflection prep + trace %.3f ms of a mesh pass of %.3f ms" % (on, off, frames["trace_ms"], frames["mesh_ms"]))
    for k in ("n_rays", "n_rays_alive_after_init", "n_rays_hit", "n_samples"):
        assert on[k] == off[k], k
    assert off["n_samples"] > 0
    assert 0 < frames["trace_ms"] <= frames["mesh_ms"]
    _render(hybrid, native, None)
    assert hybrid.frame_mesh_reflection_ms() == 0
    with pytest.raises(RuntimeError, match="traced no reflection rays"):
        _record(hybrid)


def test_two_samples_per_pixel(hybrid, native):
    """2 spp with jittered samples: every sample is traced at its own pixel offset and the record is the last sample's, which is the record
    of the one-sample frame of that sample index; with every ray beyond the box the frame is the option-off frame as bytes"""
    cam = _cam(native, snap=False)
    off = _render(hybrid, native, None, cam=cam, spp=2)
    assert _same(_render(hybrid, native, FAR, cam=cam, spp=2), off)
    hybrid.set_mesh_reflection(ON)
    try:
        on = hybrid.render(cam, _opts(native, spp=2), want_depth=True)
        rec2 = _record(hybrid)
        hybrid.render(_cam(native, snap=False, spp_index=1), _opts(native))
        rec_last = _record(hybrid)
        hybrid.render(cam, _opts(native))
        rec_first = _record(hybrid)
    finally:
        hybrid.set_mesh_reflection(None)
    assert rec2.tobytes() == rec_last.tobytes() and rec2.tobytes() != rec_first.tobytes()
    assert not _same(on, off) and on[1].tobytes() == off[1].tobytes() and np.all(on[0] >= off[0])
    q, t_hit, r, rgba, owns = _split(rec2)
    n = int(owns.sum())
    traced, _ = hybrid.trace_nerf_rays(q[owns], r[owns], np.stack([np.zeros(n, np.float32), t_hit[owns]], 1), 0.01)
    assert rgba[owns].tobytes() == traced.tobytes() and n >= rc.MIN_RAYS


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
    hybrid.set_mesh_reflection(ON)
    try:
        full, full_depth = hybrid.render(cam, _opts(native), want_depth=True)
        full_rec = _record(hybrid, w * h).reshape(h, w, 12)
        assert (full_rec[..., 11] > 0.9).sum() > 20 and (full[..., 3] == 1).sum() > 500
        total, total_depth, total_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        packed, packed_depth, packed_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        for rank in range(world):
            mine = tile % world == rank
            part, part_depth = hybrid.render(cam, _opts(native, shard_index=rank, shard_count=world), want_depth=True)
            rec = _record(hybrid, w * h).reshape(h, w, 12)
            assert not np.any(part[~mine]) and not np.any(rec[~mine])
            total[mine], total_depth[mine], total_rec[mine] = part[mine], part_depth[mine], rec[mine]
            n = native.load_library().ngp_packed_tiles(w, h, rank, world) * 64
            rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
            hybrid.render_device(cam, _opts(native, shard_index=rank, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
            rec = _record(hybrid, n)  # (synchronises the context's stream)
            src = (tile // world) * 64 + slot
            packed[mine], packed_depth[mine], packed_rec[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]], rec[src[mine]]
    finally:
        hybrid.set_mesh_reflection(None)
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes() and total_rec.tobytes() == full_rec.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes() and packed_rec.tobytes() == full_rec.tobytes()


def test_two_devices_render_the_one_device_frame(frames, native, scene_unit):
    """a context of two devices (the same ordinal twice): the option reaches the replica with the geometry, each device traces its share,
    the frame is the one-device frame as bytes; the record is the primary's tile-packed share"""
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        _load(multi, rc.scene("A"))
        multi.set_geometry_opts()
        assert _same(_render(multi, native, None), frames["off"])
        multi.set_mesh_reflection(ON)
        two = multi.render(_cam(native), _opts(native), want_depth=True)
        assert _same(two, frames["on"])
        n = native.load_library().ngp_packed_tiles(W, H, 0, 2) * 64
        rec = _record(multi, n)
        tile, slot = _tiles(W, H)
        mine = tile % 2 == 0
        assert rec[((tile // 2) * 64 + slot)[mine]].tobytes() == frames["record"][mine].tobytes()
        assert multi.frame_mesh_reflection_ms() > 0
        st = multi.render_stats()
        for k in ("n_rays", "n_rays_hit", "n_samples"):
            assert st[k] == frames["off_stats"][k], k
        multi.set_mesh_reflection(None)
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), frames["off"])  # and off reaches it too
    finally:
        multi.close()


def test_frame_on_a_callers_stream(hybrid, frames, native):
    """ngp_render_device on a caller's stream, then the caller's own synchronise: the same bytes"""
    import torch

    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    hybrid.set_mesh_reflection(ON)
    try:
        hybrid.render_device(_cam(native), _opts(native), rgba.data_ptr(), dep.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert rgba.cpu().numpy().tobytes() == frames["on"][0].tobytes() and dep.cpu().numpy().tobytes() == frames["on"][1].tobytes()
        assert _record(hybrid).tobytes() == frames["record"].tobytes()
    finally:
        hybrid.set_mesh_reflection(None)
    assert _same(_render(hybrid, native, None), frames["off"])  # (back on the context's own stream)


def test_refusal_for_a_model_the_tracer_does_not_serve(native):
    """configs/nerf/base_1layer.json: refused when the frame is rendered, with the tracer's message, naming the option; the same context
    renders with the option off, with strength 0, and in NeRF mode with it on"""
    c = native.Context(0)
    try:
        c.set_model(model_fixtures.rgb_head_scene(1))
        _load(c, rc.scene("A"))
        c.set_geometry_opts()
        off = _render(c, native, None)
        c.set_mesh_reflection(ON)
        with pytest.raises(RuntimeError, match=r"mesh_reflection frames \(ngp_set_mesh_reflection\) are built for the configs/nerf/base.json rgb head"):
            c.render(_cam(native), _opts(native))
        c.render(_cam(native), _opts(native, testbed_mode=native.MODE_NERF))
        assert c.frame_mesh_reflection_ms() == 0
        assert _same(_render(c, native, dict(strength=0.0)), off)
        assert _same(_render(c, native, None), off) and (off[0][..., 3] > 0).sum() > 500
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------------------ bindings
RAISED_FLOOR_CENTER = (0.0, -0.405, 0.0)  # the floor's top at y = 0.1, just under the object's base plate at y = 0.2


def _write_scene(tmp_path, hybrid, center=None, name="floor"):
    """the floor as an .obj file (center: its own centre, else the case's), the unit NeRF as a snapshot, and the scene file that names them"""
    mi = pkg("meshio")
    entries = []
    for i, (tris, c) in enumerate(rc.scene("A")):
        mi.save_obj(str(tmp_path / ("%s%d.obj" % (name, i))), tris)
        entries.append({"center": [float(x) for x in (center or c)], "path": "%s%d.obj" % (name, i), "type": "Mesh"})
    hybrid.save_snapshot_file(str(tmp_path / "unit.ingp"))
    entries.append({"center": [0, 0, 0], "path": "unit.ingp", "type": "Nerf"})
    path = tmp_path / ("%s_geometry_scene.json" % name)  # (the Testbed takes a scene file for a Geometry scene by the word in its name)
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
        tb.relative_focal_length = [rc.FOCAL[0] / W, rc.FOCAL[1] / W]
        tb.camera_matrix = rc.CAMERA
    return tb


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    """testbed.mesh_reflection (with its three parameters) gives the native frame as bytes, and --mesh_reflection writes the frame the
    property gives, to the 8 bits of the file"""
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    scene = _write_scene(tmp_path, hybrid)
    cam = _cam(native)
    tb = _testbed(pyngp, scene)
    assert tb.mesh_reflection is False and tb.mesh_reflection_strength == 1.0 and tb.mesh_reflection_min_transmittance == np.float32(0.01) and tb.mesh_reflection_t_min == 0.0
    off = tb.render(W, H, 1, True)
    tb.mesh_reflection = True
    on = tb.render(W, H, 1, True)
    tb.mesh_reflection_strength, tb.mesh_reflection_min_transmittance, tb.mesh_reflection_t_min = 0.5, 0.05, 0.25
    own = tb.render(W, H, 1, True)
    tb.mesh_reflection = False
    assert tb.render(W, H, 1, True).tobytes() == off.tobytes()
    del tb
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        assert c.render(cam, _opts(native)).tobytes() == off.tobytes()
        c.set_mesh_reflection(True)
        assert c.render(cam, _opts(native)).tobytes() == on.tobytes()
        c.set_mesh_reflection(OWN)
        assert c.render(cam, _opts(native)).tobytes() == own.tobytes()
    finally:
        c.close()
    changed = np.abs(on - off).max(-1) > 0
    print("\npyngp: mesh_reflection changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(on - off).max()))
    assert (on[..., 3] > 0).sum() > 500 and changed.sum() > 100 and on.tobytes() != own.tobytes()
    # the command line writes the frame of the default camera: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round
    # the last bit). That camera looks level at the object from z = 2: the mirror rays of the case's floor, 0.3 under the object, pass below
    # all of its density, so this part raises the floor to just under the object's base plate
    scene = _write_scene(tmp_path, hybrid, RAISED_FLOOR_CENTER, "raised")
    shots = {}
    for strength in (None, 1.0, 4.0):
        tb = _testbed(pyngp, scene, camera=False)
        tb.mesh_reflection = strength is not None
        if strength is not None:
            tb.mesh_reflection_strength = strength
        shots[strength] = tb.render(W, H, 1, True)
        del tb

    def as_png(frame):
        a = np.clip(frame[..., 3:4], 0, 1)
        v = np.clip(np.where(a > 0, frame[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
        srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
        return np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)

    expect = {k: as_png(v) for k, v in shots.items()}
    print("command line: the flag changes %d of %d pixels of the file, at strength 4 %d" % ((expect[1.0] != expect[None]).any(-1).sum(), W * H, (expect[4.0] != expect[None]).any(-1).sum()))
    assert (expect[4.0] != expect[None]).any(-1).sum() > 20
    exe = pkg("build").build_main()
    for strength in (4.0, 1.0, None):
        out = tmp_path / ("shot%s.png" % strength)
        flags = [] if strength is None else ["--mesh_reflection"] + ([] if strength == 1.0 else ["--mesh_reflection_strength", str(strength)])
        res = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "Shade", "--width", str(W), "--height", str(H), "--screenshot", str(out)] + flags,
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        png = np.asarray(Image.open(out)).astype(np.int64)
        assert png.shape == (H, W, 4) and np.abs(png - expect[strength]).max() <= 1 and (png != expect[strength]).mean() < 0.01, (strength, np.abs(png - expect[strength]).max(), (png != expect[strength]).mean())
        assert (png[..., 3] > 0).sum() > 100
