"""What the inserted meshes change in the ambient light on the NeRF, on the GPU (include/ngp_hip.h, "ambient"): the identities the contract
promises as bytes, the stage entry and the frame's record against the float64 restatement, the colour against the restated composite as
bytes, the effect, and the structure around it: determinism, samples, shards, devices, streams, statistics, the compute path and the
bindings. Tolerances: ambient_change_cases.ratio's `allow` (derived there from the lookup's own allowance) with its tie rule; none comes
from the code under test. The measured figures are in DESIGN 3.17.

n, the NeRF's own premultiplied pixel, is read from a second context as in test_nerf_mesh_shadow_gpu.py: the same model without meshes, its
render box set to the box the meshes give the first one, rendered in Geometry mode."""
import subprocess

import numpy as np
import pytest

from conftest import pkg

import ambient_change_cases as ac
import mesh_volume_cases as mv
import nerf_mesh_shadow_cases as nc
from test_nerf_mesh_shadow_gpu import RICH, _load, _opts, _pixel_offset, _same, _testbed, _tiles, _write_scene

pytestmark = pytest.mark.gpu

W, H = nc.WIDTH, nc.HEIGHT
SHADOW = dict(strength=nc.STRENGTH, bias=nc.BIAS)
BOX = (ac.LO, ac.HI)


def _cam(native, w=W, h=H, **kw):
    return native.make_camera(nc.CAMERA, w, h, nc.FOCAL, **kw)


def _render(c, native, change, shadow=None, cam=None, **kw):
    c.set_ambient_change_on_nerf(change)
    c.set_mesh_shadow_on_nerf(shadow)
    try:
        return c.render(cam or _cam(native), _opts(native, **kw), want_depth=True)
    finally:
        c.set_ambient_change_on_nerf(None)
        c.set_mesh_shadow_on_nerf(None)


def _set_case_volumes(c):
    after, before, _ = ac.volumes()
    c.set_irradiance_volume(mv.as_grid(after, ac.RES), BOX, ac.N_U, ac.N_V)
    c.set_reference_irradiance_volume(mv.as_grid(before, ac.RES), BOX, ac.N_U, ac.N_V)


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF over the floor and under the plate, the default geometry options, the case's two volumes"""
    c = native.Context(0)
    c.set_model(scene_unit)
    _load(c, nc.scene())
    c.set_geometry_opts()
    _set_case_volumes(c)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare(gpu_ctx, native):
    """the meshes alone"""
    c = native.Context(0)
    _load(c, nc.scene())
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames(hybrid, bare, native, scene_unit):
    """the frames of the case's view: both options off, the ambient change on (with its record, statistics and time), the meshes' shadow on,
    both on (with both records), the meshes alone (m), the model alone inside the meshes' box (n, with what the depth test culls taken out)"""
    cam = _cam(native)
    off = _render(hybrid, native, None)
    off_stats = hybrid.render_stats()
    hybrid.set_ambient_change_on_nerf(True)
    on = hybrid.render(cam, _opts(native), want_depth=True)
    record = hybrid.frame_ambient_change(W * H).reshape(H, W, 12)
    on_stats, ms = hybrid.render_stats(), hybrid.frame_ambient_change_ms()
    hybrid.set_mesh_shadow_on_nerf(SHADOW)
    both = hybrid.render(cam, _opts(native), want_depth=True)
    both_record = hybrid.frame_ambient_change(W * H).reshape(H, W, 12)
    both_shadow = hybrid.frame_mesh_shadow(W * H).reshape(H, W, 4)
    hybrid.set_ambient_change_on_nerf(None)
    shadow = hybrid.render(cam, _opts(native), want_depth=True)
    hybrid.set_mesh_shadow_on_nerf(None)
    lo, hi = hybrid.mesh_info()["aabb"]
    alone = native.Context(0)
    try:
        alone.set_model(dict(scene_unit, render_aabb=(tuple(float(x) for x in lo), tuple(float(x) for x in hi))))
        nerf = alone.render(cam, _opts(native), want_depth=True)
    finally:
        alone.close()
    m, m_depth = bare.render(cam, _opts(native), want_depth=True)
    behind = m_depth >= np.float32(0.01)
    n = np.where((behind & (nerf[1] > m_depth))[..., None], np.float32(0), nerf[0])  # what the depth test culls never reaches the frame
    unknown = (nerf[0][..., 3] > 0) & (nerf[0][..., 3] <= np.float32(nc.OWNER_ALPHA)) & behind  # (test_nerf_mesh_shadow_gpu.py: the cull cannot be read from these frames)
    return dict(off=off, on=on, record=record, off_stats=off_stats, on_stats=on_stats, ms=ms, both=both, both_record=both_record, both_shadow=both_shadow, shadow=shadow, m=m,
                m_depth=m_depth, n=n, unknown=unknown, behind=behind)


# ------------------------------------------------------------------------------------------------------- identities as bytes
def test_identities_as_bytes(hybrid, bare, frames, native, scene_unit):
    """off after on; NeRF mode, the G-buffer render modes, a context of meshes alone, Geometry mode without meshes and a model without
    density: each is the option-off frame, colour and depth. The option on is not, and its depth is."""
    off, on = frames["off"], frames["on"]
    assert (off[0][..., 3] > 0).sum() > 500 and on[0].tobytes() != off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
    assert _same(_render(hybrid, native, None), off)  # off after on
    assert hybrid.ambient_change_on_nerf() is None
    for mode in (native.RENDER_SHADE, native.RENDER_AO, native.RENDER_POSITIONS, native.RENDER_DEPTH, native.RENDER_COST, native.RENDER_NORMALS):
        kw = dict(testbed_mode=native.MODE_NERF, mode=mode)
        a, b = _render(hybrid, native, True, **kw), _render(hybrid, native, None, **kw)
        assert _same(a, b) and (a[0][..., 3] > 0).sum() > 300, mode
        with pytest.raises(RuntimeError, match="ran no ambient change pass"):
            hybrid.frame_ambient_change(W * H)
        assert hybrid.frame_ambient_change_ms() == 0
    assert _same(_render(bare, native, True), (frames["m"], frames["m_depth"]))  # no model (and no volume asked for: the option is ignored)
    with pytest.raises(RuntimeError, match="ran no ambient change pass"):
        bare.frame_ambient_change(W * H)
    hybrid.clear_meshes()
    try:
        assert _same(_render(hybrid, native, True), _render(hybrid, native, None))  # Geometry mode without meshes
    finally:
        _load(hybrid, nc.scene())
    empty = native.Context(0)
    try:
        empty.set_model(dict(scene_unit, density_grid=np.zeros_like(scene_unit["density_grid"])))
        _load(empty, nc.scene())
        empty.set_geometry_opts()
        _set_case_volumes(empty)
        a, b = _render(empty, native, True), _render(empty, native, None)
        assert _same(a, b) and (a[0][..., 3] > 0).sum() > 500
    finally:
        empty.close()


@pytest.mark.parametrize("mode", ["Shade", "ShadeEnvMap", "ShadeGridEnvMap", "ShadeIrradianceVolume"])
def test_equal_volumes_give_the_option_off_frame(mode, hybrid, native):
    """the reference = the context's own records: g = 1 exactly on every owner, so the frame is the option-off frame as bytes in each shade
    mode, with geometry options that put every term of the BRDF to work; with the meshes' shadow on the NeRF on as well it is that
    option's own frame, as bytes. The record says state 2 and g = (1, 1, 1) on every owner."""
    after, before, _ = ac.volumes()
    hybrid.set_geometry_opts(**RICH)
    try:
        hybrid.set_reference_irradiance_volume(mv.as_grid(after, ac.RES), BOX, ac.N_U, ac.N_V)
        if mode == "ShadeEnvMap":
            hybrid.compute_envmap(n_theta=16, n_phi=8)
        elif mode == "ShadeGridEnvMap":
            hybrid.compute_envmap_grid(2, 2, 16, 8)
        kw = dict(mode={"Shade": native.RENDER_SHADE, "ShadeEnvMap": native.RENDER_SHADE_ENVMAP, "ShadeGridEnvMap": native.RENDER_SHADE_GRID_ENVMAP}.get(mode, native.RENDER_SHADE_IRRADIANCE_VOLUME))
        off, shadow = _render(hybrid, native, None, **kw), _render(hybrid, native, None, SHADOW, **kw)
        hybrid.set_ambient_change_on_nerf(True)
        same = hybrid.render(_cam(native), _opts(native, **kw), want_depth=True)
        rec = hybrid.frame_ambient_change(W * H)
        hybrid.set_ambient_change_on_nerf(None)
        owner = rec[:, 3] != 0
        assert (off[0][..., 3] > 0).sum() > 500 and np.unique(off[0][..., 0]).size > 100 and owner.sum() >= 200
        assert np.all(rec[owner, 3] == 2) and np.all(rec[owner, 8:11] == 1) and np.all(rec[owner, 7] == rec[owner, 11]) and np.all(rec[owner, 7] > 0)
        assert _same(same, off)
        assert shadow[0].tobytes() != off[0].tobytes() and _same(_render(hybrid, native, True, SHADOW, **kw), shadow)
    finally:
        _set_case_volumes(hybrid)
        hybrid.set_geometry_opts()


def test_missing_volumes_and_wide_models_are_refused(hybrid, native, scene_unit):
    """a frame with the option on names the volume it misses; a Frequency model is refused for this option; the option off renders"""
    try:
        hybrid.clear_reference_irradiance_volume()
        with pytest.raises(RuntimeError, match="no reference irradiance volume"):
            hybrid.reference_irradiance_volume()
        with pytest.raises(RuntimeError, match="need the reference irradiance volume"):
            _render(hybrid, native, True)
        with pytest.raises(RuntimeError, match="no reference irradiance volume"):
            hybrid.irradiance_volume_ratio(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))
        _set_case_volumes(hybrid)
        hybrid.clear_irradiance_volume()
        with pytest.raises(RuntimeError, match="need the irradiance volume"):
            _render(hybrid, native, True)
        with pytest.raises(RuntimeError, match="no irradiance volume"):
            hybrid.irradiance_volume_ratio(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))
        assert hybrid.reference_irradiance_volume()[1].shape == (4, 4, 4, 28)  # (clearing the volume leaves the reference alone)
    finally:
        _set_case_volumes(hybrid)
    for p, n, message in ((np.float32([[np.nan, 0, 0]]), np.float32([[0, 0, 1]]), "position 0 is not finite"), (np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), "normal 0 is zero or not finite"),
                          (np.zeros((1, 3), np.float32), np.float32([[np.inf, 0, 0]]), "normal 0 is zero or not finite")):
        with pytest.raises(RuntimeError, match=message):
            hybrid.irradiance_volume_ratio(p, n)
    with pytest.raises(RuntimeError, match="invalid ambient change descriptor"):
        hybrid.irradiance_volume_ratio(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32), max_gain=0.5)
    wide = native.Context(0)
    try:
        wide.set_model(pkg("synthetic").make_scene(aabb_scale=1, seed=7, cfg=pkg("scene").frequency_network_config()))
        _load(wide, nc.scene())
        wide.set_geometry_opts()
        _set_case_volumes(wide)
        with pytest.raises(RuntimeError, match="need a grid-encoded model"):
            _render(wide, native, True)
        assert (_render(wide, native, None)[0][..., 3] > 0).sum() > 500
    finally:
        wide.close()


# ---------------------------------------------------------------------------------------------------------------- the stage
@pytest.mark.parametrize("name", ["case", "varying"])
def test_stage_entry_matches_the_float64_ratio(name, gpu_ctx, native):
    """ngp_irradiance_volume_ratio at random points inside and outside the box with random normals: the state is exact, |dg| <= allow, on
    every point that is not a tie case; at most TIE_CAP of the points are"""
    after, before, _ = ac.volumes()
    a, b, res, lo, hi = (after, before, ac.RES, ac.LO, ac.HI) if name == "case" else ac.varying_pair()
    c = native.Context(0)
    try:
        c.set_irradiance_volume(mv.as_grid(a, res), (lo, hi))
        c.set_reference_irradiance_volume(mv.as_grid(b, res), (lo, hi))
        p, n = ac.stage_points(res, lo, hi)
        got = c.irradiance_volume_ratio(p, n)
        same = native.Context(0)
        try:  # equal records: 1 exactly, whatever the normal
            same.set_irradiance_volume(mv.as_grid(a, res), (lo, hi))
            same.set_reference_irradiance_volume(mv.as_grid(a, res), (lo, hi))
            assert np.all(same.irradiance_volume_ratio(p, n)[:, :3] == 1)
        finally:
            same.close()
    finally:
        c.close()
    r = ac.ratio(a, b, res, lo, hi, p, n)
    keep = ~r["tie"]
    err = np.abs(got[:, :3].astype(np.float64) - r["g"])
    worst = (err[keep] / np.maximum(r["allow"][keep], 1e-300)).max()
    print("\n%s: %d points, ties %d, state 1 on %d, capped %d, g = 1 by the floor %d; largest |dg| %.3g, largest |dg| / allowed %.3g (where the allowance is 0: largest |dg| %.3g)"
          % (name, p.shape[0], r["tie"].sum(), (r["state"] == 1).sum(), (r["g"] == ac.MAX_GAIN).sum(), ((r["E_b"] <= ac.MIN_IRRADIANCE) & (r["state"] == 2)[:, None]).sum(), err[keep].max(), worst,
             err[keep][r["allow"][keep] == 0].max() if (r["allow"][keep] == 0).any() else 0.0))
    assert r["tie"].mean() <= ac.TIE_CAP
    assert np.array_equal(got[keep, 3], r["state"][keep])
    assert np.all(err[keep] <= r["allow"][keep])


# ---------------------------------------------------------------------------------------------------------------- the record
def test_record_owners_and_points_are_the_shadow_pass_own(frames):
    """with both options on, the owners and p of the ambient record equal what frame_mesh_shadow gives, as bytes; the record of the frame
    with the ambient change alone is the same; every other entry is zero"""
    rec, both, sh = frames["record"], frames["both_record"], frames["both_shadow"]
    owner = sh[..., 3] != 0
    assert owner.sum() >= 200 and np.array_equal(rec[..., 3] != 0, owner) and np.all(rec[~owner] == 0) and np.isfinite(rec).all()
    assert rec[..., :3].tobytes() == sh[..., :3].tobytes() and rec.tobytes() == both.tobytes()
    assert set(np.unique(rec[..., 3])) <= {0.0, 1.0, 2.0}
    assert np.array_equal(owner, frames["n"][..., 3] > np.float32(nc.OWNER_ALPHA))


def test_record_normals_are_the_density_gradient_stage(hybrid, frames, scene_unit):
    """N of the record against ngp_density_gradient at the warped recorded p through the mesh-export rule: the same arithmetic on the same
    input, so bytes"""
    rec = frames["record"].reshape(-1, 12)
    owner = rec[:, 3] != 0
    lo, hi = np.float32(scene_unit["aabb"][0]), np.float32(scene_unit["aabb"][1])
    diag = (hi - lo).astype(np.float32)
    w = ((rec[owner, :3] - lo).astype(np.float32) / diag).astype(np.float32)
    grad = hybrid.density_gradient(w)
    N, ok = ac.normals_from_gradient(grad, diag)
    dev = np.abs(rec[owner, 4:7].astype(np.float64) - N).max()
    print("\n%d owners, gradient lengths %.3g .. %.3g, normals without a length %d; largest |N - rule(ngp_density_gradient)| %.3g; equal as bytes: %s"
          % (owner.sum(), np.linalg.norm(grad, axis=1).min(), np.linalg.norm(grad, axis=1).max(), (~ok).sum(), dev, rec[owner, 4:7].tobytes() == N.tobytes()))
    assert ok.all() and np.all(rec[owner, 3] == 2)
    assert np.abs(np.linalg.norm(rec[owner, 4:7].astype(np.float64), axis=1) - 1).max() < 1e-6
    assert rec[owner, 4:7].tobytes() == N.tobytes()


def test_record_ratio_matches_float64_from_the_recorded_point_and_normal(frames):
    """g, the state and the weights of the record against the float64 restatement from the recorded (p, N), with the stage test's tolerance
    and tie rule. In this case no clamp or dead corner occurs: only the face and weight rules can leave a pixel out."""
    rec = frames["record"].reshape(-1, 12)
    owner = rec[:, 3] != 0
    r = ac.case_ratio(rec[owner, :3], rec[owner, 4:7])
    keep = ~r["tie"]
    g = rec[owner, 8:11].astype(np.float64)
    err = np.abs(g - r["g"])
    print("\n%d owners, left out %d; g %.3f .. %.3f; a channel under 0.9 on %.1f %%; largest |dg| %.3g, / allowed %.3g; W_after %.3f .. %.3f"
          % (owner.sum(), r["tie"].sum(), g.min(), g.max(), 100 * (g.min(1) < 0.9).mean(), err[keep].max(), (err[keep] / r["allow"][keep]).max(), rec[owner, 7].min(), rec[owner, 7].max()))
    assert r["tie"].mean() <= ac.TIE_CAP and np.all(r["state"] == 2) and np.all(r["E_b"] > 100 * ac.MIN_IRRADIANCE) and r["g"].max() < ac.MAX_GAIN
    assert np.array_equal(rec[owner, 3][keep], r["state"][keep])
    assert np.all(err[keep] <= r["allow"][keep])
    assert np.abs(rec[owner, 7] - r["W_a"])[keep].max() < 1e-5 and np.abs(rec[owner, 11] - r["W_b"])[keep].max() < 1e-5
    assert (g.min(1) < 0.9).mean() >= 0.30 and g.max() - g.min() >= 0.2  # the case's conditions, on the GPU's own record


# ---------------------------------------------------------------------------------------------------------------- the colour
def test_colour_is_the_restated_composite(frames):
    """on every pixel whose depth cull is decidable the frame is fl(fl(n g) f) + m (1 - a) as bytes, g (and f) from the records: with the
    ambient change alone (f = 1) and with the meshes' shadow on the NeRF as well; g = 1 and f = 1 give the option-off frame"""
    rec, n, m, known = frames["record"], frames["n"], frames["m"], ~frames["unknown"]
    g = np.where((rec[..., 3] == 2)[..., None], rec[..., 8:11], np.float32(1)).astype(np.float32)
    one = np.ones(g.shape[:2], np.float32)
    f = np.where(frames["both_shadow"][..., 3] == 2, np.float32(1) - np.float32(nc.STRENGTH), np.float32(1)).astype(np.float32)
    want, want_both = ac.composite(n, m, g, one), ac.composite(n, m, g, f)
    over_floor = frames["behind"] & known & (n[..., 3] > 0) & (rec[..., 3] == 2)
    print("\nowners %d, of them over the floor %d, under the meshes' shadow %d; left out %d (alpha <= 0.2 over the floor); equal as bytes: ambient %d, both %d of %d pixels"
          % ((rec[..., 3] != 0).sum(), over_floor.sum(), ((f != 1) & (rec[..., 3] == 2)).sum(), (~known).sum(), (frames["on"][0] == want).all(-1)[known].sum(), (frames["both"][0] == want_both).all(-1)[known].sum(), known.sum()))
    assert over_floor.sum() >= 50 and ((f != 1) & (rec[..., 3] == 2)).sum() >= 20
    assert frames["on"][0][known].tobytes() == want[known].tobytes()
    assert frames["both"][0][known].tobytes() == want_both[known].tobytes()
    assert ac.composite(n, m, np.ones_like(g), one)[known].tobytes() == frames["off"][0][known].tobytes()
    assert ac.composite(n, m, np.ones_like(g), f)[known].tobytes() == frames["shadow"][0][known].tobytes()
    not_owner = rec[..., 3] == 0
    assert frames["on"][0][not_owner].tobytes() == frames["off"][0][not_owner].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the effect
def test_owners_change_and_nothing_else_does(frames):
    """the test that fails without the option: at least 30 % of the owners change colour, none gets brighter than max_gain times its colour
    (here none gets brighter at all: every g < 1), alpha and depth are the option-off frame's, and so are the statistics"""
    (off, off_depth), (on, on_depth), rec = frames["off"], frames["on"], frames["record"]
    owner = rec[..., 3] != 0
    changed = (on != off).any(-1)
    print("\nowners %d, changed %d (%.1f %%); mean rgb sum on owners off %.4f, on %.4f; statistics on %s" % (owner.sum(), changed[owner].sum(), 100 * changed[owner].mean(), off[..., :3].sum(-1)[owner].mean(),
                                                                                                          on[..., :3].sum(-1)[owner].mean(), frames["on_stats"]))
    assert changed[owner].mean() >= 0.30 and not changed[~owner].any()
    assert np.all(on[..., :3] <= np.float32(ac.MAX_GAIN) * off[..., :3]) and np.all(on <= off)
    assert on[..., 3].tobytes() == off[..., 3].tobytes() and on_depth.tobytes() == off_depth.tobytes()
    assert frames["both"][1].tobytes() == off_depth.tobytes() and frames["both"][0][..., 3].tobytes() == off[..., 3].tobytes()
    for k in ("n_rays", "n_rays_alive_after_init", "n_rays_hit", "n_samples"):
        assert frames["on_stats"][k] == frames["off_stats"][k], k
    assert frames["off_stats"]["n_samples"] > 0
    assert np.isfinite(frames["ms"]) and frames["ms"] > 0


# ----------------------------------------------------------------------------------------------------------------- structure
def test_two_runs_give_the_same_bytes(hybrid, frames, native):
    hybrid.set_ambient_change_on_nerf(True)
    try:
        again = hybrid.render(_cam(native), _opts(native), want_depth=True)
        assert _same(again, frames["on"]) and hybrid.frame_ambient_change(W * H).tobytes() == frames["record"].tobytes()
        with pytest.raises(RuntimeError, match="n_pixels"):
            hybrid.frame_ambient_change(W * H - 1)
    finally:
        hybrid.set_ambient_change_on_nerf(None)
    _render(hybrid, native, None)
    assert hybrid.frame_ambient_change_ms() == 0
    with pytest.raises(RuntimeError, match="ran no ambient change pass"):
        hybrid.frame_ambient_change(W * H)


def test_two_samples_per_pixel(hybrid, native):
    """2 spp with jittered samples: every sample is scaled at its own point and the record is the last sample's, which is the record of the
    one-sample frame of that sample index"""
    cam = _cam(native, snap=False)
    off = _render(hybrid, native, None, cam=cam, spp=2)
    hybrid.set_ambient_change_on_nerf(True)
    try:
        on = hybrid.render(cam, _opts(native, spp=2), want_depth=True)
        rec2 = hybrid.frame_ambient_change(W * H)
        last = hybrid.render(_cam(native, snap=False, spp_index=1), _opts(native), want_depth=True)
        rec_last = hybrid.frame_ambient_change(W * H)
        hybrid.render(cam, _opts(native))
        rec_first = hybrid.frame_ambient_change(W * H)
    finally:
        hybrid.set_ambient_change_on_nerf(None)
    assert rec2.tobytes() == rec_last.tobytes() and rec2.tobytes() != rec_first.tobytes()
    assert on[0].tobytes() != off[0].tobytes() and on[1].tobytes() == off[1].tobytes() and np.all(on[0] <= off[0])
    owner = rec2[:, 3] != 0
    p64 = nc.surface_points(last[1], pixel_offset=tuple(float(x) for x in _pixel_offset(native, 1)))
    assert owner.sum() >= 200 and np.abs(rec2[:, :3].astype(np.float64) - p64)[owner].max() < 1e-5


def test_shards_and_packed_shards_cover_the_frame(hybrid, native):
    """three shards in image layout and tile-packed (60 x 44: partial tiles on both axes) against the whole frame: colour, depth and the
    record, as bytes"""
    import torch

    w, h, world = 60, 44, 3
    cam = _cam(native, w=w, h=h)
    tile, slot = _tiles(w, h)
    hybrid.set_ambient_change_on_nerf(True)
    try:
        full, full_depth = hybrid.render(cam, _opts(native), want_depth=True)
        full_rec = hybrid.frame_ambient_change(w * h).reshape(h, w, 12)
        assert (full_rec[..., 3] == 2).sum() > 200 and (full[..., 3] > 0).sum() > 500
        total, total_depth, total_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        packed, packed_depth, packed_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        for r in range(world):
            mine = tile % world == r
            part, part_depth = hybrid.render(cam, _opts(native, shard_index=r, shard_count=world), want_depth=True)
            rec = hybrid.frame_ambient_change(w * h).reshape(h, w, 12)
            assert not np.any(part[~mine]) and not np.any(rec[~mine])
            total[mine], total_depth[mine], total_rec[mine] = part[mine], part_depth[mine], rec[mine]
            n = native.load_library().ngp_packed_tiles(w, h, r, world) * 64
            rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
            hybrid.render_device(cam, _opts(native, shard_index=r, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
            rec = hybrid.frame_ambient_change(n)  # (synchronises the context's stream)
            src = (tile // world) * 64 + slot
            packed[mine], packed_depth[mine], packed_rec[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]], rec[src[mine]]
    finally:
        hybrid.set_ambient_change_on_nerf(None)
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes() and total_rec.tobytes() == full_rec.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes() and packed_rec.tobytes() == full_rec.tobytes()


def test_two_devices_render_the_one_device_frame(frames, native, scene_unit):
    """a context of two devices (the same ordinal twice): the option and both volumes reach the replica with the geometry, each device scales
    its share, the frame is the one-device frame as bytes; the record is the primary's tile-packed share; a cleared reference reaches it too"""
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        _load(multi, nc.scene())
        multi.set_geometry_opts()
        _set_case_volumes(multi)
        assert _same(_render(multi, native, None), frames["off"])
        multi.set_ambient_change_on_nerf(True)
        two = multi.render(_cam(native), _opts(native), want_depth=True)
        assert _same(two, frames["on"])
        n = native.load_library().ngp_packed_tiles(W, H, 0, 2) * 64
        rec = multi.frame_ambient_change(n)
        tile, slot = _tiles(W, H)
        mine = tile % 2 == 0
        assert rec[((tile // 2) * 64 + slot)[mine]].tobytes() == frames["record"][mine].tobytes()
        multi.set_mesh_shadow_on_nerf(SHADOW)
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), frames["both"])
        multi.set_mesh_shadow_on_nerf(None)
        multi.clear_reference_irradiance_volume()
        with pytest.raises(RuntimeError, match="need the reference irradiance volume"):
            multi.render(_cam(native), _opts(native))
        multi.set_ambient_change_on_nerf(None)
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), frames["off"])  # and off reaches it too
    finally:
        multi.close()


def test_frame_on_a_callers_stream(hybrid, frames, native):
    """ngp_render_device on a caller's stream, then the caller's own synchronise: the same bytes"""
    import torch

    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    hybrid.set_ambient_change_on_nerf(True)
    try:
        hybrid.render_device(_cam(native), _opts(native), rgba.data_ptr(), dep.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert rgba.cpu().numpy().tobytes() == frames["on"][0].tobytes() and dep.cpu().numpy().tobytes() == frames["on"][1].tobytes()
        assert hybrid.frame_ambient_change(W * H).tobytes() == frames["record"].tobytes()
    finally:
        hybrid.set_ambient_change_on_nerf(None)
    assert _same(_render(hybrid, native, None), frames["off"])  # (back on the context's own stream)


# ----------------------------------------------------------------------------------------------------------- the compute path
def test_compute_path(native, scene_unit):
    """compute_reference_irradiance_volume and compute_irradiance_volume on the case with (3, 3, 3) probes and 8 x 8 rays: the reference's
    records equal an occlude_by_meshes = 0 compute_irradiance_volume on a second context, as bytes, whatever occlusion its own descriptor
    would ask for; the context's own volume is untouched by the reference call; g in the frame follows from the records read back"""
    res = (3, 3, 3)
    c, other = native.Context(0), native.Context(0)
    try:
        for x in (c, other):
            x.set_model(scene_unit)
            _load(x, nc.scene())
            x.set_geometry_opts()
        c.compute_irradiance_volume(res, BOX, 8, 8)
        own = c.get_irradiance_volume()[1]
        c.compute_reference_irradiance_volume(res, BOX, 8, 8)
        d, ref = c.reference_irradiance_volume()
        assert c.get_irradiance_volume()[1].tobytes() == own.tobytes()
        other.compute_irradiance_volume(res, BOX, 8, 8, occlude_by_meshes=False)
        assert ref.tobytes() == other.get_irradiance_volume()[1].tobytes() and ref.tobytes() != own.tobytes()
        assert tuple(d.res) == res and (d.sh.n_u, d.sh.n_v, d.sh.occlude_by_meshes) == (8, 8, 0)
        c.set_ambient_change_on_nerf(True)
        on = c.render(_cam(native), _opts(native), want_depth=True)
        rec = c.frame_ambient_change(W * H)
        c.set_ambient_change_on_nerf(None)
        off = c.render(_cam(native), _opts(native), want_depth=True)
    finally:
        c.close()
        other.close()
    owner = rec[:, 3] != 0
    r = ac.ratio(own.reshape(-1, 28), ref.reshape(-1, 28), res, ac.LO, ac.HI, rec[owner, :3], rec[owner, 4:7])
    keep = ~r["tie"]
    err = np.abs(rec[owner, 8:11].astype(np.float64) - r["g"])
    print("\ntraced volumes: %d owners, left out %d, state 2 on %d; g %.3f .. %.3f; largest |dg| %.3g, / allowed %.3g; pixels changed %d"
          % (owner.sum(), r["tie"].sum(), (rec[owner, 3] == 2).sum(), r["g"].min(), r["g"].max(), err[keep].max(), (err[keep] / np.maximum(r["allow"][keep], 1e-300)).max(), (on[0] != off[0]).any(-1).sum()))
    assert owner.sum() >= 200 and np.array_equal(rec[owner, 3][keep], r["state"][keep])
    assert np.all(err[keep] <= r["allow"][keep])
    assert on[1].tobytes() == off[1].tobytes() and on[0].tobytes() != off[0].tobytes()


# ------------------------------------------------------------------------------------------------------------------ bindings
def test_pyngp_and_command_line(tmp_path, hybrid, native):
    """testbed.ambient_change_on_nerf computes the volumes the context lacks (8^3 probes over the render box, the reference with the same
    descriptor) and gives the native frame with those volumes, as bytes; --ambient_change_on_nerf writes the frame the property gives, to
    the 8 bits of the file"""
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    scene = _write_scene(tmp_path, hybrid)
    cam = _cam(native)
    tb = _testbed(pyngp, scene)
    assert tb.ambient_change_on_nerf is False and tb.ambient_change_on_nerf_min_irradiance == np.float32(1e-3) and tb.ambient_change_on_nerf_max_gain == 4.0
    tb.irradiance_volume_res = 3
    tb.irradiance_volume_sun = True  # (traced alone, V_0 over a black background is the same with and without meshes above the floor: the sun's bounce off them is what changes)
    off = tb.render(W, H, 1, True)
    tb.ambient_change_on_nerf = True
    on = tb.render(W, H, 1, True)  # (computes both volumes)
    tb.ambient_change_on_nerf_max_gain = 1.0
    capped = tb.render(W, H, 1, True)
    tb.ambient_change_on_nerf = False
    assert tb.render(W, H, 1, True).tobytes() == off.tobytes()
    vol = tb.get_irradiance_volume()  # the default volume the first on frame computed: 3^3 probes over the render box, 32 x 32 rays, the meshes occluding and sunlit
    assert vol["sh"].shape == (3, 3, 3, 28)
    own = tb.compute_reference_irradiance_volume([2, 2, 2])
    assert own["sh"].shape == (2, 2, 2, 28) and np.isfinite(own["sh"]).all()
    del tb
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        assert c.render(cam, _opts(native)).tobytes() == off.tobytes()
        c.set_irradiance_volume(vol["sh"], vol["aabb"], 32, 32)
        c.compute_reference_irradiance_volume((3, 3, 3), vol["aabb"], 32, 32)  # the Testbed's own: the volume's descriptor, nothing occluding
        c.set_ambient_change_on_nerf(True)
        assert c.render(cam, _opts(native)).tobytes() == on.tobytes()
        assert c.frame_ambient_change_ms() > 0
        c.set_ambient_change_on_nerf(dict(max_gain=1.0))
        assert c.render(cam, _opts(native)).tobytes() == capped.tobytes()
    finally:
        c.close()
    changed = np.abs(on - off).max(-1) > 0
    print("\npyngp: ambient_change_on_nerf changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(on - off).max()))
    assert (on[..., 3] > 0).sum() > 500 and changed.sum() > 100
    # the command line writes the frame of the default camera: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit)
    shots = {}
    for change in (False, True):
        tb = _testbed(pyngp, scene, camera=False)
        tb.ambient_change_on_nerf = change
        tb.irradiance_volume_sun = True
        shots[change] = tb.render(W, H, 1, True)
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
    for change in (True, False):
        out = tmp_path / ("shot%d.png" % change)
        r = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "Shade", "--width", str(W), "--height", str(H), "--screenshot", str(out)]
                           + (["--ambient_change_on_nerf", "--irradiance_volume_sun"] if change else []), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        png = np.asarray(Image.open(out)).astype(np.int64)
        assert png.shape == (H, W, 4) and np.abs(png - expect[change]).max() <= 1 and (png != expect[change]).mean() < 0.01, (change, np.abs(png - expect[change]).max(), (png != expect[change]).mean())
        assert (png[..., 3] > 0).sum() > 100
