"""Bounces on the GPU (include/ngp_hip.h, "bounces"): one pass ray by ray against the float64 reference, its records against the projection
of its own rays, equality as bytes wherever the contract promises it, the bounced volume against the stage entry applied by hand, the
light a floor throws back, and the lifetime rules, frames, pyngp and the command line. Tolerances: irradiance_bounce_reference.py's
docstring and test_irradiance_volume.py's projection bound; none comes from the code under test."""
import numpy as np
import pytest

from conftest import pkg

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import irradiance_visibility_reference as vr
import mesh_cases as mc
import mesh_reference as mref
import mesh_visibility_cases as vc
import mesh_volume_cases as mv
from irradiance_volume_cases import GEN_POINTS, UNSAFE_CAP, gen_meshes
from test_irradiance_visibility_gpu import NO_VISIBILITY, NO_VOLUME, SLAB_CAMERA, _load, _many_probes, _opts, _set_volume, _small_scene, _testbed, _wall_and_floor, _write_slab_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx, native):
    """meshes only, a context of this module's own"""
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF and, per test, meshes"""
    c = native.Context(0)
    c.set_model(scene_unit)
    yield c
    c.close()


def _hold_stage_volume(c, visible):
    sh, res, lo, hi = br.stage_volume()
    _set_volume(c, sh, res, lo, hi)
    if visible:
        D, maps = br.stage_maps()
        c.set_irradiance_volume_visibility(vc.as_map_grid(maps, res), D, normal_bias=br.STAGE_BIAS)


# ----------------------------------------------------------------------------------------------------------- one pass
@pytest.mark.parametrize("visible", [False, True])
def test_rays_and_records_of_one_pass(visible, ctx):
    """1. every ray's hit, distance and B against the float64 reference on safe rays; 2. the records against the float64 projection of the
    pass's own rays, within the bound of test_irradiance_volume.py::test_projection_of_the_traced_rays.
    Measured on one MI355X over the five shapes: |B - B_ref| on safe rays at most 4.4e-7 (plain) and 7.9e-7 (visible) against allowances of
    4.9e-5 to 5.2e-5, |dt| at most 1.4e-6, the records' |dc| at most 0.014 of their bound."""
    _load(ctx, gen_meshes())
    _hold_stage_volume(ctx, visible)
    try:
        for nu, nv in br.RAY_SHAPES:
            K, case = nu * nv, br.stage_case(nu, nv, visible)
            sh, rays = ctx.irradiance_sh_bounce(GEN_POINTS, br.STAGE_ALBEDO, nu, nv, alpha=case["alpha"], visible=visible, return_rays=True)
            assert sh.shape == (5, 28) and rays.shape == (5, K, 4) and np.isfinite(sh).all() and not np.isnan(rays).any()
            want_t, safe, t = case["hit"]["t"], case["safe"], rays[..., 3].astype(np.float64)
            assert (~safe).mean() <= UNSAFE_CAP
            assert np.array_equal(np.isinf(t)[safe], np.isinf(want_t)[safe])
            both = safe & np.isfinite(want_t)
            dt = np.abs(t[both] - want_t[both]).max() if both.any() else 0.0
            err = np.abs(rays[..., :3].astype(np.float64) - case["B"])[safe].max()
            print("\n%s %2d x %2d: safe rays %4d, with a hit %3d, |dt| %.2e, |dB| %.2e (allowed %.2e, of it the float32 form x %g: %.2e), largest B %.3f"
                  % ("visible" if visible else "plain  ", nu, nv, safe.sum(), both.sum(), dt, err, case["allow"], mc.GPU_FACTOR, mc.GPU_FACTOR * case["dev"], case["B"].max()))
            assert dt < mref.TIE_EPS, dt
            assert err <= case["allow"], (err, case["allow"])
            assert np.all(rays[..., :3][np.isinf(t)] == 0)
            # 2. the records of these rays
            want = sh_ref.project(rays[..., :3], sh_ref.sphere_dirs(nu, nv)).reshape(5, 27)
            bound = 1e-5 * (4 * np.pi / K) * np.abs(rays[..., :3].astype(np.float64)).sum(1)  # (5, 3): per channel
            dc = np.abs(sh[:, :27].astype(np.float64) - want).reshape(5, 9, 3)
            print("        records: max |dc| = %.3e, max |dc| / bound = %.3f, max |c| = %.3f" % (dc.max(), (dc / np.maximum(bound[:, None, :], 1e-30)).max(), np.abs(want).max()))
            assert np.all(dc <= bound[:, None, :])
            assert np.array_equal(sh[:, 27], np.isinf(t).mean(1).astype(np.float32))
        if visible:  # the maps are in the numbers
            plain = ctx.irradiance_sh_bounce(GEN_POINTS, br.STAGE_ALBEDO, 16, 16, alpha=case["alpha"])
            assert np.abs(plain - sh).max() > 1e-3
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()


def test_a_pass_is_deterministic_and_independent_of_the_split(ctx):
    """3. run to run, 5 probes in one call against 2 + 3 (five probes: two workgroups of the projection, the second with one live wave;
    5 x 81 rays: no multiple of a workgroup of the ray kernel), with both lookups"""
    _load(ctx, gen_meshes())
    try:
        for visible in (False, True):
            _hold_stage_volume(ctx, visible)
            for nu, nv in ((9, 9), (16, 16)):
                alpha = br.stage_alpha(5, nu * nv)
                one = ctx.irradiance_sh_bounce(GEN_POINTS, br.STAGE_ALBEDO, nu, nv, alpha=alpha, visible=visible, return_rays=True)
                two = ctx.irradiance_sh_bounce(GEN_POINTS, br.STAGE_ALBEDO, nu, nv, alpha=alpha, visible=visible, return_rays=True)
                a = ctx.irradiance_sh_bounce(GEN_POINTS[:2], br.STAGE_ALBEDO, nu, nv, alpha=alpha[:2], visible=visible, return_rays=True)
                b = ctx.irradiance_sh_bounce(GEN_POINTS[2:], br.STAGE_ALBEDO, nu, nv, alpha=alpha[2:], visible=visible, return_rays=True)
                for k in (0, 1):
                    assert one[k].tobytes() == two[k].tobytes() and one[k].tobytes() == np.concatenate([a[k], b[k]]).tobytes()
                assert np.abs(one[0][:, :27]).max() > 1e-2
                # no alpha is alpha 0, and occlusion off is no bounce
                assert ctx.irradiance_sh_bounce(GEN_POINTS, br.STAGE_ALBEDO, nu, nv, visible=visible).tobytes() == \
                    ctx.irradiance_sh_bounce(GEN_POINTS, br.STAGE_ALBEDO, nu, nv, alpha=np.zeros_like(alpha), visible=visible).tobytes()
                off, off_rays = ctx.irradiance_sh_bounce(GEN_POINTS, br.STAGE_ALBEDO, nu, nv, alpha=alpha, visible=visible, occlude_by_meshes=False, return_rays=True)
                assert np.all(off[:, :27] == 0) and np.all(off[:, 27] == 1) and np.all(off_rays[..., :3] == 0) and np.all(np.isinf(off_rays[..., 3]))
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()


@pytest.mark.parametrize("visible", [False, True])
def test_a_pass_over_two_host_chunks(visible, ctx):
    """600 probes x 64 x 64 rays (a host chunk of 512 whole probes and a tail of 88, see _many_probes), each ray with an alpha of its own:
    every probe's record and every ray from the one call is the bytes of the same probe asked for in calls of 100 probes (one chunk each). A
    probe's result does not depend on which probes share its launch, so the small calls are the reference. The stage volume was made for
    other meshes; here it is only a source of numbers (the last asserts see to it that light does come back in both chunks)."""
    _load(ctx, _small_scene())
    _hold_stage_volume(ctx, visible)
    try:
        probes, alpha = _many_probes(), br.stage_alpha(600, 64 * 64)
        sh, rays = ctx.irradiance_sh_bounce(probes, br.STAGE_ALBEDO, 64, 64, alpha=alpha, visible=visible, return_rays=True)
        assert sh.shape == (600, 28) and rays.shape == (600, 4096, 4) and np.isfinite(sh).all() and not np.isnan(rays).any()
        for i in range(0, 600, 100):
            s = slice(i, i + 100)
            part_sh, part_rays = ctx.irradiance_sh_bounce(probes[s], br.STAGE_ALBEDO, 64, 64, alpha=alpha[s], visible=visible, return_rays=True)
            assert np.array_equal(sh[s], part_sh) and np.array_equal(rays[s], part_rays), i
        for chunk in (slice(0, 512), slice(512, 600)):  # (light comes back in both chunks, and some rays of both see the sky)
            assert np.abs(sh[chunk, :27]).max() > 1e-2 and np.isinf(rays[chunk, :, 3]).any() and np.isfinite(rays[chunk, :, 3]).any()
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()


# ------------------------------------------------------------------------------------------------------ the bounced volume
def _volume(c):
    return c.get_irradiance_volume()[1].reshape(-1, 28)


def test_no_source_leaves_the_records_alone(hybrid):
    """3. N = 0, a black albedo, and no meshes give ngp_compute_irradiance_volume's records as bytes"""
    res, lo, hi, nu, nv = br.E2E_CASE
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        v0 = _volume(hybrid)
        assert ((v0[:, 27] > 0) & (v0[:, 27] < 1)).any() and np.abs(v0[:, :3]).max() > 1e-2
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=2, albedo=0.0)
        assert _volume(hybrid).tobytes() == v0.tobytes()
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=2, albedo=br.E2E_ALBEDO, occlude_by_meshes=False)
        free = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, occlude_by_meshes=False)
        assert _volume(hybrid).tobytes() == free.tobytes()
        d = hybrid._volume_desc(res, (lo, hi), hybrid._sh_desc(nu, nv, True, 0.01))  # N = 0 reaches the entry through the C ABI alone
        hybrid._check(hybrid.L.ngp_compute_irradiance_volume_bounced(hybrid.h, _byref(d), _byref(hybrid._bounce_desc(0, 0.5)), None))
        assert _volume(hybrid).tobytes() == v0.tobytes()
        hybrid.clear_meshes()
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        bare = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=3, albedo=br.E2E_ALBEDO)
        assert _volume(hybrid).tobytes() == bare.tobytes() and bare.tobytes() != v0.tobytes()
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


def _byref(x):
    import ctypes

    return ctypes.byref(x)


def _step(c, v0, positions, nu, nv, alpha, visible=False):
    """V_0 + one stage pass from the volume the context holds, in float32; float 27 V_0's"""
    r = c.irradiance_sh_bounce(positions, br.E2E_ALBEDO, nu, nv, alpha=alpha, visible=visible)
    out = v0.copy()
    out[:, :27] = v0[:, :27] + r[:, :27]
    assert np.array_equal(r[:, 27], v0[:, 27])  # (the same rays against the same meshes)
    return out


def test_bounced_volume_is_the_stage_applied_by_hand(hybrid):
    """4. N = 1 is V_0 + a stage pass from V_0 with the trace's own alpha, N = 2 the same step from V_1, as bytes; with a visibility
    descriptor the passes look the volume up through the maps ngp_compute_irradiance_volume_visibility gives this lattice, and those stay"""
    res, lo, hi, nu, nv = br.E2E_CASE
    positions = vr.probe_positions(res, lo, hi)
    vis = dict(n_u=8, n_v=8, sharpness_log2=4, max_distance=0.0, normal_bias=0.01)
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        v0 = _volume(hybrid)
        _, traced = hybrid.irradiance_sh_traced(positions, nu, nv, return_rays=True)
        alpha = traced[..., 3]
        assert (alpha > 0.05).any() and (alpha < 0.95).any()  # the NeRF is in front of some hits
        v1 = _step(hybrid, v0, positions, nu, nv, alpha)
        _set_volume(hybrid, v1, res, lo, hi)
        v2 = _step(hybrid, v0, positions, nu, nv, alpha)
        assert np.abs(v1[:, :27] - v0[:, :27]).max() > 1e-3 and np.abs(v2[:, :27] - v1[:, :27]).max() > 1e-5
        for n, want in ((1, v1), (2, v2)):
            hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=n, albedo=br.E2E_ALBEDO)
            got = _volume(hybrid)
            assert got.tobytes() == want.tobytes(), (n, np.abs(got - want).max())
            assert np.array_equal(got[:, 27], v0[:, 27])
            with pytest.raises(RuntimeError, match=NO_VISIBILITY):  # (the bounced compute drops what was held, like the plain one)
                hybrid.get_irradiance_volume_visibility()
            hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=n, albedo=br.E2E_ALBEDO)  # (and run to run)
            assert _volume(hybrid).tobytes() == want.tobytes()
        # through the visibility
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        hybrid.compute_irradiance_volume_visibility(**vis)
        d0, maps = hybrid.get_irradiance_volume_visibility()
        w1 = _step(hybrid, v0, positions, nu, nv, alpha, visible=True)
        _set_volume(hybrid, w1, res, lo, hi)
        hybrid.set_irradiance_volume_visibility(maps, d0.max_distance, d0.sharpness_log2, d0.normal_bias)
        w2 = _step(hybrid, v0, positions, nu, nv, alpha, visible=True)
        assert w1.tobytes() != v1.tobytes()
        for n, want in ((1, w1), (2, w2)):
            hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=n, albedo=br.E2E_ALBEDO, visibility=vis)
            assert _volume(hybrid).tobytes() == want.tobytes()
            d, held = hybrid.get_irradiance_volume_visibility()
            assert held.tobytes() == maps.tobytes()
            assert (d.n_u, d.n_v, d.sharpness_log2, d.max_distance, d.normal_bias) == (d0.n_u, d0.n_v, d0.sharpness_log2, d0.max_distance, d0.normal_bias)
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


def test_a_floor_throws_light_back(hybrid):
    """5. under a point above a floor, E for the down-facing normal grows with one bounce, by no more than albedo x the largest E the floor
    itself receives (the irradiance of a radiance below X is below pi X, and the floor's radiance is below albedo E / pi)"""
    albedo, res, lo, hi, nu, nv = br.FLOOR_CASE
    _load(hybrid, br.floor_scene())
    try:
        p, down = np.float32([[0.5, 0.05, 0.5], [0.3, 0.1, 0.6]]), np.float32([[0, -1, 0], [0, -1, 0]])
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        before = hybrid.irradiance_volume_at(p, down)
        g = np.linspace(0.0, 1.0, 41, dtype=np.float32)
        floor = np.stack([np.repeat(g, 41), np.full(41 * 41, br.normalised(br.floor_scene())[0][..., 1].max(), np.float32), np.tile(g, 41)], 1)
        received = hybrid.irradiance_volume_at(floor, np.tile(np.float32([[0, 1, 0]]), (floor.shape[0], 1)))[:, :3].max(0)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=1, albedo=albedo)
        after = hybrid.irradiance_volume_at(p, down)
        gain = (after - before)[:, :3]
        print("\nE(down) %s -> %s; the floor receives at most %s" % (before[0, :3], after[0, :3], received))
        assert np.all(received > 1e-3)
        assert np.all(gain > 0) and np.all(gain <= albedo * received), (gain, albedo * received)
        assert np.array_equal(after[:, 3], before[:, 3])
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# --------------------------------------------------------------------------------------------- lifetime, frames, bindings
def test_frames_devices_and_other_modes(hybrid, native, scene_unit):
    """6. a bounced volume (with visibility: one change of the held data) reaches the replicas of a multi-device context in one step: the
    ShadeIrradianceVolume frame is the same bytes on two devices and on one, and differs from the frame without bounces; Shade and
    ShadeGridEnvMap frames do not see it. The scene is the visibility tests' wall and floor beside the NeRF's box, seen from above; the
    volume's probes are the corners of that box."""
    res, box, nu, nv = (2, 2, 2), (np.float32([0, 0, 0]), np.float32([1, 1, 1])), 16, 16
    cam = native.make_camera(SLAB_CAMERA, mc.WIDTH, mc.HEIGHT, (100.0, 100.0))
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        frames = {}
        for c in (hybrid, multi):
            _load(c, _wall_and_floor())
            c.set_geometry_opts()
        hybrid.set_geometry_opts(ambientcolor=mv.SKY_AMBIENT)
        hybrid.compute_envmap_grid(2, 2, 16, 8)
        modes = (native.RENDER_SHADE, native.RENDER_SHADE_GRID_ENVMAP)
        hybrid.compute_irradiance_volume(res, box, nu, nv)
        others = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
        hybrid.set_geometry_opts()
        for key, kw in (("plain", {}), ("bounced", dict(bounces=1, albedo=0.64)), ("visible", dict(bounces=1, albedo=0.64, visibility=dict(n_u=8, n_v=8)))):
            for c in (hybrid, multi):
                c.compute_irradiance_volume(res, box, nu, nv, **kw)
            one, one_depth = hybrid.render(cam, _opts(native), want_depth=True)
            two, two_depth = multi.render(cam, _opts(native), want_depth=True)
            assert (one[..., 3] > 0).sum() > 500
            assert one.tobytes() == two.tobytes() and one_depth.tobytes() == two_depth.tobytes(), key
            frames[key] = one
        assert len({f.tobytes() for f in frames.values()}) == 3
        changed = np.abs(frames["bounced"] - frames["plain"]).max(-1) > 0
        print("\none bounce changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(frames["bounced"] - frames["plain"]).max()))
        assert changed.sum() > 100
        hybrid.set_geometry_opts(ambientcolor=mv.SKY_AMBIENT)
        held = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
        for (a, ad), (b, bd) in zip(held, others):
            assert (a[..., 3] > 0).sum() > 500 and a.tobytes() == b.tobytes() and ad.tobytes() == bd.tobytes()
    finally:
        multi.close()
        hybrid.set_geometry_opts()
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


def test_refusals(hybrid, native):
    res, lo, hi, nu, nv = br.E2E_CASE
    one = np.float32([[0.5, 0.5, 0.5]])
    c = native.Context(0)
    try:
        with pytest.raises(RuntimeError, match="No network"):
            c.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=1, albedo=0.5)
        with pytest.raises(RuntimeError, match=NO_VOLUME):
            c.irradiance_sh_bounce(one, 0.5, 4, 4)
        _hold_stage_volume(c, False)
        with pytest.raises(RuntimeError, match=NO_VISIBILITY):
            c.irradiance_sh_bounce(one, 0.5, 4, 4, visible=True)
        assert c.irradiance_sh_bounce(np.zeros((0, 3), np.float32), 0.5, 4, 4).shape == (0, 28)
        for kw, message in ((dict(n_u=0), "n_u and n_v"), (dict(n_u=2048, n_v=2048), "too large")):
            with pytest.raises(RuntimeError, match=message):
                c.irradiance_sh_bounce(one, 0.5, **kw)
        with pytest.raises(RuntimeError, match="position 0 is not finite"):
            c.irradiance_sh_bounce(np.float32([[0.5, np.nan, 0.5]]), 0.5, 4, 4)
        for bad in (np.nan, np.inf):
            alpha = np.zeros((1, 16), np.float32)
            alpha[0, 7] = bad
            with pytest.raises(RuntimeError, match="alpha 7 is not finite"):
                c.irradiance_sh_bounce(one, 0.5, 4, 4, alpha=alpha)
        for bad in (1.5, -0.1, np.nan):
            with pytest.raises(RuntimeError, match="albedo must be finite and in"):
                c.irradiance_sh_bounce(one, bad, 4, 4)
    finally:
        c.close()
    held = None
    try:
        hybrid.clear_meshes()
        hybrid.compute_irradiance_volume(res, (lo, hi), 4, 4)
        held = _volume(hybrid)
        bad = [(dict(bounces=17, albedo=0.5), "n_bounces must be at most 16"), (dict(bounces=1, albedo=1.5), "albedo"), (dict(bounces=1, albedo=(0.1, np.nan, 0.1)), "albedo"),
               (dict(bounces=1, albedo=0.5, n_u=0), "n_u and n_v"), (dict(bounces=1, albedo=0.5, visibility=dict(sharpness_log2=7)), "sharpness_log2"),
               (dict(bounces=1, albedo=0.5, visibility=dict(normal_bias=-1.0)), "normal_bias"), (dict(bounces=1, albedo=0.5, visibility=dict(n_u=0)), "n_u and n_v")]
        for kw, message in bad:
            with pytest.raises(RuntimeError, match=message):
                hybrid.compute_irradiance_volume(res, (lo, hi), **dict(dict(n_u=4, n_v=4), **kw))
        with pytest.raises(RuntimeError, match="resolution"):
            hybrid.compute_irradiance_volume((2, 0, 2), (lo, hi), 4, 4, bounces=1, albedo=0.5)
        assert _volume(hybrid).tobytes() == held.tobytes()  # the failed calls left the held volume alone
    finally:
        hybrid.clear_irradiance_volume()


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    """the Testbed's keyword and its default albedo (the base colour squared), irradiance_volume_bounces for the default volume of a
    ShadeIrradianceVolume render, and --irradiance_volume_bounces"""
    import subprocess
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    hybrid.clear_meshes()
    scene = _write_slab_scene(tmp_path, hybrid)
    w, h = mc.WIDTH, mc.HEIGHT
    cam = native.make_camera(SLAB_CAMERA, w, h, (100.0, 100.0))
    tb = _testbed(pyngp, scene)
    assert tb.irradiance_volume_bounces == 0
    off = tb.render(w, h, 1, True)
    v0 = tb.get_irradiance_volume()
    box = (np.float32(v0["aabb"][0]), np.float32(v0["aabb"][1]))
    vol = tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, bounces=2)
    own = tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, bounces=2, albedo=[0.9, 0.5, 0.1])
    with pytest.raises(RuntimeError, match="n_bounces must be at most 16"):
        tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, bounces=17)
    del tb
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, bounces=2)
        assert c.get_irradiance_volume()[1].tobytes() == vol["sh"].tobytes() and vol["sh"].tobytes() != v0["sh"].tobytes()
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, bounces=2, albedo=(0.9, 0.5, 0.1))
        assert c.get_irradiance_volume()[1].tobytes() == own["sh"].tobytes() and own["sh"].tobytes() != vol["sh"].tobytes()
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, bounces=1)
        direct = c.render(cam, _opts(native))
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, bounces=1, visibility={})
        direct_visible = c.render(cam, _opts(native))
    finally:
        c.close()
    frames = {}
    for visibility in (False, True):
        tb = _testbed(pyngp, scene, visibility=visibility)
        tb.irradiance_volume_bounces = 1
        frames[visibility] = tb.render(w, h, 1, True)
        assert tb.render(w, h, 1, True).tobytes() == frames[visibility].tobytes()
        del tb
    on = frames[False]
    changed = np.abs(on - off).max(-1) > 0
    print("\npyngp: irradiance_volume_bounces = 1 changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(on - off).max()))
    assert (off[..., 3] > 0).sum() > 500 and changed.sum() > 100
    assert on.tobytes() == direct.tobytes() and frames[True].tobytes() == direct_visible.tobytes() and frames[True].tobytes() != on.tobytes()
    # the command line writes that frame: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit)
    tb = _testbed(pyngp, scene, camera=False)
    tb.irradiance_volume_bounces = 1
    want = tb.render(w, h, 1, True)
    del tb
    exe = pkg("build").build_main()
    out = tmp_path / "shot.png"
    r = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "ShadeIrradianceVolume", "--irradiance_volume_res", "2", "--irradiance_volume_bounces", "1", "--width", str(w),
                        "--height", str(h), "--screenshot", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    png = np.asarray(Image.open(out)).astype(np.int64)
    a = np.clip(want[..., 3:4], 0, 1)
    v = np.clip(np.where(a > 0, want[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
    srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
    expect = np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)
    assert png.shape == (h, w, 4) and np.abs(png - expect).max() <= 1 and (png != expect).mean() < 0.01, (np.abs(png - expect).max(), (png != expect).mean())
    assert (png[..., 3] > 0).sum() > 100
