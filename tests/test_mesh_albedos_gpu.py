"""Mesh albedos on the GPU (include/ngp_hip.h, "mesh albedos"): off is off as bytes; a per-mesh run against two uniform runs ray by ray as
bytes, with the float64 reference naming the run; B against the composed float64 reference; determinism and chunking; the colour a red
torus lays on its surroundings, without a tolerance; the no-source rules; the volume against the stage entries applied by hand; frames and
devices; pyngp and the command line. Tolerances: mesh_albedo_cases.py's docstring and test_irradiance_volume.py's projection bound; none
comes from the code under test. The measured figures are in DESIGN 3.23."""
import json
import subprocess

import numpy as np
import pytest

from conftest import pkg

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import irradiance_sun_reference as sr
import irradiance_visibility_reference as vr
import mesh_albedo_cases as ma
import mesh_cases as mc
import mesh_material_cases as mm
import mesh_reference as mref
from irradiance_volume_cases import GEN_POINTS, gen_meshes
from test_irradiance_visibility_gpu import SLAB_CAMERA, _load, _opts, _set_volume, _testbed, _wall_and_floor, _write_slab_scene

pytestmark = pytest.mark.gpu

STAGE = (sr.STAGE_SUN, sr.STAGE_RADIANCE, sr.STAGE_BIAS)
E2E_SUN = ((1.0, 1.0, 1.0), sr.STAGE_RADIANCE, sr.STAGE_BIAS)  # the frames' default sun
NERF = (0.01, 0.0)  # min_transmittance, t_min of the sun's shadow rays
OTHER = np.float32([0.3, 0.6, 0.8])  # a call's albedo that no mesh uses
REFUSAL = r"mesh albedo must be finite and in \[0, 1\] on every channel"


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


def _own(c, albedos):
    """mesh m owns albedos[m]; None: it owns none"""
    for m, a in enumerate(albedos):
        c.set_mesh_albedo(m, a)


def _hold_stage_volume(c, visible):
    sh, res, lo, hi = br.stage_volume()
    _set_volume(c, sh, res, lo, hi)
    if visible:
        import mesh_visibility_cases as vc

        D, maps = br.stage_maps()
        c.set_irradiance_volume_visibility(vc.as_map_grid(maps, res), D, normal_bias=br.STAGE_BIAS)


def _bounce(c, albedo, nu, nv, alpha, visible, probes=GEN_POINTS):
    return c.irradiance_sh_bounce(probes, albedo, nu, nv, alpha=alpha, visible=visible, return_rays=True)


def _sun(c, albedo, nu, nv, alpha, shadowed, probes=GEN_POINTS):
    """(sh, rays) of the plain sun stage, (sh, rays, shadow) of the shadowed one"""
    if shadowed:
        return c.irradiance_sh_sun(probes, STAGE, albedo, nu, nv, alpha=alpha, return_rays=True, nerf_shadow=NERF, return_shadow=True)
    return c.irradiance_sh_sun(probes, STAGE, albedo, nu, nv, alpha=alpha, return_rays=True)


def _volume(c):
    return c.get_irradiance_volume()[1].reshape(-1, 28)


def _add(v0, r):
    """V_0 + the records of a stage pass, in float32; float 27 V_0's"""
    out = v0.copy()
    out[:, :27] = v0[:, :27] + r[:, :27]
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------- 1. off is off
def test_off_is_off_on_the_stages(ctx, hybrid):
    """a run with no mesh owning an albedo is the bytes of a run where every mesh owns the call's albedo (and the call carries another
    one): rays, records and the shadow output; the bounce with both lookups, the sun, the shadowed sun on scene_unit"""
    nu, nv = 9, 9
    alpha = br.stage_alpha(5, nu * nv)
    same = (br.STAGE_ALBEDO, br.STAGE_ALBEDO)
    _load(ctx, gen_meshes())
    _load(hybrid, gen_meshes())
    try:
        for visible in (False, True):
            _hold_stage_volume(ctx, visible)
            plain = _bounce(ctx, br.STAGE_ALBEDO, nu, nv, alpha, visible)
            _own(ctx, same)
            assert _same(_bounce(ctx, OTHER, nu, nv, alpha, visible), plain) and np.abs(plain[0][:, :27]).max() > 1e-2
            _own(ctx, (None, None))
            assert _same(_bounce(ctx, br.STAGE_ALBEDO, nu, nv, alpha, visible), plain)  # (and cleared is off again)
        plain = _sun(ctx, br.STAGE_ALBEDO, nu, nv, alpha, False)
        _own(ctx, same)
        assert _same(_sun(ctx, OTHER, nu, nv, alpha, False), plain) and np.abs(plain[0][:, :27]).max() > 1e-2
        plain = _sun(hybrid, br.STAGE_ALBEDO, nu, nv, alpha, True)
        _own(hybrid, same)
        assert _same(_sun(hybrid, OTHER, nu, nv, alpha, True), plain) and len(plain) == 3 and np.any(plain[2] != 0)
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()
        hybrid.clear_meshes()


def test_off_is_off_on_the_whole_volume(hybrid):
    """ngp_compute_irradiance_volume_sunlit_shadowed, N = 2, sun on: the records without albedos are the records with every mesh owning
    the call's"""
    res, lo, hi, nu, nv = br.E2E_CASE
    kw = dict(bounces=2, sun=E2E_SUN, sun_nerf_shadow=NERF)
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, albedo=br.E2E_ALBEDO, **kw)
        plain = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        assert _volume(hybrid).tobytes() != plain.tobytes()
        _own(hybrid, (br.E2E_ALBEDO, br.E2E_ALBEDO))
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, albedo=OTHER, **kw)
        assert _volume(hybrid).tobytes() == plain.tobytes()
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# ------------------------------------------------------------------------------------ 2. and 3. ray by ray, and against float64
def _check_selection(per, u0, u1, case, lit=None):
    """every ray's (B, t) of the per-mesh run is the A_0 run's or the A_1 run's as bytes, t is equal in all three, and on a safe ray with a
    hit (lit: that the reference lights) it is the run of the reference's mesh. Returns how many rays told the runs apart per mesh."""
    rays, r0, r1 = (x.view(np.uint32) for x in (per, u0, u1))
    assert np.array_equal(rays[..., 3], r0[..., 3]) and np.array_equal(rays[..., 3], r1[..., 3])
    is0, is1 = (rays == r0).all(-1), (rays == r1).all(-1)
    assert np.all(is0 | is1)
    told = []
    for m, (mine, other) in enumerate(((is0, is1), (is1, is0))):
        on = case["safe"] & (case["mesh"] == m)
        assert np.all(mine[on])
        if lit is not None:
            on = on & lit
        told.append(int((on & ~other).sum()))
    return told


@pytest.mark.parametrize("visible", [False, True])
def test_bounce_rays_take_their_meshes_albedo(visible, ctx):
    """2. the per-mesh run against the two uniform runs as bytes, K = 15, 64, 81, 256 (and K = 1, the tail: mesh 0 alone); a mesh without
    its own albedo under a call's A_1 is the mesh owning A_1. 3. B on safe rays against the composed float64 reference within 256 ULP of
    the source volume's largest |E| / pi + GPU_FACTOR x the composed float32 form's deviation; the records against the projection of the
    run's own rays within test_rays_and_records_of_one_pass's bound.
    Measured on one MI355X over the five shapes: |dB| at most 4.4e-7 (plain) and 6.4e-7 (visible) against allowances of 4.9e-5 to 5.2e-5,
    the nearer uniform run off by 0.48 to 1.13; the records' |dc| at most 0.014 of their bound."""
    _load(ctx, gen_meshes())
    _hold_stage_volume(ctx, visible)
    try:
        for nu, nv in br.RAY_SHAPES:
            K, case = nu * nv, ma.bounce_case(nu, nv, visible)
            alpha = case["alpha"]
            u0, u1 = _bounce(ctx, ma.A0, nu, nv, alpha, visible), _bounce(ctx, ma.A1, nu, nv, alpha, visible)
            _own(ctx, ma.ALBEDOS)
            sh, rays = _bounce(ctx, br.STAGE_ALBEDO, nu, nv, alpha, visible)
            _own(ctx, (ma.A0, None))
            assert _same(_bounce(ctx, ma.A1, nu, nv, alpha, visible), (sh, rays))
            _own(ctx, (None, None))
            told = _check_selection(rays, u0[1], u1[1], case)
            assert sh.shape == (5, 28) and rays.shape == (5, K, 4) and np.isfinite(sh).all() and not np.isnan(rays).any()
            t, want_t, safe = rays[..., 3].astype(np.float64), case["hit"]["t"], case["safe"]
            assert np.array_equal(np.isinf(t)[safe], np.isinf(want_t)[safe])
            both = safe & np.isfinite(want_t)
            assert np.abs(t[both] - want_t[both]).max() < mref.TIE_EPS
            err = np.abs(rays[..., :3].astype(np.float64) - case["B"])[safe].max()
            uniform = max(np.abs(u[1][..., :3].astype(np.float64) - case["B"])[safe].max() for u in (u0, u1))
            print("\n%s %2d x %2d: rays that tell the runs apart %s, |dB| %.2e (allowed %.2e, of it the float32 form x %g: %.2e); the nearer uniform run is off by %.3f"
                  % ("visible" if visible else "plain  ", nu, nv, told, err, case["allow"], mc.GPU_FACTOR, mc.GPU_FACTOR * case["dev"], uniform))
            assert err <= case["allow"], (err, case["allow"])
            if K > 1:
                assert min(told) >= 1 and uniform > 1000 * case["allow"]
            want = sh_ref.project(rays[..., :3], sh_ref.sphere_dirs(nu, nv)).reshape(5, 27)
            bound = 1e-5 * (4 * np.pi / K) * np.abs(rays[..., :3].astype(np.float64)).sum(1)  # (5, 3): per channel
            dc = np.abs(sh[:, :27].astype(np.float64) - want).reshape(5, 9, 3)
            print("        records: max |dc| = %.3e, max |dc| / bound = %.3f" % (dc.max(), (dc / np.maximum(bound[:, None, :], 1e-30)).max()))
            assert np.all(dc <= bound[:, None, :])
            assert np.array_equal(sh[:, 27], np.isinf(t).mean(1).astype(np.float32))
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()


@pytest.mark.parametrize("shadowed", [False, True])
def test_sun_rays_take_their_meshes_albedo(shadowed, ctx, hybrid):
    """2. as above for the sun pass, plain and with the NeRF's shadow rays (on scene_unit), K = 64, 81, 256: (B, t) as bytes from the run
    of the hit's mesh, and the shadow output (q, alpha_s) the same bytes in all three runs. 3. the plain pass's B on safe rays against the
    composed float64 reference within 256 ULP of the largest albedo x radiance / pi + GPU_FACTOR x the composed float32 form's deviation,
    its records against the projection of its own rays; the shadowed pass's B is apply(the plain per-mesh rays, its alpha_s) as bytes.
    Measured on one MI355X: |dB| at most 1.2e-7 against allowances of 1.8e-5, the nearer uniform run off by 0.62 to 0.87; the records'
    |dc| at most 0.011 of their bound; every lit safe ray of either mesh tells the runs apart, also behind the NeRF's shadow."""
    import irradiance_sun_shadow_reference as ssr

    c = hybrid if shadowed else ctx
    _load(c, gen_meshes())
    try:
        for nu, nv in ma.SUN_SHAPES:
            K, case = nu * nv, ma.sun_case(nu, nv)
            alpha, safe, lit = case["alpha"], case["safe"], case["info"]["lit"]
            u0, u1 = _sun(c, ma.A0, nu, nv, alpha, shadowed), _sun(c, ma.A1, nu, nv, alpha, shadowed)
            _own(c, ma.ALBEDOS)
            per = _sun(c, br.STAGE_ALBEDO, nu, nv, alpha, shadowed)
            plain = per if not shadowed else _sun(c, br.STAGE_ALBEDO, nu, nv, alpha, False)
            _own(c, (ma.A0, None))
            assert _same(_sun(c, ma.A1, nu, nv, alpha, shadowed), per)
            _own(c, (None, None))
            sh, rays = per[0], per[1]
            told = _check_selection(rays, u0[1], u1[1], case, lit & (alpha < 1))
            assert told[0] >= 1 and (shadowed or told[1] >= 1), told  # (the NeRF may stand in front of mesh 1's two or so lit rays)
            B = rays[..., :3]
            assert np.all(B[safe & ~lit] == 0)
            if shadowed:
                print("\n%2d x %2d shadowed: lit rays that tell the runs apart %s" % (nu, nv, told))
                assert per[2].tobytes() == u0[2].tobytes() and per[2].tobytes() == u1[2].tobytes()
                assert np.array_equal(B, ssr.apply(plain[1][..., :3], per[2][..., 3])) and np.array_equal(rays[..., 3], plain[1][..., 3])
                continue
            err = np.abs(B.astype(np.float64) - case["B"])[safe].max()
            uniform = max(np.abs(u[1][..., :3].astype(np.float64) - case["B"])[safe].max() for u in (u0, u1))
            print("\n%2d x %2d: lit rays that tell the runs apart %s, |dB| %.2e (allowed %.2e, of it the float32 form x %g: %.2e); the nearer uniform run is off by %.3f"
                  % (nu, nv, told, err, case["allow"], mc.GPU_FACTOR, mc.GPU_FACTOR * case["dev"], uniform))
            assert err <= case["allow"] and uniform > 1000 * case["allow"], (err, case["allow"], uniform)
            want = sh_ref.project(B, sh_ref.sphere_dirs(nu, nv)).reshape(5, 27)
            bound = 1e-5 * (4 * np.pi / K) * np.abs(B.astype(np.float64)).sum(1)
            dc = np.abs(sh[:, :27].astype(np.float64) - want).reshape(5, 9, 3)
            print("        records: max |dc| = %.3e, max |dc| / bound = %.3f" % (dc.max(), (dc / np.maximum(bound[:, None, :], 1e-30)).max()))
            assert np.all(dc <= bound[:, None, :])
    finally:
        c.clear_meshes()


# ------------------------------------------------------------------------------------------------------------ 4. determinism
def test_per_mesh_passes_are_deterministic_and_independent_of_the_split(ctx, hybrid):
    """run to run, and 5 probes in one call against 2 + 3 (5 x 81 rays: no multiple of a workgroup of the ray kernel), as bytes: the
    bounce with both lookups, the sun, the shadowed sun"""
    nu, nv = 9, 9
    alpha = br.stage_alpha(5, nu * nv)
    _load(ctx, gen_meshes())
    _load(hybrid, gen_meshes())
    try:
        _own(ctx, ma.ALBEDOS)
        _own(hybrid, ma.ALBEDOS)
        runs = [lambda p, a: _sun(ctx, OTHER, nu, nv, a, False, p), lambda p, a: _sun(hybrid, OTHER, nu, nv, a, True, p)]
        for visible in (False, True):
            runs.append(lambda p, a, visible=visible: (_hold_stage_volume(ctx, visible), _bounce(ctx, OTHER, nu, nv, a, visible, p))[1])
        for run in runs:
            one, two = run(GEN_POINTS, alpha), run(GEN_POINTS, alpha)
            a, b = run(GEN_POINTS[:2], alpha[:2]), run(GEN_POINTS[2:], alpha[2:])
            assert _same(one, two) and _same(one, [np.concatenate([x, y]) for x, y in zip(a, b)])
            assert np.abs(one[0][:, :27]).max() > 1e-2
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()
        hybrid.clear_meshes()


# -------------------------------------------------------------------------------------------------- 5. channels are independent
@pytest.mark.parametrize("n_bounces", [1, 2])
def test_a_red_torus_takes_green_and_blue_away(n_bounces, hybrid):
    """the colour bleed without a tolerance: the floor (0.8, 0.8, 0.8) and the torus (0.8, 0.1, 0.1) against a uniform 0.8 on the e2e_scene
    volume, sun on. The red coefficients of every record are equal as bytes. Green and blue: every ray's B is not greater, so the
    coefficient of the constant harmonic (Y_0 > 0 everywhere) is not greater on any probe, and it is smaller on every probe with the torus
    among its safe hits. (The other eight harmonics change sign over the sphere: a darker torus below a probe RAISES its coefficient of y,
    so no order holds for them, and none is asserted.)
    Measured on one MI355X: all 12 probes have the torus in sight; the constant harmonic's green and blue fall by 3.5e-4 to 0.555 (N = 1)
    and by 3.5e-3 to 0.557 (N = 2)."""
    res, lo, hi, nu, nv = br.E2E_CASE
    hit, mesh = ma.e2e_hits()
    sees_torus = ((mesh == 1) & ~hit["unsafe"]).any(1)
    assert sees_torus.sum() >= 2
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=n_bounces, albedo=0.8, sun=E2E_SUN)
        uniform = _volume(hybrid)
        _own(hybrid, ((0.8, 0.8, 0.8), (0.8, 0.1, 0.1)))
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=n_bounces, albedo=0.8, sun=E2E_SUN)
        red_torus = _volume(hybrid)
        u, r = uniform[:, :27].reshape(-1, 9, 3), red_torus[:, :27].reshape(-1, 9, 3)
        assert u[..., 0].tobytes() == r[..., 0].tobytes() and np.array_equal(uniform[:, 27], red_torus[:, 27])
        drop = u[:, 0, 1:] - r[:, 0, 1:]
        print("\nN = %d: probes with the torus in sight %d of %d; the constant harmonic's green and blue fall by %.3g to %.3g there, by at most %.3g elsewhere"
              % (n_bounces, sees_torus.sum(), sees_torus.size, drop[sees_torus].min(), drop[sees_torus].max(), drop[~sees_torus].max() if (~sees_torus).any() else 0.0))
        assert np.all(r[:, 0, 1:] <= u[:, 0, 1:])
        assert np.all(r[sees_torus][:, 0, 1:] < u[sees_torus][:, 0, 1:])
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# ------------------------------------------------------------------------------------------------------- 6. no-source rules
def test_no_source_rules_over_the_resolved_albedos(hybrid):
    """a black call's albedo with the torus owning A_1 runs the passes; every resolved albedo black gives V_0's bytes, whatever the call's"""
    res, lo, hi, nu, nv = br.E2E_CASE
    box, black = (lo, hi), (0.0, 0.0, 0.0)
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, box, nu, nv)
        v0 = _volume(hybrid)
        for kw in (dict(bounces=2), dict(bounces=0, sun=E2E_SUN), dict(bounces=1, sun=E2E_SUN, sun_nerf_shadow=NERF)):
            _own(hybrid, (None, ma.A1))
            hybrid.compute_irradiance_volume(res, box, nu, nv, albedo=0.0, **kw)
            lit = _volume(hybrid)
            assert lit.tobytes() != v0.tobytes() and np.array_equal(lit[:, 27], v0[:, 27]), kw
            _own(hybrid, (None, black))
            hybrid.compute_irradiance_volume(res, box, nu, nv, albedo=0.0, **kw)
            assert _volume(hybrid).tobytes() == v0.tobytes(), kw
            _own(hybrid, (black, black))
            hybrid.compute_irradiance_volume(res, box, nu, nv, albedo=br.E2E_ALBEDO, **kw)
            assert _volume(hybrid).tobytes() == v0.tobytes(), kw
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# ------------------------------------------------------------------------------- 7. the volume is the stage applied by hand
@pytest.mark.parametrize("shadowed", [False, True])
def test_per_mesh_volume_is_the_stages_applied_by_hand(shadowed, hybrid):
    """N = 1 and N = 2, sun on, the floor owning A_0 and the torus A_1: the held records are V_0 + the sun stage with the trace's own
    alpha (S), then S + the bounce stage from S, then S + the bounce stage from that, as bytes; plain and with the sun's shadow rays"""
    res, lo, hi, nu, nv = br.E2E_CASE
    positions = vr.probe_positions(res, lo, hi)
    nerf = NERF if shadowed else None
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        v0 = _volume(hybrid)
        _, traced = hybrid.irradiance_sh_traced(positions, nu, nv, return_rays=True)
        alpha = traced[..., 3]
        uniform_S = _add(v0, hybrid.irradiance_sh_sun(positions, E2E_SUN, OTHER, nu, nv, alpha=alpha, nerf_shadow=nerf))
        _own(hybrid, ma.ALBEDOS)
        S = _add(v0, hybrid.irradiance_sh_sun(positions, E2E_SUN, OTHER, nu, nv, alpha=alpha, nerf_shadow=nerf))
        _set_volume(hybrid, S, res, lo, hi)
        v1 = _add(S, hybrid.irradiance_sh_bounce(positions, OTHER, nu, nv, alpha=alpha))
        _set_volume(hybrid, v1, res, lo, hi)
        v2 = _add(S, hybrid.irradiance_sh_bounce(positions, OTHER, nu, nv, alpha=alpha))
        assert np.abs(S[:, :27] - v0[:, :27]).max() > 1e-3 and np.abs(S - uniform_S).max() > 1e-3
        assert np.abs(v1[:, :27] - S[:, :27]).max() > 1e-3 and np.abs(v2[:, :27] - v1[:, :27]).max() > 1e-5
        for n, want in ((0, S), (1, v1), (2, v2)):
            hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=n, albedo=OTHER, sun=E2E_SUN, sun_nerf_shadow=nerf)
            got = _volume(hybrid)
            assert got.tobytes() == want.tobytes(), (n, np.abs(got - want).max())
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# ------------------------------------------------------------------------------------------------------ 8. frames and devices
def test_frames_and_devices(hybrid, native, scene_unit):
    """a Shade frame, and one with every mesh owning a material, are the same bytes with and without albedos; a ShadeIrradianceVolume frame of
    the per-mesh volume differs from the uniform volume's on mesh pixels; on two devices the held volume is the one device's as bytes, and so
    is the frame. The scene is the visibility tests' wall and floor beside the NeRF's box, seen from above."""
    res, box, nu, nv = (2, 2, 2), (np.float32([0, 0, 0]), np.float32([1, 1, 1])), 16, 16
    kw = dict(bounces=1, albedo=0.64, sun=E2E_SUN)
    cam = native.make_camera(SLAB_CAMERA, mc.WIDTH, mc.HEIGHT, (100.0, 100.0))
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        for c in (hybrid, multi):
            _load(c, _wall_and_floor())
            c.set_geometry_opts()

        def frames():
            shade = hybrid.render(cam, _opts(native, mode=native.RENDER_SHADE), want_depth=True)
            hybrid.set_mesh_material(0, mm.FLOOR)
            hybrid.set_mesh_material(1, mm.PLATE)
            materials = hybrid.render(cam, _opts(native, mode=native.RENDER_SHADE), want_depth=True)
            hybrid.set_mesh_material(0, None)
            hybrid.set_mesh_material(1, None)
            hybrid.compute_irradiance_volume(res, box, nu, nv, **kw)
            return shade + materials, hybrid.render(cam, _opts(native), want_depth=True)

        plain, plain_volume = frames()
        uniform = _volume(hybrid)
        for c in (hybrid, multi):
            _own(c, ma.ALBEDOS)
        with_albedos, per_mesh_volume = frames()
        assert _same(plain, with_albedos) and plain[0].tobytes() != plain[2].tobytes() and (plain[0][..., 3] > 0).sum() > 500
        assert hybrid.mesh_albedo(0) == tuple(float(x) for x in ma.A0)  # (set_mesh_material left it alone on the device context too)
        changed = np.abs(per_mesh_volume[0] - plain_volume[0]).max(-1) > 0
        print("\nthe meshes' albedos change %d of %d pixels of the ShadeIrradianceVolume frame, by at most %.3g" % (changed.sum(), changed.size, np.abs(per_mesh_volume[0] - plain_volume[0]).max()))
        assert changed.sum() > 100 and np.all(plain_volume[0][..., 3][changed] > 0) and per_mesh_volume[1].tobytes() == plain_volume[1].tobytes()
        held = _volume(hybrid)
        assert held.tobytes() != uniform.tobytes()
        multi.compute_irradiance_volume(res, box, nu, nv, **kw)
        assert _volume(multi).tobytes() == held.tobytes()
        two = multi.render(cam, _opts(native), want_depth=True)
        assert _same(two, per_mesh_volume)
    finally:
        multi.close()
        hybrid.set_geometry_opts()
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# --------------------------------------------------------------------------------------------------------------- 9. bindings
def test_refusals_on_a_device(hybrid):
    """every refusal of the setter and the getter, and of a call whose per-mesh source is refused like the descriptor's; each leaves the
    albedos and the held volume alone"""
    res, lo, hi, nu, nv = br.E2E_CASE
    _load(hybrid, br.e2e_scene())
    try:
        _own(hybrid, (ma.A0, None))
        hybrid.compute_irradiance_volume(res, (lo, hi), 4, 4, bounces=1, albedo=0.5)
        held = _volume(hybrid)
        for bad in (-1, 2):
            with pytest.raises(RuntimeError, match="mesh: index"):
                hybrid.set_mesh_albedo(bad, ma.A1)
            with pytest.raises(RuntimeError, match="mesh: index"):
                hybrid.mesh_albedo(bad)
        for rgb in ((np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -0.1), (1.5, 0.5, 0.5)):
            for mesh in (0, 1):
                with pytest.raises(RuntimeError, match=REFUSAL):
                    hybrid.set_mesh_albedo(mesh, rgb)
        # the descriptor's own checks come first and are what they were
        with pytest.raises(RuntimeError, match="albedo must be finite and in"):
            hybrid.compute_irradiance_volume(res, (lo, hi), 4, 4, bounces=1, albedo=1.5)
        with pytest.raises(RuntimeError, match="radiance must be finite"):
            hybrid.compute_irradiance_volume(res, (lo, hi), 4, 4, bounces=1, albedo=0.5, sun=((1, 1, 1), np.inf, 1e-3))
        with pytest.raises(RuntimeError, match="resolution"):
            hybrid.compute_irradiance_volume((2, 0, 2), (lo, hi), 4, 4, bounces=1, albedo=0.5)
        assert hybrid.mesh_albedo(0) == tuple(float(x) for x in ma.A0) and hybrid.mesh_albedo(1) is None
        assert _volume(hybrid).tobytes() == held.tobytes()
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


def _write_scene(tmp_path, hybrid, name, extras):
    """_write_slab_scene's files with extras[i] (a dict of further keys) on mesh entry i"""
    src = json.loads(open(_write_slab_scene(tmp_path, hybrid)).read())
    for entry, extra in zip(src["geometry"], extras):
        entry.update(extra)
    path = tmp_path / ("%s_geometry_scene.json" % name)
    path.write_text(json.dumps(src))
    return str(path)


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    """the Testbed's set / get / clear, kept across load_training_data; irradiance_volume_albedo_from_materials off is the volume without
    albedos as bytes, on it is the volume of set_mesh_albedo(material_albedo(the mesh's material)), for compute_irradiance_volume and for the
    default volume of a render, and an explicit albedo wins; --irradiance_volume_albedo_from_materials and the scene file's "albedo" give the
    volume of a Context that was handed those albedos through set_mesh_albedo, as bytes"""
    pyngp = pkg("build").import_pyngp()
    hybrid.clear_meshes()
    plate = {k: (list(v) if isinstance(v, tuple) else v) for k, v in mm.PLATE.items()}
    scene = _write_scene(tmp_path, hybrid, "plain", ({}, {}))
    w, h = mc.WIDTH, mc.HEIGHT

    def context_volume(path, albedos, n=16, **kw):
        c = native.Context(0)
        try:
            c.load_scene(path)
            c.set_geometry_opts()
            for m, a in enumerate(albedos):
                if a is not None:
                    c.set_mesh_albedo(m, a)
            c.compute_irradiance_volume((2, 2, 2), box, n, n, **kw)
            return c.get_irradiance_volume()[1]
        finally:
            c.close()

    tb = _testbed(pyngp, scene)
    assert tb.irradiance_volume_albedo_from_materials is False and tb.mesh_albedo(0) is None and tb.mesh_albedo(1) is None
    v0 = tb.compute_irradiance_volume([2, 2, 2], None, 16, 16, True)
    box = (np.float32(v0["aabb"][0]), np.float32(v0["aabb"][1]))
    plain = context_volume(scene, (None, None), bounces=1)
    assert plain.tobytes() != v0["sh"].tobytes()
    b = pyngp.Testbed.BRDFParams()
    b.basecolor, b.roughness, b.specular = list(mm.PLATE["basecolor"]), 0.8, 0.5
    tb.set_mesh_material(0, b)  # (the wall: the lattice's probes get no light back from the floor beside the box)
    assert tb.compute_irradiance_volume([2, 2, 2], None, 16, 16, True, bounces=1)["sh"].tobytes() == plain.tobytes()  # off: the material lends no albedo
    tb.irradiance_volume_albedo_from_materials = True
    from_material = tb.compute_irradiance_volume([2, 2, 2], None, 16, 16, True, bounces=1)["sh"]
    assert tb.mesh_albedo(0) is None  # (lent for the computation alone)
    want = context_volume(scene, (native.material_albedo(mm.PLATE), None), bounces=1)
    assert from_material.tobytes() == want.tobytes() and want.tobytes() != plain.tobytes()
    fresh = _testbed(pyngp, scene)  # the default volume of a render (a Testbed that holds no volume yet): 32 x 32 rays
    fresh.set_mesh_material(0, b)
    fresh.irradiance_volume_albedo_from_materials = True
    fresh.irradiance_volume_bounces = 1
    fresh.render(w, h, 1, True)
    assert fresh.get_irradiance_volume()["sh"].tobytes() == context_volume(scene, (native.material_albedo(mm.PLATE), None), 32, bounces=1).tobytes()
    assert fresh.mesh_albedo(0) is None
    del fresh
    tb.set_mesh_albedo(1, [float(x) for x in ma.A1])  # an explicit albedo wins over the material's
    tb.set_mesh_albedo(0, [float(x) for x in ma.A0])
    assert tb.mesh_albedo(1) == tuple(float(x) for x in ma.A1) and tb.mesh_albedo(0) == tuple(float(x) for x in ma.A0)
    explicit = tb.compute_irradiance_volume([2, 2, 2], None, 16, 16, True, bounces=1, sun=True)["sh"]
    sun = ([float(x) for x in tb.sun_dir], [float(x) for x in tb.irradiance_volume_sun_radiance], 1e-3)
    assert explicit.tobytes() == context_volume(scene, ma.ALBEDOS, bounces=1, sun=sun).tobytes()
    tb.clear_mesh_albedo(0)
    assert tb.mesh_albedo(0) is None and tb.mesh_albedo(1) is not None
    tb.load_training_data(scene)  # the file gives none; what the Testbed was given comes back over it
    assert tb.mesh_albedo(1) == tuple(float(x) for x in ma.A1) and tb.mesh_albedo(0) is None
    for bad in ([0.5, 1.5, 0.5], [float("nan"), 0.5, 0.5]):
        with pytest.raises(RuntimeError, match=REFUSAL):
            tb.set_mesh_albedo(0, bad)
    with pytest.raises(RuntimeError, match="mesh: index"):
        tb.set_mesh_albedo(2, [0.5, 0.5, 0.5])
    del tb
    # the command line: a file that gives the wall a material (the flag lends it the material's albedo), and one that gives it an albedo
    lent = _write_scene(tmp_path, hybrid, "lent", ({"material": plate}, {"albedo": [float(x) for x in ma.A1]}))
    given = _write_scene(tmp_path, hybrid, "given", ({"albedo": [float(x) for x in ma.A1]}, {}))
    plain = context_volume(scene, (None, None), 32, bounces=1)
    from_material = context_volume(scene, (native.material_albedo(mm.PLATE), ma.A1), 32, bounces=1)
    from_file = context_volume(scene, (ma.A1, None), 32, bounces=1)
    assert len({plain.tobytes(), from_material.tobytes(), from_file.tobytes()}) == 3
    exe = pkg("build").build_main()
    for path, flag, expect in ((lent, ["--irradiance_volume_albedo_from_materials"], from_material), (given, [], from_file), (scene, ["--irradiance_volume_albedo_from_materials"], plain)):
        out = tmp_path / "volume.bin"
        r = subprocess.run([exe, "--no-gui", "--scene", path, "--render_mode", "ShadeIrradianceVolume", "--irradiance_volume_res", "2", "--irradiance_volume_bounces", "1",
                            "--width", "32", "--height", "24", "--screenshot", str(tmp_path / "shot.png"), "--save_irradiance_volume", str(out)] + flag,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(out, np.float32)
        assert got.size == 8 * 28 and got.tobytes() == expect.tobytes(), (path, flag)
