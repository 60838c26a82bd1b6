"""The NeRF shadow of the sun pass on the GPU (include/ngp_hip.h, "sun", the *_shadowed entries): one pass ray by ray (B' against the
unshadowed entry, alpha_s against the ray-list tracer and against the oracle, q against the float64 reference), equality as bytes wherever
the contract promises it, determinism and chunking, the volume against the stage entries applied by hand, the light a shadowed floor
throws up, and frames, devices, bindings and refusals. Tolerances: the allowance rule of test_irradiance_sun_gpu.py for q and the bound of
test_irradiance_traced.py::test_caller_rays_match_oracle for alpha; none comes from the code under test. The measured figures are in
DESIGN 3.14."""
import ctypes
import subprocess

import numpy as np
import pytest

from conftest import pkg

import irradiance_bounce_reference as br
import irradiance_sun_reference as sr
import irradiance_sun_shadow_reference as ssr
import irradiance_visibility_reference as vr
import mesh_cases as mc
import mesh_reference as mref
import mesh_volume_cases as mv
from test_irradiance_sun_gpu import E2E_SUN, SUN_CAMERA, _add, _sun_testbed, _volume, _write_scene
from test_irradiance_sun_shadow_cpu import BLOCKED_SHARE, DOWN, FLOOR_SUN, OPEN_SHARE, TEST_POINTS, mix, oracle_alpha
from test_irradiance_visibility_gpu import NO_VISIBILITY, _load, _many_probes, _opts, _set_volume, _small_scene

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
NERF = (0.01, 0.0)  # min_transmittance, t_min
ALPHA_BOUND = 1e-2  # test_caller_rays_match_oracle's for scene_unit
# (name, scene, (res, lo, hi, n_u, n_v)): 8 probes x 16 x 16 over the floor; 12 probes x 8 x 8 (K = 64: one wave) over the floor and a torus
CASES = {"floor": (br.floor_scene, br.FLOOR_CASE[1:]), "e2e": (br.e2e_scene, br.E2E_CASE)}
_cache = {}


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF and, per test, meshes"""
    c = native.Context(0)
    c.set_model(scene_unit)
    yield c
    c.close()


def _case(name):
    if name not in _cache:
        scene, (res, lo, hi, nu, nv) = CASES[name]
        _cache[name] = dict(ssr.case(scene(), res, lo, hi, nu, nv, FLOOR_SUN), scene=scene(), nu=nu, nv=nv)
    return _cache[name]


def _sun(direction=FLOOR_SUN):
    return (direction, sr.STAGE_RADIANCE, sr.STAGE_BIAS)


def _mesh_box(oracle, scene):
    """the render box while these meshes are loaded: the meshes' box inflated by 4"""
    h = oracle.mesh_scene(scene)
    lo, hi = oracle.mesh_scene_aabb(h)
    oracle.mesh_scene_destroy(h)
    return lo - 4, hi + 4


# ----------------------------------------------------------------------------------------------------------- one pass
@pytest.mark.parametrize("name", ["floor", "e2e"])
def test_one_pass_ray_by_ray(name, hybrid, oracle, scene_unit):
    """(a) rays_out is apply(the unshadowed entry's rays, shadow_out's alpha_s) as bytes, t untouched; (b) alpha_s is ngp_trace_nerf_rays'
    alpha of (q_out, s^, (t_min, inf)) as bytes, and alpha_s = 0, q = 0 where the reference lights nothing; (c) on safe rays |q - q64| <=
    TIE_EPS + GPU_FACTOR x the float32 form's deviation; (d) on safe rays |alpha_s - the oracle's alpha on the reference's q| < 1e-2, and
    the floor case's mix of blocked and open rays holds on the GPU's own alpha_s"""
    c = _case(name)
    nu, nv, probes = c["nu"], c["nv"], c["probes"]
    P, K = probes.shape[0], nu * nv
    assert (P, K) == ((8, 256) if name == "floor" else (12, 64))
    alpha = br.stage_alpha(P, K)
    s_hat = sr.unit_sun(FLOOR_SUN)
    _load(hybrid, c["scene"])
    try:
        plain_sh, plain = hybrid.irradiance_sh_sun(probes, _sun(), 0.8, nu, nv, alpha=alpha, return_rays=True)
        for nerf in (NERF, (0.05, 0.25)):
            sh, rays, shadow = hybrid.irradiance_sh_sun(probes, _sun(), 0.8, nu, nv, alpha=alpha, return_rays=True, nerf_shadow=nerf, return_shadow=True)
            st = hybrid.render_stats()
            assert sh.shape == (P, 28) and rays.shape == (P, K, 4) and shadow.shape == (P, K, 4) and np.isfinite(sh).all() and np.isfinite(shadow).all()
            q, a = shadow[..., :3], shadow[..., 3]
            # (a)
            assert np.array_equal(rays[..., :3], ssr.apply(plain[..., :3], a)) and np.array_equal(rays[..., 3], plain[..., 3])
            assert np.array_equal(sh[:, 27], plain_sh[:, 27])
            # (b)
            has = np.any(q != 0, axis=-1)
            safe, lit = c["safe"], c["lit"]
            assert np.array_equal(has[safe], lit[safe]) and np.all(a[~has] == 0) and np.all(a[safe & ~lit] == 0) and np.all(q[safe & ~lit] == 0)
            n = int(has.sum())
            traced, _ = hybrid.trace_nerf_rays(q[has], np.tile(s_hat, (n, 1)), np.tile(np.float32([nerf[1], INF]), (n, 1)), nerf[0])
            assert np.array_equal(a[has], traced[:, 3])
            assert st["n_rays"] == P * K and st["n_samples"] > 0  # the shadow trace is the call the statistics report: one entry per probe ray
            assert hybrid.irradiance_sun_shadow_ms() > 0 and hybrid.irradiance_sun_ms() >= hybrid.irradiance_sun_shadow_ms()
            if nerf != NERF:
                continue
            m = safe & lit
            # (c)
            dq = np.abs(q.astype(np.float64) - c["q"])[m].max()
            allow = mref.TIE_EPS + mc.GPU_FACTOR * c["dev"]
            # (d)
            want = oracle_alpha(oracle, scene_unit, c["q"][m], FLOOR_SUN, _mesh_box(oracle, c["scene"]))
            da = np.abs(a[m] - want).max()
            blocked, open_ = mix(a[lit])
            print("\n%s: %d rays, lit %d (safe %d), alpha_s > 0.9: %d, = 0: %d, between: %d; |dq| %.2e (allowed %.2e, of it the float32 form x %g: %.2e); |dalpha| against the oracle %.2e"
                  % (name, P * K, lit.sum(), m.sum(), (a[lit] > 0.9).sum(), (a[lit] == 0).sum(), ((a[lit] > 0) & (a[lit] <= 0.9)).sum(), dq, allow, mc.GPU_FACTOR,
                     mc.GPU_FACTOR * c["dev"], da))
            hits = c["hit"]["tri"] >= 0
            assert (c["unsafe"] & hits).sum() <= 0.02 * hits.sum()
            assert dq <= allow, (dq, allow)
            assert da < ALPHA_BOUND, da
            assert (a[lit] > 0.9).any() and (a[lit] == 0).any() and (rays[..., :3] < plain[..., :3]).any()
            if name == "floor":
                assert blocked >= BLOCKED_SHARE and open_ >= OPEN_SHARE, (blocked, open_)
        # a pass without the shadow reports no shadow time
        hybrid.irradiance_sh_sun(probes, _sun(), 0.8, nu, nv)
        assert hybrid.irradiance_sun_shadow_ms() == 0
    finally:
        hybrid.clear_meshes()


# ------------------------------------------------------------------------------------------------------- identities as bytes
def test_identities_as_bytes(hybrid):
    """nerf = NULL and a t_min beyond the box are ngp_compute_irradiance_volume_sunlit; no sun, a sun without radiance, a black albedo,
    occlusion off and no meshes are ngp_compute_irradiance_volume_bounced; all through the new entry"""
    res, lo, hi, nu, nv = br.E2E_CASE
    box = (lo, hi)
    kw = dict(bounces=1, albedo=br.E2E_ALBEDO)
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, box, nu, nv, sun=E2E_SUN, **kw)
        sunlit = _volume(hybrid)
        d = hybrid._volume_desc(res, box, hybrid._sh_desc(nu, nv, True, 0.01))  # nerf = NULL reaches the entry through the C ABI alone
        hybrid._check(hybrid.L.ngp_compute_irradiance_volume_sunlit_shadowed(hybrid.h, ctypes.byref(d), ctypes.byref(hybrid._bounce_desc(1, br.E2E_ALBEDO)), None,
                                                                             ctypes.byref(hybrid._sun_desc(E2E_SUN)), None))
        assert _volume(hybrid).tobytes() == sunlit.tobytes()
        hybrid.compute_irradiance_volume(res, box, nu, nv, sun=E2E_SUN, sun_nerf_shadow=(0.01, 100.0), **kw)  # every shadow ray starts beyond the box
        assert _volume(hybrid).tobytes() == sunlit.tobytes()
        hybrid.compute_irradiance_volume(res, box, nu, nv, sun=E2E_SUN, sun_nerf_shadow=True, **kw)
        assert _volume(hybrid).tobytes() != sunlit.tobytes()  # (and the NeRF in front of the sun is in the numbers)
        probes = vr.probe_positions(res, lo, hi)
        far = hybrid.irradiance_sh_sun(probes, E2E_SUN, br.E2E_ALBEDO, nu, nv, return_rays=True, nerf_shadow=(0.01, 100.0), return_shadow=True)
        plain = hybrid.irradiance_sh_sun(probes, E2E_SUN, br.E2E_ALBEDO, nu, nv, return_rays=True)
        assert far[0].tobytes() == plain[0].tobytes() and far[1].tobytes() == plain[1].tobytes() and np.all(far[2][..., 3] == 0) and np.any(far[2][..., :3] != 0)

        hybrid.compute_irradiance_volume(res, box, nu, nv, **kw)
        bounced = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, box, nu, nv, sun_nerf_shadow=True, **kw)  # sun = NULL
        assert _volume(hybrid).tobytes() == bounced.tobytes() and bounced.tobytes() != sunlit.tobytes()
        hybrid.compute_irradiance_volume(res, box, nu, nv, sun=(E2E_SUN[0], 0.0, 1e-3), sun_nerf_shadow=True, **kw)
        assert _volume(hybrid).tobytes() == bounced.tobytes()
        hybrid.compute_irradiance_volume(res, box, nu, nv)
        v0 = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, box, nu, nv, bounces=2, albedo=0.0, sun=E2E_SUN, sun_nerf_shadow=True)
        assert _volume(hybrid).tobytes() == v0.tobytes()
        hybrid.compute_irradiance_volume(res, box, nu, nv, occlude_by_meshes=False, **kw)
        free = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, box, nu, nv, occlude_by_meshes=False, sun=E2E_SUN, sun_nerf_shadow=True, **kw)
        assert _volume(hybrid).tobytes() == free.tobytes()
        hybrid.clear_meshes()
        hybrid.compute_irradiance_volume(res, box, nu, nv, **kw)
        bare = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, box, nu, nv, sun=E2E_SUN, sun_nerf_shadow=True, **kw)
        assert _volume(hybrid).tobytes() == bare.tobytes() and bare.tobytes() != bounced.tobytes()
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# ------------------------------------------------------------------------------------------------- determinism and chunking
def _pass(c, probes, nu, nv, alpha, sun=None):
    return c.irradiance_sh_sun(probes, _sun() if sun is None else sun, 0.8, nu, nv, alpha=alpha, return_rays=True, nerf_shadow=NERF, return_shadow=True)


def test_a_shadowed_pass_is_deterministic_and_independent_of_the_split(hybrid):
    """run to run, and the floor case's 8 probes in one call against 3 + 5"""
    c = _case("floor")
    nu, nv, probes = c["nu"], c["nv"], c["probes"]
    alpha = br.stage_alpha(8, nu * nv)
    _load(hybrid, c["scene"])
    try:
        one, two = _pass(hybrid, probes, nu, nv, alpha), _pass(hybrid, probes, nu, nv, alpha)
        a, b = _pass(hybrid, probes[:3], nu, nv, alpha[:3]), _pass(hybrid, probes[3:], nu, nv, alpha[3:])
        for k in range(3):
            assert np.array_equal(one[k], two[k]) and np.array_equal(one[k], np.concatenate([a[k], b[k]])), k
        assert (one[2][..., 3] > 0.9).any() and np.abs(one[0][:, :27]).max() > 1e-2
    finally:
        hybrid.clear_meshes()


def test_a_shadowed_pass_over_two_host_chunks(hybrid):
    """600 probes x 64 x 64 rays among the 32 triangles of test_a_sun_pass_over_two_host_chunks (a host chunk of 512 whole probes and a tail
    of 88), each ray with an alpha of its own: every record, ray and shadow output of the one call equals the same probe asked for in calls
    of 100 probes. A probe's result does not depend on which probes share its launch, so the small calls are the reference."""
    _load(hybrid, _small_scene())
    try:
        probes, alpha = _many_probes(), br.stage_alpha(600, 64 * 64)
        # a sun from below: of the directions tried on 60 of these probes with the oracle, the one whose shadow rays cross the NeRF from
        # probes of both chunks (irradiance_sun_reference.STAGE_SUN's all pass beside it: alpha_s would be 0 throughout)
        sun = ((-0.2, -1.0, 0.1), sr.STAGE_RADIANCE, sr.STAGE_BIAS)
        whole = _pass(hybrid, probes, 64, 64, alpha, sun)
        assert whole[0].shape == (600, 28) and whole[1].shape == (600, 4096, 4) and whole[2].shape == (600, 4096, 4) and all(np.isfinite(w[..., :3]).all() for w in whole)
        for i in range(0, 600, 100):
            s = slice(i, i + 100)
            part = _pass(hybrid, probes[s], 64, 64, alpha[s], sun)
            assert all(np.array_equal(whole[k][s], part[k]) for k in range(3)), i
        for chunk in (slice(0, 512), slice(512, 600)):  # (shadow rays in both chunks: some blocked by the NeRF, some open, and rays without one)
            a, has = whole[2][chunk, :, 3], np.any(whole[2][chunk, :, :3] != 0, axis=-1)
            assert (a[has] > 0.5).any() and (a[has] == 0).any() and (~has).any() and np.abs(whole[0][chunk, :27]).max() > 1e-2
    finally:
        hybrid.clear_meshes()


# ------------------------------------------------------------------------------------------------------ the shadowed volume
def test_shadowed_volume_is_the_stages_applied_by_hand(hybrid):
    """as test_sunlit_volume_is_the_stages_applied_by_hand builds it, with the shadowed stage entry in the sun pass's place: N = 0 holds S =
    V_0 + the stage pass with the trace's own alpha; N = 2 continues from that S with two stage bounce passes; as bytes, plain and through a
    visibility descriptor, whose maps are ngp_compute_irradiance_volume_visibility's and stay"""
    res, lo, hi, nu, nv = br.E2E_CASE
    positions = vr.probe_positions(res, lo, hi)
    vis = dict(n_u=8, n_v=8, sharpness_log2=4, max_distance=0.0, normal_bias=0.01)
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        v0 = _volume(hybrid)
        hybrid.compute_irradiance_volume_visibility(**vis)
        d0, maps = hybrid.get_irradiance_volume_visibility()
        _, traced = hybrid.irradiance_sh_traced(positions, nu, nv, return_rays=True)
        alpha = traced[..., 3]
        S_plain = _add(v0, hybrid.irradiance_sh_sun(positions, E2E_SUN, br.E2E_ALBEDO, nu, nv, alpha=alpha))
        S = _add(v0, hybrid.irradiance_sh_sun(positions, E2E_SUN, br.E2E_ALBEDO, nu, nv, alpha=alpha, nerf_shadow=NERF))
        assert np.abs(S[:, :27] - v0[:, :27]).max() > 1e-3 and np.abs(S[:, :27] - S_plain[:, :27]).max() > 1e-3
        for visibility in (None, vis):
            visible = visibility is not None

            def hold(records):
                _set_volume(hybrid, records, res, lo, hi)
                if visible:
                    hybrid.set_irradiance_volume_visibility(maps, d0.max_distance, d0.sharpness_log2, d0.normal_bias)

            hold(S)
            v1 = _add(S, hybrid.irradiance_sh_bounce(positions, br.E2E_ALBEDO, nu, nv, alpha=alpha, visible=visible))
            hold(v1)
            v2 = _add(S, hybrid.irradiance_sh_bounce(positions, br.E2E_ALBEDO, nu, nv, alpha=alpha, visible=visible))
            for n, want in ((0, S), (2, v2)):
                for _ in range(2):  # (and run to run)
                    hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=n, albedo=br.E2E_ALBEDO, visibility=visibility, sun=E2E_SUN, sun_nerf_shadow=NERF)
                    got = _volume(hybrid)
                    assert got.tobytes() == want.tobytes(), (n, visible, np.abs(got - want).max())
                if visible:
                    d, held = hybrid.get_irradiance_volume_visibility()
                    assert held.tobytes() == maps.tobytes()
                    assert (d.n_u, d.n_v, d.sharpness_log2, d.max_distance, d.normal_bias) == (d0.n_u, d0.n_v, d0.sharpness_log2, d0.max_distance, d0.normal_bias)
                else:
                    with pytest.raises(RuntimeError, match=NO_VISIBILITY):
                        hybrid.get_irradiance_volume_visibility()
        assert hybrid.irradiance_sun_shadow_ms() > 0
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


def test_the_nerf_takes_sun_light_off_the_floor(hybrid):
    """under FLOOR_CASE's two points E(down) with the NeRF shadow lies above E without a sun and at or below E with the plain sun on every
    channel, strictly below it on at least one point; float 27 does not move"""
    albedo, res, lo, hi, nu, nv = br.FLOOR_CASE
    _load(hybrid, br.floor_scene())
    try:
        E = []
        for kw in ({}, dict(albedo=albedo, sun=E2E_SUN, sun_nerf_shadow=True), dict(albedo=albedo, sun=E2E_SUN)):
            hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, **kw)
            E.append(hybrid.irradiance_volume_at(TEST_POINTS, DOWN))
        dark, shadowed, sunlit = E
        print("\nE(down) at %s: no sun %s, the sun behind the NeRF %s, the plain sun %s" % (TEST_POINTS[0], dark[0, :3], shadowed[0, :3], sunlit[0, :3]))
        print("E(down) at %s: no sun %s, the sun behind the NeRF %s, the plain sun %s" % (TEST_POINTS[1], dark[1, :3], shadowed[1, :3], sunlit[1, :3]))
        assert np.all(shadowed[:, :3] > dark[:, :3]) and np.all(shadowed[:, :3] <= sunlit[:, :3])
        assert np.any(np.all(shadowed[:, :3] < sunlit[:, :3], axis=1))
        assert np.array_equal(shadowed[:, 3], dark[:, 3]) and np.array_equal(sunlit[:, 3], dark[:, 3])
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# --------------------------------------------------------------------------------------------- frames, refusals, bindings
def test_frames_devices_and_other_modes(hybrid, native, scene_unit):
    """a shadowed volume reaches the replicas of a multi-device context: the ShadeIrradianceVolume frame is the same bytes on two devices
    and on one, and differs from the plain sun's frame; Shade and ShadeGridEnvMap frames do not see it"""
    res, box, nu, nv = (2, 2, 2), (np.float32([0, 0, 0]), np.float32([1, 1, 1])), 16, 16
    cam = native.make_camera(SUN_CAMERA, mc.WIDTH, mc.HEIGHT, (100.0, 100.0))
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        frames = {}
        for c in (hybrid, multi):
            _load(c, br.e2e_scene())
            c.set_geometry_opts()
        hybrid.set_geometry_opts(ambientcolor=mv.SKY_AMBIENT)
        hybrid.compute_envmap_grid(2, 2, 16, 8)
        modes = (native.RENDER_SHADE, native.RENDER_SHADE_GRID_ENVMAP)
        hybrid.compute_irradiance_volume(res, box, nu, nv, albedo=0.64, sun=E2E_SUN)
        others = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
        hybrid.set_geometry_opts()
        for key, kw in (("sunlit", dict(albedo=0.64, sun=E2E_SUN)), ("shadowed", dict(albedo=0.64, sun=E2E_SUN, sun_nerf_shadow=True)),
                        ("shadowed_bounced_visible", dict(bounces=1, albedo=0.64, visibility=dict(n_u=8, n_v=8), sun=E2E_SUN, sun_nerf_shadow=True))):
            for c in (hybrid, multi):
                c.compute_irradiance_volume(res, box, nu, nv, **kw)
            one, one_depth = hybrid.render(cam, _opts(native), want_depth=True)
            two, two_depth = multi.render(cam, _opts(native), want_depth=True)
            assert (one[..., 3] > 0).sum() > 500
            assert one.tobytes() == two.tobytes() and one_depth.tobytes() == two_depth.tobytes(), key
            frames[key] = one
        assert len({f.tobytes() for f in frames.values()}) == 3
        changed = np.abs(frames["shadowed"] - frames["sunlit"]).max(-1) > 0
        print("\nthe NeRF in front of the sun changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(frames["shadowed"] - frames["sunlit"]).max()))
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
    up = dict(direction=(0, 1, 0))
    nan, inf = float("nan"), float("inf")
    bad = [(dict(min_transmittance=nan), "min_transmittance is NaN"), (dict(t_min=-1e-3), "t_min must be finite and >= 0"), (dict(t_min=nan), "t_min"), (dict(t_min=inf), "t_min")]
    c = native.Context(0)
    try:
        # the stage entry traces the model; the descriptors come first
        with pytest.raises(RuntimeError, match="No network"):
            c.irradiance_sh_sun(one, up, 0.5, 4, 4, nerf_shadow=True)
        with pytest.raises(RuntimeError, match="No network"):
            c.compute_irradiance_volume(res, (lo, hi), nu, nv, sun=up, sun_nerf_shadow=True)
        for shadow, message in bad:
            with pytest.raises(RuntimeError, match="invalid irradiance sun NeRF descriptor: " + message):
                c.irradiance_sh_sun(one, up, 0.5, 4, 4, nerf_shadow=shadow)
        with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: direction"):
            c.irradiance_sh_sun(one, dict(direction=(0, 0, 0)), 0.5, 4, 4, nerf_shadow=dict(t_min=-1.0))
        assert c.irradiance_sun_shadow_ms() == 0
    finally:
        c.close()
    try:
        hybrid.clear_meshes()
        hybrid.compute_irradiance_volume(res, (lo, hi), 4, 4)
        held = _volume(hybrid)
        # without meshes nothing is hit: no shadow ray, no light
        sh, rays, shadow = hybrid.irradiance_sh_sun(one, up, 0.5, 4, 4, return_rays=True, nerf_shadow=True, return_shadow=True)
        assert np.all(sh[:, :27] == 0) and np.all(sh[:, 27] == 1) and np.all(np.isinf(rays[..., 3])) and np.all(shadow == 0)
        assert hybrid.irradiance_sh_sun(np.zeros((0, 3), np.float32), up, 0.5, 4, 4, nerf_shadow=True).shape == (0, 28)
        for shadow, message in bad:
            with pytest.raises(RuntimeError, match="invalid irradiance sun NeRF descriptor: " + message):
                hybrid.compute_irradiance_volume(res, (lo, hi), 4, 4, bounces=1, albedo=0.5, sun=up, sun_nerf_shadow=shadow)
            with pytest.raises(RuntimeError, match="invalid irradiance sun NeRF descriptor: " + message):
                hybrid.irradiance_sh_sun(one, up, 0.5, 4, 4, nerf_shadow=shadow)
        for kw, message in ((dict(bounces=17, albedo=0.5), "n_bounces must be at most 16"), (dict(albedo=1.5), "albedo"), (dict(albedo=0.5, n_u=0), "n_u and n_v"),
                            (dict(albedo=0.5, sun=dict(direction=(0, 1, 0), shadow_bias=-0.5)), "shadow_bias"), (dict(albedo=0.5, visibility=dict(sharpness_log2=7)), "sharpness_log2")):
            with pytest.raises(RuntimeError, match=message):
                hybrid.compute_irradiance_volume(res, (lo, hi), **dict(dict(n_u=4, n_v=4, sun=up, sun_nerf_shadow=True), **kw))
        with pytest.raises(RuntimeError, match="position 0 is not finite"):
            hybrid.irradiance_sh_sun(np.float32([[0.5, nan, 0.5]]), up, 0.5, 4, 4, nerf_shadow=True)
        alpha = np.zeros((1, 16), np.float32)
        alpha[0, 7] = nan
        with pytest.raises(RuntimeError, match="alpha 7 is not finite"):
            hybrid.irradiance_sh_sun(one, up, 0.5, 4, 4, alpha=alpha, nerf_shadow=True)
        d = hybrid._volume_desc(res, (lo, hi), hybrid._sh_desc(4, 4, True, 0.01))
        with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: the bounce descriptor"):
            hybrid._check(hybrid.L.ngp_compute_irradiance_volume_sunlit_shadowed(hybrid.h, ctypes.byref(d), None, None, ctypes.byref(hybrid._sun_desc(up)),
                                                                                 ctypes.byref(hybrid._sun_nerf_desc(True))))
        assert _volume(hybrid).tobytes() == held.tobytes()  # the failed calls left the held volume alone
    finally:
        hybrid.clear_irradiance_volume()


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    """the Testbed's keyword and irradiance_volume_sun_nerf_shadow for the default volume of a ShadeIrradianceVolume render (the frame's sun,
    render_min_transmittance, t_min 0) hold the native entry's records as bytes, and --irradiance_volume_sun_nerf_shadow writes the frame the
    property gives, to the 8 bits of the file"""
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    hybrid.clear_meshes()
    scene = _write_scene(tmp_path, hybrid)
    w, h = mc.WIDTH, mc.HEIGHT
    cam = native.make_camera(SUN_CAMERA, w, h, (100.0, 100.0))
    tb = _sun_testbed(pyngp, scene)
    assert tb.irradiance_volume_sun_nerf_shadow is False
    plain = tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, sun=True)
    vol = tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, sun=True, sun_nerf_shadow=True)
    tb.nerf.render_min_transmittance = 0.05
    own = tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, bounces=1, albedo=[0.9, 0.5, 0.1], sun=True, sun_nerf_shadow=True)
    with pytest.raises(RuntimeError, match="sun_nerf_shadow belongs to sun"):
        tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, sun_nerf_shadow=True)
    box = (np.float32(vol["aabb"][0]), np.float32(vol["aabb"][1]))
    del tb
    sun = ((1.0, 1.0, 1.0), native.SUN_RADIANCE, 1e-3)  # _testbed's sun_dir
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, sun=sun, sun_nerf_shadow=True)
        assert c.get_irradiance_volume()[1].tobytes() == vol["sh"].tobytes() and vol["sh"].tobytes() != plain["sh"].tobytes()
        direct = c.render(cam, _opts(native))
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, min_transmittance=0.05, bounces=1, albedo=(0.9, 0.5, 0.1), sun=sun, sun_nerf_shadow=(0.05, 0.0))
        assert c.get_irradiance_volume()[1].tobytes() == own["sh"].tobytes() and own["sh"].tobytes() != vol["sh"].tobytes()
        assert c.irradiance_sun_shadow_ms() > 0
    finally:
        c.close()
    tb = _sun_testbed(pyngp, scene)
    tb.irradiance_volume_sun = True
    sunlit = tb.render(w, h, 1, True)
    del tb
    tb = _sun_testbed(pyngp, scene)
    tb.irradiance_volume_sun_nerf_shadow = True  # (without irradiance_volume_sun it is not looked at)
    assert tb.render(w, h, 1, True).tobytes() != sunlit.tobytes()
    del tb
    tb = _sun_testbed(pyngp, scene)
    tb.irradiance_volume_sun, tb.irradiance_volume_sun_nerf_shadow = True, True
    on = tb.render(w, h, 1, True)
    assert tb.get_irradiance_volume()["sh"].tobytes() == vol["sh"].tobytes()  # the render holds compute_irradiance_volume(sun=True, sun_nerf_shadow=True)'s records
    del tb
    changed = np.abs(on - sunlit).max(-1) > 0
    print("\npyngp: irradiance_volume_sun_nerf_shadow changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(on - sunlit).max()))
    assert (on[..., 3] > 0).sum() > 500 and changed.sum() > 100 and on.tobytes() == direct.tobytes()
    # the command line writes that frame: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit)
    frames = {}
    for shadow in (False, True):
        tb = _sun_testbed(pyngp, scene, camera=False)
        tb.irradiance_volume_sun, tb.irradiance_volume_sun_nerf_shadow = True, shadow
        frames[shadow] = tb.render(w, h, 1, True)
        del tb

    def as_png(frame):
        a = np.clip(frame[..., 3:4], 0, 1)
        v = np.clip(np.where(a > 0, frame[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
        srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
        return np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)

    expect = as_png(frames[True])
    # (the shadowed floor is in the default camera's frame; there the NeRF takes at most 0.002 off a pixel, which 8 bits mostly hide: the
    # file is held to the shadowed frame, and that the flag reaches the volume is the property's check above)
    assert (np.abs(frames[True] - frames[False]).max(-1) > 0).sum() > 20
    exe = pkg("build").build_main()
    out = tmp_path / "shot.png"
    r = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "ShadeIrradianceVolume", "--irradiance_volume_res", "2", "--irradiance_volume_sun",
                        "--irradiance_volume_sun_nerf_shadow", "--width", str(w), "--height", str(h), "--screenshot", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    png = np.asarray(Image.open(out)).astype(np.int64)
    assert png.shape == (h, w, 4) and np.abs(png - expect).max() <= 1 and (png != expect).mean() < 0.01, (np.abs(png - expect).max(), (png != expect).mean())
    assert (png[..., 3] > 0).sum() > 100
