"""The sun pass without a GPU: the float64 reference's own properties (the share of unsafe rays and the mix of shadowed and open rays in
every case the GPU file uses, linearity, a sun below the horizon, a NeRF in front, the light an open floor throws up) and the library's
refusals on a host-only context."""
import re

import numpy as np
import pytest

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import irradiance_sun_reference as sr
import irradiance_visibility_reference as vr
from irradiance_volume_cases import GEN_POINTS

UNSAFE_SHARE = 0.02  # of the rays with a hit


@pytest.mark.parametrize("nu,nv", br.RAY_SHAPES)
def test_stage_cases_are_safe_and_mixed(nu, nv):
    """from the reference alone: at most 2 % of the rays with a hit are unsafe, and every case with K >= 15 has shadowed and open safe rays"""
    case = sr.stage_case(nu, nv)
    info, safe = case["info"], case["safe"]
    print("\n%2d x %2d: hits %3d, facing the sun %3d, shadowed %3d, open %3d, unsafe %d, nearest shadow hit %.3f, float32 deviation %.2e, allowance %.2e (largest B %.3f)"
          % (nu, nv, info["hit"].sum(), info["facing"].sum(), info["shadowed"].sum(), info["lit"].sum(), info["unsafe"].sum(), info["t_shadow"].min(), case["dev"],
             case["allow"], case["B"].max()))
    assert info["hit"].sum() > 0 and (info["unsafe"] & info["hit"]).sum() <= UNSAFE_SHARE * info["hit"].sum()
    if nu * nv >= 15:
        assert (info["shadowed"] & safe).any() and (info["lit"] & safe).any()
        assert case["allow"] < 1e-3 * case["B"].max()
    else:
        assert info["shadowed"].sum() == 1  # K = 1: one ray, which hits, faces the sun and is shadowed
    if (nu, nv) == (16, 16):
        assert (info["hit"].sum(), info["facing"].sum(), info["shadowed"].sum(), info["lit"].sum(), info["unsafe"].sum()) == (386, 262, 155, 107, 0)
    assert np.all(case["B"][~info["lit"]] == 0) and np.all(case["B"][info["lit"] & (case["alpha"] < 1)] > 0)


def test_end_to_end_cases_are_mostly_safe():
    """the lattices the GPU file lights, their own probes' rays, under the default sun (1, 1, 1): few unsafe, and the sun reaches some hits"""
    for (res, lo, hi, nu, nv), scene in ((br.E2E_CASE, br.e2e_scene()), (br.FLOOR_CASE[1:], br.floor_scene())):
        probes = vr.probe_positions(res, lo, hi)
        hit = br.hits(br.normalised(scene), probes, nu, nv)
        _, info = sr.sun_rays(hit, probes, nu, nv, (1, 1, 1), sr.STAGE_RADIANCE, sr.STAGE_BIAS, 0.64, None)
        assert (info["unsafe"] & info["hit"]).sum() <= UNSAFE_SHARE * info["hit"].sum() and info["lit"].any()


def _stage(nu=9, nv=9, sun=sr.STAGE_SUN, radiance=sr.STAGE_RADIANCE, albedo=br.STAGE_ALBEDO, alpha="stage"):
    hit = br.hits(br.stage_meshes(), GEN_POINTS, nu, nv)
    a = br.stage_alpha(GEN_POINTS.shape[0], nu * nv) if isinstance(alpha, str) else alpha
    B, info = sr.sun_rays(hit, GEN_POINTS, nu, nv, sun, radiance, sr.STAGE_BIAS, albedo, a)
    return B, info, hit


def test_linear_in_radiance_and_albedo():
    B1, _, hit = _stage(radiance=np.float32([1.0, 0.5, 0.25]), albedo=np.float32([0.25, 0.125, 0.5]))
    B2, _, _ = _stage(radiance=np.float32([2.0, 1.0, 0.5]), albedo=np.float32([0.25, 0.125, 0.5]))
    B3, _, _ = _stage(radiance=np.float32([1.0, 0.5, 0.25]), albedo=np.float32([0.5, 0.25, 1.0]))
    R1, R2, R3 = (br.records(B, hit["t"], 9, 9) for B in (B1, B2, B3))
    assert np.abs(R1[:, :27]).max() > 1e-2
    assert np.abs(R2[:, :27] - 2 * R1[:, :27]).max() < 1e-14 and np.abs(R3[:, :27] - 2 * R1[:, :27]).max() < 1e-14
    assert np.array_equal(R1[:, 27], R2[:, 27])


def test_a_sun_below_every_facing_hit_gives_nothing():
    """a cube seen from outside: every hit's normal faces the probe; a probe above the top face sees that face alone, and a sun straight
    below lights none of it"""
    import mesh_cases as mc

    cube = [mc.cube().astype(np.float32) * np.float32(0.25) + np.float32(0.5)]
    probe = np.float32([[0.625, 1.2, 0.625]])
    hit = br.hits(cube, probe, 16, 16)
    assert (hit["tri"] >= 0).sum() > 5 and np.all(hit["N"][hit["tri"] >= 0][:, 1] > 0.99)
    B, info = sr.sun_rays(hit, probe, 16, 16, (0, -1, 0), sr.STAGE_RADIANCE, sr.STAGE_BIAS, 0.8, None)
    assert np.all(B == 0) and not info["facing"].any()
    B, info = sr.sun_rays(hit, probe, 16, 16, (0, 1, 0), sr.STAGE_RADIANCE, sr.STAGE_BIAS, 0.8, None)
    assert info["lit"].sum() == (hit["tri"] >= 0).sum() and np.all(B[info["lit"]] > 0)


def test_an_opaque_nerf_in_front_gives_nothing():
    ones = np.ones((GEN_POINTS.shape[0], 81), np.float32)
    B, info, _ = _stage(alpha=ones)
    assert info["lit"].any() and np.all(B == 0)
    B0, _, _ = _stage(alpha=None)
    Bz, _, _ = _stage(alpha=0 * ones)
    assert np.array_equal(B0, Bz) and B0.max() > 0.1


def test_an_open_floor_throws_sun_light_up():
    """over the unshadowed floor of FLOOR_CASE, the E the sun pass adds for the down-facing normal is positive on every channel and at most
    albedo x radiance x c x OVERSHOOT: the floor's radiance is albedo radiance c / pi everywhere, the irradiance of a radiance below X is
    below pi X, and nine coefficients at 16 x 16 rays overshoot by at most OVERSHOOT"""
    albedo, res, lo, hi, nu, nv = br.FLOOR_CASE
    probes = vr.probe_positions(res, lo, hi)
    hit = br.hits(br.normalised(br.floor_scene()), probes, nu, nv)
    sun = (1, 1, 1)
    B, info = sr.sun_rays(hit, probes, nu, nv, sun, sr.STAGE_RADIANCE, sr.STAGE_BIAS, albedo, None)
    assert info["hit"].any() and np.array_equal(info["lit"], info["hit"])  # nothing stands on the floor
    S = sr.sunlit(np.zeros((probes.shape[0], 28)), B, nu, nv)
    S[:, 27] = 1.0
    p, down = np.float32([[0.5, 0.05, 0.5], [0.3, 0.1, 0.6]]), np.float32([[0, -1, 0], [0, -1, 0]])
    E, W = sh_ref.lookup(S.astype(np.float32), res, lo, hi, p, down)
    c = float(sr.unit_sun(sun)[1])
    bound = np.float32(albedo).astype(np.float64) * sr.STAGE_RADIANCE.astype(np.float64) * c * sr.OVERSHOOT
    print("\nE(down) added by the sun over an open floor: %s, bound %s" % (E[0], bound))
    assert np.all(E > 0) and np.all(E <= bound) and np.all(W > 0)


# ------------------------------------------------------------------------------------------------------------ the library
def test_sun_desc_layout(native):
    C = native.C
    s = native.IrradianceSunDesc
    assert [f for f, _ in s._fields_] == ["direction", "radiance", "shadow_bias"] and C.sizeof(s) == 28 and s.radiance.offset == 12 and s.shadow_bias.offset == 24
    with open(native.HEADER_PATH) as f:
        h = f.read()
    body = re.search(r"typedef struct ngp_irradiance_sun_desc \{(.*?)\} ngp_irradiance_sun_desc;", h, re.S).group(1)
    assert re.findall(r"\b(direction|radiance|shadow_bias)\b(?=[\[,;])", body) == ["direction", "radiance", "shadow_bias"]
    assert np.allclose(native.SUN_RADIANCE, sr.STAGE_RADIANCE, rtol=1e-6, atol=0)
    d = native.Context._sun_desc({"direction": (0, 2, 0)})
    assert list(d.direction) == [0, 2, 0] and np.allclose(list(d.radiance), native.SUN_RADIANCE) and d.shadow_bias == np.float32(1e-3)
    d = native.Context._sun_desc(((1, 0, 0), 2.0, 0.5))
    assert list(d.radiance) == [2, 2, 2] and d.shadow_bias == 0.5


def test_sun_entries_refuse_host_only_and_bad_descriptors(native):
    L = native.load_library()
    for name in ("ngp_compute_irradiance_volume_sunlit", "ngp_irradiance_sh_sun", "ngp_get_irradiance_sun_ms"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    p = np.float32([[0.5, 0.5, 0.5]])
    box = (np.float32([0, 0, 0]), np.float32([1, 1, 1]))
    up = {"direction": (0, 1, 0)}
    for call in (lambda: ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=up), lambda: ctx.irradiance_sh_sun(p, up, 0.5, 4, 4),
                 lambda: ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, bounces=2, albedo=(0.1, 0.2, 0.3), visibility=dict(n_u=4, n_v=4), sun=((1, 1, 1), 2.0, 0.0)),
                 lambda: ctx.irradiance_sun_ms()):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    # the descriptor is looked at first: each refusal names its field
    nan, inf = float("nan"), float("inf")
    bad = [(dict(direction=(0, 0, 0)), "direction must be finite and not zero"), (dict(direction=(nan, 1, 0)), "direction"), (dict(direction=(inf, 1, 0)), "direction"),
           (dict(direction=(0, 1, 0), radiance=(1, -0.5, 1)), "radiance must be finite and >= 0"), (dict(direction=(0, 1, 0), radiance=nan), "radiance"),
           (dict(direction=(0, 1, 0), radiance=inf), "radiance"), (dict(direction=(0, 1, 0), shadow_bias=-1e-3), "shadow_bias must be finite and >= 0"),
           (dict(direction=(0, 1, 0), shadow_bias=nan), "shadow_bias"), (dict(direction=(0, 1, 0), shadow_bias=inf), "shadow_bias")]
    for sun, message in bad:
        with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: " + message):
            ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=sun)
        with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: " + message):
            ctx.irradiance_sh_sun(p, sun, 0.5, 4, 4)
    for albedo in (1.5, -0.1, nan):
        with pytest.raises(RuntimeError, match="albedo must be finite and in"):
            ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, albedo=albedo, sun=up)
        with pytest.raises(RuntimeError, match="albedo must be finite and in"):
            ctx.irradiance_sh_sun(p, up, albedo, 4, 4)
    with pytest.raises(RuntimeError, match="n_bounces must be at most 16"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, bounces=17, sun=up)
    # a sun without the bounce descriptor that carries the albedo, through the C ABI alone
    C = native.C
    d = ctx._volume_desc((2, 2, 2), box, ctx._sh_desc(4, 4, True, 0.01))
    with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: the bounce descriptor"):
        ctx._check(L.ngp_compute_irradiance_volume_sunlit(ctx.h, C.byref(d), None, None, C.byref(ctx._sun_desc(up))))
    with pytest.raises(RuntimeError, match="null argument"):
        ctx._check(L.ngp_compute_irradiance_volume_sunlit(ctx.h, C.byref(d), None, None, None))
    with pytest.raises(RuntimeError, match="null argument"):
        ctx._check(L.ngp_irradiance_sh_sun(ctx.h, 1, p.ctypes.data, C.byref(ctx._sh_desc(4, 4, True, 0.01)), None, np.float32([0.5] * 3).ctypes.data, None, None, None))
    # the argument checks of native.py come before the library
    with pytest.raises(ValueError, match="sun: direction"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=dict(radiance=1.0))
    with pytest.raises(ValueError, match="n x K values"):
        ctx.irradiance_sh_sun(p, up, 0.5, 4, 4, alpha=np.zeros(15, np.float32))
    ctx.close()
