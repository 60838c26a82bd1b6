"""The NeRF in front of the frames' sun without a GPU (include/ngp_hip.h, "sun: the NeRF in front of the frames' sun"): the restated mesh
pass against mesh_volume_cases', the conditions the case has to meet as the oracle traces its shadow rays, what a factor on the sun can and
cannot do to a pixel, and the option's descriptor and refusals on a host-only context."""
import numpy as np
import pytest

import mesh_cases as mc
import mesh_sun_nerf_shadow_cases as sc
import mesh_volume_cases as mv
from test_irradiance_sun_shadow_cpu import oracle_alpha

_cache = {}


def mesh_box(oracle):
    """the render box while the case's meshes are loaded: their box inflated by 4"""
    h = oracle.mesh_scene(sc.scene())
    lo, hi = oracle.mesh_scene_aabb(h)
    oracle.mesh_scene_destroy(h)
    return lo - 4, hi + 4


def oracle_alpha_s(oracle, scene_unit):
    """(h, w) float32: the oracle's alpha of the case's shadow rays from the reference's q, 0 where a pixel has none; once per process"""
    if "alpha" not in _cache:
        fr = sc.frame()
        a = np.zeros(fr["has_ray"].shape, np.float32)
        a[fr["has_ray"]] = oracle_alpha(oracle, scene_unit, fr["q"][fr["has_ray"]], sc.SUN, mesh_box(oracle))
        _cache["alpha"] = a
    return _cache["alpha"]


def test_restatement_is_render_with_ambient():
    """factor = 1 (and none) gives mesh_volume_cases.render_with_ambient's arrays, every one of them"""
    want = mv.render_with_ambient(sc.meshes(), sc.CAMERA, sc.WIDTH, sc.HEIGHT, sc.FOCAL, sc.no_ambient, sun_dir=sc.SUN)
    for factor in (None, 1.0, np.ones((sc.HEIGHT, sc.WIDTH))):
        got = sc.render_with_sun_factor(sc.meshes(), sc.CAMERA, sc.WIDTH, sc.HEIGHT, sc.FOCAL, sc.no_ambient, factor)
        for k, x in want.items():
            assert np.array_equal(got[k], x), k
    sky = mv.sky_ambient_fn(mv.SKY_AMBIENT, (0.0, 1.0, 0.0))
    want = mv.render_with_ambient(sc.meshes(), sc.CAMERA, sc.WIDTH, sc.HEIGHT, sc.FOCAL, sky, sun_dir=sc.SUN, metallic=0.5)
    got = sc.frame(ambient_fn=sky, metallic=0.5)
    assert all(np.array_equal(got[k], x) for k, x in want.items())


def test_case_has_blocked_and_open_shadow_rays(oracle, scene_unit):
    """conditions on the case, not tolerances: at least 200 pixels have a shadow ray; of them at least 10 % are blocked (alpha_s > 0.9) and at
    least 30 % open (alpha_s = 0); unsafe pixels are at most mesh_cases.UNSAFE_CAP of the covered ones. Measured: 830 rays, 302 blocked,
    514 open, no unsafe pixel, the float32 form of q within 2.6e-7."""
    fr = sc.frame()
    has = fr["has_ray"]
    a = oracle_alpha_s(oracle, scene_unit)[has]
    print("\n%d pixels, covered %d, with a shadow ray %d, alpha_s > 0.9: %d, = 0: %d, between: %d, unsafe %d, float32 deviation of q %.2e"
          % (has.size, fr["covered"].sum(), has.sum(), (a > 0.9).sum(), (a == 0).sum(), ((a > 0) & (a <= 0.9)).sum(), (fr["unsafe"] & fr["covered"]).sum(), fr["q_dev"]))
    assert has.sum() >= sc.MIN_RAYS
    assert (a > 0.9).mean() >= sc.BLOCKED_SHARE and (a == 0).mean() >= sc.OPEN_SHARE
    assert (fr["unsafe"] & fr["covered"]).sum() <= mc.UNSAFE_CAP * fr["covered"].sum()
    assert np.all(fr["q"][~has] == 0) and np.all(fr["q32"][~has] == 0) and np.all(np.any(fr["q"][has] != 0, axis=-1))
    assert np.array_equal(has, fr["covered"] & ~fr["shadowed"])
    assert fr["q_dev"] < 1e-6  # float32 of points of size 2, a few roundings


def test_a_factor_only_takes_away(oracle, scene_unit):
    """a factor <= 1 never brightens a pixel of the reference, and a factor of 0 is the reference's mesh-shadowed colour: the frame whose
    sun is switched off on every pixel"""
    plain = sc.frame()
    a = oracle_alpha_s(oracle, scene_unit)
    T = sc.factor_of(a)
    assert T.dtype == np.float32 and np.all(T <= 1) and np.all(T >= 0) and np.all(T[a == 0] == 1)
    assert np.all(sc.factor_of(np.float32([1.0000001, 2.0])) == 0)  # alpha above 1 (a tracer's rounding) clamps to no light
    fr = sc.frame(T)
    assert np.all(fr["rgba"] <= plain["rgba"]) and np.array_equal(fr["depth"], plain["depth"]) and np.array_equal(fr["rgba"][..., 3], plain["rgba"][..., 3])
    same = (T == 1) | ~plain["has_ray"]
    assert np.array_equal(fr["rgba"][same], plain["rgba"][same])
    darker = plain["lit"] & (a > 0.9)
    assert darker.sum() > 20 and np.all(fr["rgba"][..., :3][darker].sum(-1) < 0.2 * plain["rgba"][..., :3][darker].sum(-1))
    # factor 0: what the pass computes where the meshes shadow a pixel, light = 0
    dark = sc.frame(0.0)
    night = sc.render_with_sun_factor(sc.meshes(), sc.CAMERA, sc.WIDTH, sc.HEIGHT, sc.FOCAL, sc.no_ambient, np.zeros((sc.HEIGHT, sc.WIDTH)))
    assert np.array_equal(dark["rgba"], night["rgba"])
    assert np.all(dark["rgba"][..., :3][plain["has_ray"]] == 0)  # (no ambient light in this case: black)
    assert np.array_equal(dark["rgba"][plain["shadowed"]], plain["rgba"][plain["shadowed"]])
    sky = mv.sky_ambient_fn(mv.SKY_AMBIENT, (1.0, 0.0, 0.0))  # (up = x: the floor's normal is at right angles to it, half the sky term)
    lit, unlit = sc.frame(ambient_fn=sky), sc.frame(0.0, ambient_fn=sky)
    assert np.all(unlit["rgba"] <= lit["rgba"]) and (unlit["rgba"][..., :3][plain["has_ray"]] > 0).all()  # the ambient term stays


# ------------------------------------------------------------------------------------------------------------ the library
def test_option_round_trip_and_refusals_on_a_host_only_context(native):
    L = native.load_library()
    for name in ("ngp_set_sun_nerf_shadow", "ngp_get_sun_nerf_shadow", "ngp_get_frame_sun_shadow", "ngp_get_frame_sun_shadow_ms"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    try:
        assert ctx.sun_nerf_shadow() is None  # off by default
        ctx.set_sun_nerf_shadow(True)
        assert ctx.sun_nerf_shadow() == dict(min_transmittance=np.float32(0.01), t_min=0.0)
        ctx.set_sun_nerf_shadow(dict(min_transmittance=0.05, t_min=0.25))
        assert ctx.sun_nerf_shadow() == dict(min_transmittance=np.float32(0.05), t_min=0.25)
        ctx.set_sun_nerf_shadow((0.5, 100.0))
        assert ctx.sun_nerf_shadow() == dict(min_transmittance=0.5, t_min=100.0)
        for mt in (0.0, -1.0, 2.0, float("inf")):  # no refusal: <= 0 selects 0.01 when a frame is traced
            ctx.set_sun_nerf_shadow((mt, 0.0))
            assert ctx.sun_nerf_shadow()["min_transmittance"] == np.float32(mt)
        nan, inf = float("nan"), float("inf")
        ctx.set_sun_nerf_shadow((0.02, 0.5))
        for shadow, message in ((dict(min_transmittance=nan), "min_transmittance is NaN"), (dict(t_min=-1e-3), "t_min must be finite and >= 0"), (dict(t_min=nan), "t_min"),
                                (dict(t_min=inf), "t_min"), (dict(t_min=-inf), "t_min")):
            with pytest.raises(RuntimeError, match="invalid irradiance sun NeRF descriptor: " + message):
                ctx.set_sun_nerf_shadow(shadow)
            assert ctx.sun_nerf_shadow() == dict(min_transmittance=np.float32(0.02), t_min=0.5)  # a refused call leaves the option alone
        with pytest.raises(ValueError, match="sun_nerf_shadow: min_transmittance and t_min"):
            ctx.set_sun_nerf_shadow(dict(tmin=0.0))
        for off in (None, False):
            ctx.set_sun_nerf_shadow(True)
            ctx.set_sun_nerf_shadow(off)
            assert ctx.sun_nerf_shadow() is None
        with pytest.raises(RuntimeError, match="null argument"):
            ctx._check(L.ngp_get_sun_nerf_shadow(ctx.h, None, None))
        # the stage entries read a frame: they need a device
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_sun_shadow(16)
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_sun_shadow_ms()
    finally:
        ctx.close()
