"""The NeRF mirrored in the meshes without a GPU (include/ngp_hip.h, "mesh reflection"): the restated mesh pass against
mesh_sun_nerf_shadow_cases', the conditions the two cases have to meet as the oracle traces their mirror rays, what the added term can and
cannot do to a pixel, and the option's descriptor and refusals on a host-only context."""
import numpy as np
import pytest

import mesh_cases as mc
import mesh_reflection_cases as rc
import mesh_sun_nerf_shadow_cases as sc
import mesh_volume_cases as mv
from test_irradiance_traced import _box_start, _cam_along, _linear, _oracle_payloads

_cache = {}


def mesh_box(oracle, case):
    """the render box while the case's meshes are loaded: their box inflated by 4"""
    h = oracle.mesh_scene(rc.scene(case))
    lo, hi = oracle.mesh_scene_aabb(h)
    oracle.mesh_scene_destroy(h)
    return lo - 4, hi + 4


def oracle_reflection(oracle, scene_unit, case="A"):
    """(h, w, 4) float32: the oracle's linear premultiplied rgba of the case's mirror rays from the reference's (q, unit(r)), UNCUT (the oracle
    has no t_max: a ray runs until it leaves the box), zeros where a pixel owns none; once per process and case"""
    if case not in _cache:
        fr = rc.frame(case)
        owns = fr["owns"]
        q = np.ascontiguousarray(fr["rq"][owns], np.float32)
        d = rc.unit32(fr["r"][owns].astype(np.float32))
        box = mesh_box(oracle, case)
        t0, alive = _box_start(q, d, box[0], box[1], np.zeros(q.shape[0], np.float32))
        m = oracle.make_model(dict(scene_unit, render_aabb=(tuple(float(x) for x in box[0]), tuple(float(x) for x in box[1]))))
        rgba, _, _ = oracle.trace_payloads(m, _cam_along(np.zeros(3), np.zeros(3)), _oracle_payloads(q, d, t0, alive), oracle.make_opts(capped_skip=True))
        oracle.release(m)
        out = np.zeros(owns.shape + (4,), np.float32)
        out[owns] = _linear(oracle, rgba)
        _cache[case] = out
    return _cache[case]


def test_restatement_is_render_with_sun_factor():
    """nothing added (no reflected radiance, zeros, or strength 0) gives mesh_sun_nerf_shadow_cases.render_with_sun_factor's arrays, every
    one of them, with and without a factor on the sun and an ambient term"""
    want = sc.frame()
    some = np.full((rc.HEIGHT, rc.WIDTH, 4), 0.5, np.float32)
    for kw in (dict(), dict(reflected=np.zeros((rc.HEIGHT, rc.WIDTH, 4), np.float32)), dict(reflected=some, strength=0.0)):
        got = rc.render_with_reflection(rc.meshes(), rc.CAMERA, rc.WIDTH, rc.HEIGHT, rc.FOCAL, sc.no_ambient, **kw)
        assert set(want) == set(rc.SHARED_KEYS)
        for k, x in want.items():
            assert np.array_equal(got[k], x), k
        assert not got["added"].any() and not got["added32"].any()
    sky = mv.sky_ambient_fn(mv.SKY_AMBIENT, (0.0, 1.0, 0.0))
    factor = np.linspace(0, 1, rc.WIDTH * rc.HEIGHT).reshape(rc.HEIGHT, rc.WIDTH)
    want = sc.render_with_sun_factor(sc.meshes(), sc.CAMERA, sc.WIDTH, sc.HEIGHT, sc.FOCAL, sky, factor, metallic=0.5)
    got = rc.render_with_reflection(rc.meshes(), rc.CAMERA, rc.WIDTH, rc.HEIGHT, rc.FOCAL, sky, factor, metallic=0.5)
    assert all(np.array_equal(got[k], x) for k, x in want.items())


def test_case_a_has_full_and_empty_mirror_rays(oracle, scene_unit):
    """conditions on case A, not tolerances: at least 200 pixels own a ray; of them at least 20 % see the object (alpha_r > 0.9) and at least
    30 % see nothing (alpha_r = 0); unsafe pixels are at most mesh_cases.UNSAFE_CAP of the covered ones. Measured: 840 rays, 311 full, 515
    empty, 14 between, no unsafe pixel, c from 0.19 to 0.94, no ray cut by a mesh."""
    fr = rc.frame("A")
    owns = fr["owns"]
    a = oracle_reflection(oracle, scene_unit, "A")[..., 3][owns]
    c = fr["c"][owns]
    print("\n%d pixels, covered %d, owning a ray %d, alpha_r > 0.9: %d, = 0: %d, between: %d, unsafe %d (mirror rays %d), c %.3f .. %.3f, cut %d, float32 deviation of q %.2e, of r %.2e"
          % (owns.size, fr["covered"].sum(), owns.sum(), (a > 0.9).sum(), (a == 0).sum(), ((a > 0) & (a <= 0.9)).sum(), (fr["unsafe"] & fr["covered"]).sum(),
             fr["t_unsafe"].sum(), c.min(), c.max(), np.isfinite(fr["t_hit"][owns]).sum(), fr["rq_dev"], fr["r_dev"]))
    assert owns.sum() >= rc.MIN_RAYS
    assert (a > 0.9).mean() >= rc.FULL_SHARE and (a == 0).mean() >= rc.EMPTY_SHARE
    assert (fr["unsafe"] & fr["covered"]).sum() <= mc.UNSAFE_CAP * fr["covered"].sum()
    assert np.all(fr["covered"]) and owns.sum() < fr["covered"].sum()  # (a pixel whose ray chose no mesh is covered too, and owns no ray)
    assert np.all(fr["rq"][~owns] == 0) and np.all(fr["r"][~owns] == 0) and np.all(fr["rq32"][~owns] == 0) and np.all(fr["t_hit"][~owns] == 0)
    assert np.all(np.isinf(fr["t_hit"][owns])) and not fr["t_unsafe"].any()
    assert np.all(c > 0) and np.all(c <= 1 + 1e-12) and c.max() - c.min() > 0.5  # F varies across the case
    assert np.allclose(np.linalg.norm(fr["r"][owns], axis=-1), 1.0, atol=1e-12)  # a mirrored unit vector
    assert (fr["r"][owns][:, 1] > 0).mean() > 0.95                               # off the floor's top, upwards (a few pixels see the slab's rim)
    assert fr["rq_dev"] < 1e-6 and fr["r_dev"] < 1e-6                            # float32 of values of size 2, a few roundings


def test_case_b_has_mirror_rays_cut_in_front_of_the_object(oracle, scene_unit):
    """conditions on case B: at least 100 rays have a finite t_hit, and at least 50 of those would see the object (uncut alpha_r > 0.9 by the
    oracle). A covered pixel whose primary ray found no triangle owns no ray. Measured: 867 owners, 2205 covered pixels without a triangle,
    279 cut rays, 73 of them full, t_hit from 0.007 to 0.423, no unsafe pixel, the float32 form of t_hit within 4.2e-7."""
    fr = rc.frame("B")
    owns = fr["owns"]
    cut = owns & np.isfinite(fr["t_hit"])
    a = oracle_reflection(oracle, scene_unit, "B")[..., 3]
    print("\ncovered %d, owning a ray %d, covered without a triangle %d, cut %d (uncut alpha_r > 0.9: %d), unsafe %d (mirror rays %d), t_hit %.3f .. %.3f, float32 deviation of t_hit %.2e"
          % (fr["covered"].sum(), owns.sum(), (fr["covered"] & ~owns).sum(), cut.sum(), (cut & (a > 0.9)).sum(), (fr["unsafe"] & fr["covered"]).sum(), fr["t_unsafe"].sum(),
             fr["t_hit"][cut].min(), fr["t_hit"][cut].max(), fr["t_dev"]))
    assert cut.sum() >= rc.MIN_CUT and (cut & (a > 0.9)).sum() >= rc.MIN_CUT_FULL
    assert (fr["unsafe"] & fr["covered"]).sum() <= mc.UNSAFE_CAP * fr["covered"].sum()
    assert np.all(fr["covered"][owns]) and np.all(fr["t_hit"][cut] > 0)
    assert fr["rq_dev"] < 1e-6 and fr["r_dev"] < 1e-6 and 0 < fr["t_dev"] < 1e-5  # (a grazing hit stretches the rounding of q and r along the ray)


def test_the_added_term_only_adds(oracle, scene_unit):
    """the added term never darkens a pixel and is 0 where alpha_r = 0 or where a pixel owns no ray; depth and coverage are untouched;
    F = 1 at c = 0 and F = Cspec0 at c = 1; strength scales the term; the float32 form of the term is the float64 one to a few roundings"""
    plain = rc.frame("A")
    refl = oracle_reflection(oracle, scene_unit, "A")
    fr = rc.frame("A", refl)
    a = refl[..., 3]
    assert np.all(fr["rgba"] >= plain["rgba"]) and np.array_equal(fr["depth"], plain["depth"]) and np.array_equal(fr["rgba"][..., 3], plain["rgba"][..., 3])
    same = (a == 0) | ~plain["owns"]
    assert np.array_equal(fr["rgba"][same], plain["rgba"][same]) and not fr["added"][same].any()
    seen = plain["owns"] & (a > 0.9)
    assert seen.sum() > 100 and np.all(fr["added"][seen].sum(-1) > 0)
    assert np.allclose(fr["rgba"][..., :3], plain["rgba"][..., :3] + fr["added"], rtol=0, atol=1e-15)
    half = rc.frame("A", refl, strength=0.5)
    assert np.allclose(half["added"], 0.5 * fr["added"], rtol=1e-15, atol=0)
    # what a float32 program makes of the term: a handful of roundings of values below 1
    assert np.abs(fr["added32"].astype(np.float64) - fr["added"]).max() < 1e-6
    # F at the ends of c, for three materials
    for kw in (dict(), dict(metallic=1.0), dict(metallic=0.3, specular=0.5, basecolor=(0.9, 0.5, 0.1))):
        base2 = np.asarray(kw.get("basecolor", (0.8, 0.8, 0.8)), np.float32).astype(np.float64) ** 2
        cspec0 = 0.08 * float(np.float32(kw.get("specular", 1.0))) + (base2 - 0.08 * float(np.float32(kw.get("specular", 1.0)))) * float(np.float32(kw.get("metallic", 0.0)))
        F = rc.fresnel(np.array([0.0, 1.0, 0.5]), **kw)
        assert np.allclose(F[0], 1.0, atol=1e-15) and np.allclose(F[1], cspec0, atol=1e-15)
        assert np.all(F[2] > np.minimum(cspec0, 1.0) - 1e-15) and np.all(F[2] < np.maximum(cspec0, 1.0) + 1e-15)
    # a metallic surface tints the reflection by its own colour, a dielectric one does not
    tinted = rc.frame("A", refl, metallic=1.0, basecolor=(0.9, 0.5, 0.1))
    px = seen & (plain["c"] > 0.8)
    assert px.sum() > 10
    ratio = tinted["added"][px] / refl[..., :3][px].astype(np.float64)
    assert np.all(ratio[:, 0] > ratio[:, 1]) and np.all(ratio[:, 1] > ratio[:, 2])


# ------------------------------------------------------------------------------------------------------------ the library
def test_option_round_trip_and_refusals_on_a_host_only_context(native):
    L = native.load_library()
    for name in ("ngp_set_mesh_reflection", "ngp_get_mesh_reflection", "ngp_get_frame_mesh_reflection", "ngp_get_frame_mesh_reflection_ms"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    try:
        assert ctx.mesh_reflection() is None  # off by default
        ctx.set_mesh_reflection(True)
        assert ctx.mesh_reflection() == dict(strength=1.0, min_transmittance=np.float32(0.01), t_min=0.0)
        ctx.set_mesh_reflection(dict(strength=0.25, min_transmittance=0.05, t_min=0.5))
        assert ctx.mesh_reflection() == dict(strength=0.25, min_transmittance=np.float32(0.05), t_min=0.5)
        ctx.set_mesh_reflection(dict(strength=0.0))  # allowed: the frame is then the option-off frame
        assert ctx.mesh_reflection() == dict(strength=0.0, min_transmittance=np.float32(0.01), t_min=0.0)
        for mt in (0.0, -1.0, 2.0, float("inf")):  # no refusal: <= 0 selects 0.01 when a frame is traced
            ctx.set_mesh_reflection(dict(min_transmittance=mt))
            assert ctx.mesh_reflection()["min_transmittance"] == np.float32(mt)
        nan, inf = float("nan"), float("inf")
        ctx.set_mesh_reflection(dict(strength=2.0, min_transmittance=0.02, t_min=0.5))
        kept = dict(strength=2.0, min_transmittance=np.float32(0.02), t_min=0.5)
        for bad, message in ((dict(min_transmittance=nan), "min_transmittance is NaN"), (dict(t_min=-1e-3), "t_min must be finite and >= 0"), (dict(t_min=nan), "t_min"),
                             (dict(t_min=inf), "t_min"), (dict(t_min=-inf), "t_min"), (dict(strength=-1e-3), "strength must be finite and >= 0"),
                             (dict(strength=nan), "strength"), (dict(strength=inf), "strength")):
            with pytest.raises(RuntimeError, match="invalid mesh reflection descriptor: " + message):
                ctx.set_mesh_reflection(bad)
            assert ctx.mesh_reflection() == kept  # a refused call leaves the option alone
        with pytest.raises(ValueError, match="mesh_reflection: True, False, None or a dict"):
            ctx.set_mesh_reflection(dict(tmin=0.0))
        with pytest.raises(ValueError, match="mesh_reflection: True, False, None or a dict"):
            ctx.set_mesh_reflection((1.0, 0.01, 0.0))
        for off in (None, False):
            ctx.set_mesh_reflection(True)
            ctx.set_mesh_reflection(off)
            assert ctx.mesh_reflection() is None
        with pytest.raises(RuntimeError, match="null argument"):
            ctx._check(L.ngp_get_mesh_reflection(ctx.h, None, None))
        # the stage entries read a frame: they need a device
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_mesh_reflection(16)
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_mesh_reflection_ms()
    finally:
        ctx.close()
