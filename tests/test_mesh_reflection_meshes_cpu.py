"""The meshes in the mesh reflection without a GPU (include/ngp_hip.h, "mesh reflection, the meshes in it"): the restated mesh pass against
mesh_reflection_cases', the conditions the cases have to meet as the oracle traces their mirror rays, what the hit's term can and cannot do to
a pixel, and the option's round trip and refusals on a host-only context."""
import numpy as np
import pytest

import mesh_cases as mc
import mesh_reflection_cases as rc
import mesh_reflection_meshes_cases as hc
import mesh_sun_nerf_shadow_cases as sc
import mesh_volume_cases as mv
from test_irradiance_traced import _box_start, _cam_along, _linear, _oracle_payloads

_cache = {}


def oracle_reflection_uncut(oracle, scene_unit, case):
    """(h, w, 4) float32: the oracle's linear premultiplied rgba of the case's mirror rays from the reference's (q, unit(r)), UNCUT (the oracle
    has no t_max: a ray runs until it leaves the box), zeros where a pixel owns none; once per process and case. In case C the wall stands
    behind the object, so a cut ray crosses the same density as the uncut one."""
    if case not in _cache:
        fr = hc.frame(case)
        owns = fr["owns"]
        q = np.ascontiguousarray(fr["rq"][owns], np.float32)
        d = rc.unit32(fr["r"][owns].astype(np.float32))
        h = oracle.mesh_scene(hc.scene(case))
        lo, hi = oracle.mesh_scene_aabb(h)
        oracle.mesh_scene_destroy(h)
        box = (lo - 4, hi + 4)
        t0, alive = _box_start(q, d, box[0], box[1], np.zeros(q.shape[0], np.float32))
        m = oracle.make_model(dict(scene_unit, render_aabb=(tuple(float(x) for x in box[0]), tuple(float(x) for x in box[1]))))
        rgba, _, _ = oracle.trace_payloads(m, _cam_along(np.zeros(3), np.zeros(3)), _oracle_payloads(q, d, t0, alive), oracle.make_opts(capped_skip=True))
        oracle.release(m)
        out = np.zeros(owns.shape + (4,), np.float32)
        out[owns] = _linear(oracle, rgba)
        _cache[case] = out
    return _cache[case]


def test_restatement_is_render_with_reflection():
    """no hit colour handed in: mesh_reflection_cases.render_with_reflection's arrays, every one, in cases A and B, with and without a
    reflected radiance, an ambient term and a material; and in case A, where no ray is cut, the hit's shade changes nothing either"""
    some = np.full((hc.HEIGHT, hc.WIDTH, 4), 0.5, np.float32)
    sky = mv.sky_ambient_fn(mv.SKY_AMBIENT, (0.0, 1.0, 0.0))
    for case in ("A", "B"):
        for amb, kw in ((sc.no_ambient, dict()), (sc.no_ambient, dict(reflected=some, strength=0.5)), (sky, dict(reflected=some, metallic=0.5))):
            want = rc.render_with_reflection(rc.meshes(case), rc.CAMERA, rc.WIDTH, rc.HEIGHT, rc.FOCAL, amb, **kw)
            got = hc.render_with_reflection_meshes(hc.meshes(case), hc.CAMERA, hc.WIDTH, hc.HEIGHT, hc.FOCAL, amb, **kw)
            assert set(got) == set(want)
            for k, x in want.items():
                assert np.array_equal(got[k], x), (case, k)
    want = rc.render_with_reflection(rc.meshes("A"), rc.CAMERA, rc.WIDTH, rc.HEIGHT, rc.FOCAL, sc.no_ambient, reflected=some)
    got = hc.render_with_reflection_meshes(hc.meshes("A"), hc.CAMERA, hc.WIDTH, hc.HEIGHT, hc.FOCAL, sc.no_ambient, reflected=some, hit_colour="shade")
    assert not got["cut"].any() and not got["C2"].any()
    for k, x in want.items():
        assert np.array_equal(got[k], x), k


def test_cases_meet_their_conditions(oracle, scene_unit):
    """conditions, not tolerances. Case C: at least 100 lit hits whose ray sees nothing of the NeRF (alpha_r = 0) and at least 20 whose ray
    the object hides (alpha_r > 0.9, by the oracle's uncut trace: the wall stands behind the object). Case B: at least 100 sun-facing hits in
    a mesh's shadow, and both values of shadow2. Unsafe hits are at most mesh_cases.UNSAFE_CAP of the cut rays in both; case A cuts no ray."""
    assert not hc.frame("A")["cut"].any()
    for case in ("B", "C"):
        fr = hc.frame(case)
        a = oracle_reflection_uncut(oracle, scene_unit, case)[..., 3]
        cut, faces, lit = fr["cut"], fr["cut"] & fr["faces_sun"], fr["cut"] & fr["faces_sun"] & (fr["shadow2"] == 1)
        print("\ncase %s: owners %d, cut rays %d, hits that face the sun %d, of them lit %d (alpha_r = 0: %d, > 0.9: %d, between: %d) and shadowed %d; unsafe hits %d; smallest |N.V| %.2f; "
              "float32 deviation of p2 %.2e, of q2 %.2e" % (case, fr["owns"].sum(), cut.sum(), faces.sum(), lit.sum(), (lit & (a == 0)).sum(), (lit & (a > 0.9)).sum(),
                                                           (lit & (a > 0) & (a <= 0.9)).sum(), (faces & ~lit).sum(), (fr["hit_unsafe"] & cut).sum(), np.abs(fr["ndv2"][cut]).min(),
                                                           fr["p2_dev"], fr["q2_dev"]))
        assert (fr["hit_unsafe"] & cut).sum() <= mc.UNSAFE_CAP * cut.sum()
        assert fr["p2_dev"] < 1e-5 and fr["q2_dev"] < 1e-5
        assert not fr["C2"][~cut].any() and not fr["p2"][~cut].any()
        if case == "C":
            assert (lit & (a == 0)).sum() >= hc.MIN_LIT_OPEN and (lit & (a > 0.9)).sum() >= hc.MIN_LIT_HIDDEN
        else:
            assert (faces & ~lit).sum() >= hc.MIN_SHADOWED and lit.sum() > 0
            n2 = fr["n2"][cut]  # (rays are cut on both meshes: at the plate's face towards the camera, and at the floor's top seen from the plate's pixels)
            assert (n2[:, 0] < -0.5).sum() > 50 and (n2[:, 1] > 0.5).sum() > 50


def test_the_hit_term_only_adds():
    """case C with a radiance handed in. A hit at alpha_r = 0 adds strength F (.) C2; a hit at alpha_r = 1 adds nothing beyond rgb_r; the term
    never darkens a pixel; a ray without a hit keeps its pixel; depth and coverage are untouched; a shadowed hit under no_ambient has C2 = 0"""
    plain = hc.frame("C")
    cut = plain["cut"]
    refl = np.zeros((hc.HEIGHT, hc.WIDTH, 4), np.float32)
    ys = np.arange(hc.HEIGHT)[:, None] + np.zeros((1, hc.WIDTH), int)
    refl[..., 3] = np.where(ys % 3 == 0, 0.0, np.where(ys % 3 == 1, 1.0, 0.4))
    refl[..., :3] = refl[..., 3:4] * np.float32([0.3, 0.2, 0.1])
    without = hc.frame("C", refl, hit_colour=None)
    fr = hc.frame("C", refl)
    assert cut.sum() > 100 and np.array_equal(fr["cut"], cut)
    assert np.all(fr["rgba"] >= without["rgba"] - 1e-15) and np.array_equal(fr["depth"], without["depth"]) and np.array_equal(fr["rgba"][..., 3], without["rgba"][..., 3])
    assert np.array_equal(fr["rgba"][~cut], without["rgba"][~cut]) and np.array_equal(fr["added"][~cut], without["added"][~cut])
    open_, full = cut & (refl[..., 3] == 0), cut & (refl[..., 3] == 1)
    assert open_.sum() > 20 and full.sum() > 20
    assert np.allclose(fr["added"][open_], (fr["F"] * fr["C2"])[open_], rtol=1e-15, atol=0) and not without["added"][open_].any()
    assert np.allclose(fr["added"][full], without["added"][full], rtol=1e-15, atol=0)
    lit = cut & fr["faces_sun"] & (fr["shadow2"] == 1)
    assert np.all(fr["added"][lit & open_].sum(-1) > 0)
    half = hc.frame("C", refl, strength=0.5)
    assert np.allclose(half["added"], 0.5 * fr["added"], rtol=1e-15, atol=0)
    assert np.abs(fr["added32"].astype(np.float64) - fr["added"]).max() < 1e-5
    # a C2 handed in takes the reference's place
    own = hc.frame("C", refl, hit_colour=np.full((hc.HEIGHT, hc.WIDTH, 3), 0.25, np.float32))
    assert np.allclose(own["added"][open_], 0.25 * fr["F"][open_], rtol=1e-15, atol=0) and np.array_equal(own["C2"], fr["C2"])
    # case B: a hit in a mesh's shadow has nothing but the ambient term
    b = hc.frame("B")
    dark = b["cut"] & (b["shadow2"] == 0)
    assert dark.sum() >= hc.MIN_SHADOWED and not b["C2"][dark].any()
    sky = hc.frame("B", ambient_fn=mv.sky_ambient_fn(mv.SKY_AMBIENT, (0.0, 1.0, 0.0)))
    up = sky["n2"][dark][:, 1] > 0.5  # (the sky term is (1 - N.up) / 2: nothing on the floor's top, all of it on the plate's sides)
    assert np.all(sky["C2"][dark][~up].sum(-1) > 0) and (~up).sum() > 20 and not sky["C2"][dark][up].any()


def test_option_round_trip_and_refusals_on_a_host_only_context(native):
    L = native.load_library()
    for name in ("ngp_set_mesh_reflection_meshes", "ngp_get_mesh_reflection_meshes", "ngp_get_frame_mesh_reflection_hits", "ngp_get_frame_mesh_reflection_hits_ms"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    try:
        assert ctx.mesh_reflection_meshes() is False  # off by default
        ctx.set_mesh_reflection_meshes(True)
        assert ctx.mesh_reflection_meshes() is True and ctx.mesh_reflection() is None  # (a sub-option: it does not switch the reflection on)
        ctx.set_mesh_reflection(True)
        ctx.set_mesh_reflection(None)
        assert ctx.mesh_reflection_meshes() is True  # ... and the reflection does not switch it off
        ctx.set_mesh_reflection_meshes(False)
        assert ctx.mesh_reflection_meshes() is False
        for bad in (None, 1, "on", dict()):
            with pytest.raises(ValueError, match="mesh_reflection_meshes: True or False"):
                ctx.set_mesh_reflection_meshes(bad)
        with pytest.raises(RuntimeError, match="null argument"):
            ctx._check(L.ngp_get_mesh_reflection_meshes(ctx.h, None))
        with pytest.raises(RuntimeError, match="no HIP device"):  # the stage entries read a frame: they need a device
            ctx.frame_mesh_reflection_hits(16)
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_mesh_reflection_hits_ms()
    finally:
        ctx.close()
