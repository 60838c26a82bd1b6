"""All the frame options at once, without a GPU: the conditions frame_options_cases' one case has to meet as the float64 tracer and the oracle
render it (every class of pixel present at once, few ties), the 48 option sets, and the composed float64 reference against the
restatements it is composed from: with one option on it is that option's own restatement, array for array, and with none on it is
mesh_reference's plain frame."""
import numpy as np

import ambient_change_cases as ac
import frame_options_cases as fo
import mesh_reference as ref
import mesh_reflection_cases as rc
import mesh_reflection_meshes_cases as hc
import mesh_sun_nerf_shadow_cases as sc
import nerf_mesh_shadow_cases as nc
import sun_disk_cases as sd

W, H = fo.WIDTH, fo.HEIGHT
_cache = {}


def oracle_case(oracle, scene_unit):
    """the case through the oracle, once per process: m (the mesh pass's frame) and its depth, n (the NeRF pass over zeros behind the mesh
    depth) and its depth, alone (the model's own alpha, no depth test), the owners' points and normals and the ambient ratio there"""
    if "case" not in _cache:
        h = oracle.mesh_scene(fo.scene())
        cam = oracle.make_camera(fo.CAMERA, W, H, fo.FOCAL)
        m, mesh_depth = oracle.render_mesh(h, cam, oracle.make_mesh_opts(sun_dir=fo.SUN))
        lo, hi = oracle.mesh_scene_aabb(h)
        model = oracle.make_model(dict(scene_unit, render_aabb=(tuple(lo.tolist()), tuple(hi.tolist()))))
        opts = oracle.make_opts(depth_test=True)
        n, depth, _ = oracle.render_nerf(model, cam, opts, depth_buffer=mesh_depth)
        alone, _, _ = oracle.render_nerf(model, cam, opts)
        owner = n[..., 3] > np.float32(nc.OWNER_ALPHA)
        p = nc.surface_points32(depth, fo.CAMERA, W, H, fo.FOCAL)[owner.reshape(-1)]
        grad = oracle.density_gradient(model, p)  # (the unit model's box is the unit cube: the warped position is p itself)
        oracle.release(model)
        oracle.mesh_scene_destroy(h)
        N, ok = ac.normals_from_gradient(grad)
        r = ac.case_ratio(p, np.where(ok[:, None], N, 1.0))
        g = np.ones((H, W, 3), np.float32)
        g[owner] = np.where(ok[:, None], r["g"], 1.0).astype(np.float32)
        changed = np.zeros((H, W), bool)
        changed[owner] = ok & (r["state"] == 2) & (r["g"] != 1).any(1)
        _cache["case"] = dict(m=m, mesh_depth=mesh_depth, n=n, depth=depth, alone=alone[..., 3], owner=owner, g=g, changed=changed, ratio=r)
    return _cache["case"]


def test_the_48_option_sets():
    """6 switches, the sub-option only with the reflection: 48 sets, each once in either order; the Gray-coded order changes one option
    between neighbours except across the sets that do not exist"""
    sets, gray = fo.option_sets(), fo.gray_order()
    assert len(sets) == 48 and len(set(sets)) == 48 and set(gray) == set(sets) and len(gray) == 48
    assert frozenset() in sets and fo.ALL in sets and all(t in sets for t in fo.TRIPLES)
    assert all(("hits" not in s) or ("refl" in s) for s in sets)
    steps = [len(a ^ b) for a, b in zip(gray, gray[1:])]
    assert steps.count(1) >= 40 and max(steps) <= 2
    assert fo.name(frozenset()) == "none" and fo.name(fo.ALL) == "sun+disk+refl+hits+shadow+ambient"


def test_case_has_every_class_of_pixel(oracle, scene_unit):
    """conditions on the case, not tolerances: every line of frame_options_cases.SHARES holds at 60 x 44 by the float64 tracer and the
    oracle's alpha and depth alone, and the pixels the float64 tracer flags over all the rays a pixel owns stay under UNSAFE_CAP. The lit
    mirrored hits and the penumbra on the NeRF are there too, so the sub-option and the soft factor have something to show."""
    c = oracle_case(oracle, scene_unit)
    geo = fo.geometry()
    sh = fo.nerf_shadow(fo.ALL, c["n"][..., 3], c["depth"])
    shares = fo.classes(geo, c["alone"], c["n"][..., 3], sh["count"], c["changed"])
    flagged = fo.flagged_pixels(geo, sh["flagged"])
    mr = geo["mirror"]
    lit = mr["cut"] & mr["faces_sun"] & (mr["shadow2"] == 1) & ~mr["hit_unsafe"]
    soft = sh["owner"] & (sh["count"] > 0) & (sh["count"] < fo.K)
    print("\n%d x %d: " % (W, H) + ", ".join("%s %.1f %% (>= %.0f %%)" % (k, 100 * shares[k], 100 * v) for k, v in fo.SHARES.items())
          + "; flagged %.2f %% (<= %.0f %%); lit mirrored hits %d, largest C2 %.3f; NeRF owners in a penumbra %d; ambient ties %d"
          % (100 * flagged.mean(), 100 * fo.UNSAFE_CAP, lit.sum(), mr["C2"].max(), soft.sum(), c["ratio"]["tie"].sum()))
    for k, least in fo.SHARES.items():
        assert shares[k] >= least, (k, shares[k], least)
    assert flagged.mean() <= fo.UNSAFE_CAP
    assert lit.sum() >= hc.MIN_LIT_OPEN and mr["C2"][lit].max() > 0.1 and soft.sum() >= 50
    assert geo["covered"].all() and np.all(c["m"][..., 3] == 1)  # every ray enters the scene box: a pixel without a triangle is the opaque black of no mesh
    assert np.all(c["m"][..., :3][~geo["owner"].reshape(H, W)] == 0)
    assert c["ratio"]["tie"].mean() <= ac.TIE_CAP


def test_no_option_is_the_plain_frame():
    """the composed reference with nothing on is mesh_reference.render: colour, depth and the pixels left out, array for array; the
    sub-option without the reflection changes nothing"""
    plain = ref.render(fo.meshes(), fo.CAMERA, W, H, fo.FOCAL, sun_dir=fo.SUN)
    for options in (frozenset(), frozenset(("hits",))):
        fr = fo.frame(options)
        assert np.array_equal(fr["rgba"], plain["rgba"]) and np.array_equal(fr["depth"], plain["depth"]) and np.array_equal(fr["unsafe"], plain["unsafe"])
        assert all(v is None for v in fr["records"].values())
    assert (plain["rgba"][..., :3].sum(-1) > 0).sum() > 500 and np.array_equal(fo.frame(frozenset())["rgba32"], plain["rgba"].astype(np.float32))


def test_one_option_is_its_own_restatement(oracle, scene_unit):
    """each of the six alone, with what the network would supply drawn at random or taken from the oracle: the sun shadow is
    mesh_sun_nerf_shadow_cases.render_with_sun_factor, the disk sun_disk_cases.mesh_colour of the restated count, the reflection
    mesh_reflection_cases.render_with_reflection, the sub-option alone the plain frame, the meshes' shadow nerf_mesh_shadow_cases.composite
    with nerf_mesh_shadow_cases.shadow's factor, the ambient change ambient_change_cases.composite; array for array. The reflection with
    its sub-option is mesh_reflection_meshes_cases' frame, which forms the sum in another order: to 1e-13."""
    rng = np.random.default_rng(11)
    view = (fo.meshes(), fo.CAMERA, W, H, fo.FOCAL, sc.no_ambient)
    geo = fo.geometry()
    alpha_s = rng.uniform(0, 1.2, (H, W)).astype(np.float32)
    reflected = rng.uniform(0, 1, (H, W, 4)).astype(np.float32)
    reflected[rng.uniform(size=(H, W)) < 0.3] = 0
    # the sun shadow
    got, want = fo.frame(("sun",), dict(alpha_s=alpha_s)), sc.render_with_sun_factor(*view, factor=sc.factor_of(alpha_s), sun_dir=fo.SUN)
    assert np.array_equal(got["rgba"], want["rgba"]) and np.array_equal(got["unsafe"], want["unsafe"]) and np.array_equal(got["depth"], want["depth"])
    assert np.array_equal(got["records"]["frame_sun_shadow"]["live"], want["has_ray"]) and not np.array_equal(got["rgba"], fo.frame(())["rgba"])
    own = geo["owner"].reshape(H, W)
    assert np.array_equal(got["records"]["frame_sun_shadow"]["q"][own], want["q"][own])
    # the disk
    count, flagged = sd.counts(fo.meshes(), geo["q"][geo["owner"]], sd.directions(fo.SUN, fo.RADIUS, fo.K, 0))
    V = np.zeros(W * H, np.float32)
    V[geo["owner"]] = sd.visibility(count, fo.K)
    want, unsafe = sd.mesh_colour(sd.mesh_geometry((0.5, 0.5), W, H, fo.meshes(), fo.CAMERA), V)
    got = fo.frame(("disk",))
    assert np.array_equal(got["rgba"], want) and np.array_equal(got["unsafe"][~own], unsafe[~own]) and np.array_equal(got["records"]["frame_sun_disk"]["count"][own], count)
    assert np.array_equal(got["unsafe"][own], (unsafe[own] | flagged))
    # the reflection, alone and with its sub-option
    got, want = fo.frame(("refl",), dict(reflected=reflected)), rc.render_with_reflection(*view, None, reflected, fo.REFLECTION["strength"], sun_dir=fo.SUN)
    assert np.array_equal(got["rgba"], want["rgba"]) and np.array_equal(got["unsafe"], want["unsafe"] | (want["owns"] & want["t_unsafe"]))
    assert np.array_equal(got["records"]["frame_mesh_reflection"]["r"], want["r"]) and got["records"]["frame_mesh_reflection_hits"] is None
    both, want = fo.frame(("refl", "hits"), dict(reflected=reflected)), hc.render_with_reflection_meshes(*view, None, reflected, "shade", fo.REFLECTION["strength"], sun_dir=fo.SUN)
    assert np.abs(both["rgba"] - want["rgba"]).max() <= 1e-13 and np.abs(both["rgba"] - got["rgba"]).max() > 0.01
    assert np.array_equal(both["records"]["frame_mesh_reflection_hits"]["C2"], want["C2"])
    # the NeRF side
    c = oracle_case(oracle, scene_unit)
    nerf = dict(n=c["n"], n_depth=c["depth"], g=c["g"])
    m32 = fo.frame(())["rgba"].astype(np.float32)
    got, sh = fo.frame(("shadow",), nerf), nc.shadow(c["n"][..., 3], c["depth"], fo.meshes(), matrix_3x4=fo.CAMERA, width=W, height=H, focal=fo.FOCAL)
    assert np.array_equal(got["rgba32"], nc.composite(c["n"], m32, sh["f"])) and np.array_equal(got["records"]["frame_mesh_shadow"]["w"], sh["record"][..., 3])
    assert (sh["f"] != 1).sum() > 50 and np.array_equal(got["depth"][sh["owner"]], c["depth"][sh["owner"]])
    got = fo.frame(("ambient",), nerf)
    one = np.ones((H, W), np.float32)
    assert np.array_equal(got["rgba32"], ac.composite(c["n"], m32, c["g"], one)) and not np.array_equal(got["rgba32"], ac.composite(c["n"], m32, np.ones_like(c["g"]), one))
    # and the float64 composite of every set stays within its own bound of the float32 one
    for options in (fo.ALL,) + fo.TRIPLES:
        fr = fo.frame(options, dict(nerf, alpha_s=alpha_s, reflected=reflected))
        assert np.all(np.abs(fr["rgba"][..., :3] - fr["rgba32"][..., :3]) <= fr["bound"]) and np.isfinite(fr["rgba"]).all()


def test_ratio_before_factor_and_soft_factor(oracle, scene_unit):
    """the interaction rules the composed reference follows: the ambient ratio scales the scratch before the shadow's factor, fl(fl(n g) f);
    with the disk the NeRF side's factor is sun_disk_cases.factor of the count and its hard value where the count is K; with the disk and
    the sun shadow the live shadow entries are the owners with V > 0"""
    c = oracle_case(oracle, scene_unit)
    nerf = dict(n=c["n"], n_depth=c["depth"], g=c["g"])
    m32 = fo.frame(("disk",))["rgba"].astype(np.float32)
    fr = fo.frame(("disk", "ambient", "shadow"), nerf)
    f = fr["shadow"]["f"]
    assert np.array_equal(fr["rgba32"], ac.composite(c["n"], m32, c["g"], f))
    hard = fo.frame(("ambient", "shadow"), nerf)["shadow"]
    full = fr["shadow"]["count"] == fo.K
    assert full.sum() > 20 and np.array_equal(f[full], np.full(full.sum(), np.float32(1) - np.float32(fo.SHADOW["strength"])))
    assert np.all(f[fr["shadow"]["owner"]] >= hard["f"].min()) and ((f < 1) & (f > hard["f"].min())).sum() >= 50
    own = fo.geometry()["owner"].reshape(H, W)
    sun = fo.frame(("sun", "disk"), dict(alpha_s=np.zeros((H, W), np.float32)))
    assert np.array_equal(sun["records"]["frame_sun_shadow"]["live"][own], (sun["mesh"]["V"] > 0)[own])
    assert (own & ~sun["records"]["frame_sun_shadow"]["live"]).sum() > 50
