"""The meshes in front of the sun on the NeRF without a GPU (include/ngp_hip.h, "sun: the meshes in front of the sun on the NeRF"): the
conditions the case has to meet as the oracle renders it, the restated composite against the NeRF pass's own, what a factor can and cannot
do to a pixel, and the option's descriptor and refusals on a host-only context."""
import numpy as np
import pytest

import mesh_cases as mc
import nerf_mesh_shadow_cases as nc

_cache = {}


def oracle_frames(oracle, scene_unit):
    """the case through the oracle, once per process: m (the mesh pass's frame) and its depth, n (the NeRF pass over zeros, behind the mesh
    depth) and the depth it leaves, full (the NeRF pass over m: the option-off frame)"""
    if "frames" not in _cache:
        h = oracle.mesh_scene(nc.scene())
        cam = oracle.make_camera(nc.CAMERA, nc.WIDTH, nc.HEIGHT, nc.FOCAL)
        m, mesh_depth = oracle.render_mesh(h, cam, oracle.make_mesh_opts(sun_dir=nc.SUN))
        lo, hi = oracle.mesh_scene_aabb(h)
        model = oracle.make_model(dict(scene_unit, render_aabb=(tuple(lo.tolist()), tuple(hi.tolist()))))
        opts = oracle.make_opts(depth_test=True)
        n, depth, _ = oracle.render_nerf(model, cam, opts, depth_buffer=mesh_depth)
        full, full_depth, _ = oracle.render_nerf(model, cam, opts, frame_buffer=m, depth_buffer=mesh_depth)
        oracle.release(model)
        oracle.mesh_scene_destroy(h)
        _cache["frames"] = dict(m=m, mesh_depth=mesh_depth, n=n, depth=depth, full=full, full_depth=full_depth)
    return _cache["frames"]


def oracle_shadow(oracle, scene_unit):
    if "shadow" not in _cache:
        fr = oracle_frames(oracle, scene_unit)
        _cache["shadow"] = nc.shadow(fr["n"][..., 3], fr["depth"], nc.meshes())
    return _cache["shadow"]


def test_case_has_blocked_and_open_surface_points(oracle, scene_unit):
    """conditions on the case, not tolerances, from the oracle's depth: at least 200 pixels own a surface point; of them at least 10 % are
    blocked and at least 30 % open; the float64 tracer calls at most mesh_cases.UNSAFE_CAP of their shadow rays unsafe. Measured: see the
    test's own line of output and DESIGN 3.16."""
    fr, sh = oracle_frames(oracle, scene_unit), oracle_shadow(oracle, scene_unit)
    owner, blocked = sh["owner"], sh["blocked"]
    a = fr["n"][..., 3]
    floor = fr["mesh_depth"] >= 0.01  # (a ray that enters no mesh's box leaves an opaque black pixel at no depth: the NeRF pass's rule for "nothing there")
    on_floor = owner & floor
    print("\n%d pixels, alpha > 0.001: %d, owners %d (over the floor %d), blocked %d, open %d, unsafe %d, bare mesh pixels %d, float32 deviation of p %.2e"
          % (a.size, (a > 0.001).sum(), owner.sum(), on_floor.sum(), blocked.sum(), (owner & ~blocked).sum(), sh["unsafe"].sum(), ((a == 0) & floor).sum(), sh["p_dev"]))
    assert owner.sum() >= nc.MIN_OWNERS
    assert blocked.sum() >= nc.BLOCKED_SHARE * owner.sum() and (owner & ~blocked).sum() >= nc.OPEN_SHARE * owner.sum()
    assert sh["unsafe"].sum() <= mc.UNSAFE_CAP * owner.sum()
    # the three kinds of pixel the frame is meant to have: the NeRF over a mesh, the NeRF over nothing, a mesh alone
    assert on_floor.sum() >= 50 and (owner & ~floor).sum() >= 50 and ((a == 0) & floor).sum() >= 50
    assert np.all(fr["m"][..., :3][~floor] == 0)
    assert not np.any(blocked & ~owner) and np.all(sh["p"][~owner] == 0) and np.all(sh["record"][~owner] == 0)
    assert np.array_equal(sh["record"][..., 3][owner], np.where(blocked, 2.0, 1.0)[owner])
    assert np.array_equal(fr["depth"][owner], fr["full_depth"][owner])  # the depth an owner reads is the option-off frame's
    assert sh["p_dev"] < 1e-6  # float32 of points of size 2, a few roundings
    # the plate itself is out of view: every mesh pixel of the frame is the floor
    lo, hi = [np.asarray(x, np.float64) for x in (nc.meshes()[1].reshape(-1, 3).min(0), nc.meshes()[1].reshape(-1, 3).max(0))]
    assert np.allclose(lo, [0.507, 1.190, 0.007], atol=1e-3) and np.allclose(hi, [1.493, 1.210, 0.993], atol=1e-3)


def test_surface_point_lies_on_the_ray_at_the_depth():
    """the restated p: its z-depth from the camera is the depth it was formed from, in float64 to rounding and in the float32 form to a few
    float32 roundings of a distance of that size"""
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.5, 3.0, (nc.HEIGHT, nc.WIDTH))
    o, d, fwd, pos = nc.pixel_rays()
    p = nc.surface_points(depth)
    assert np.abs((p - pos) @ fwd - depth.reshape(-1)).max() < 1e-12
    assert np.abs(np.cross(p - o, d)).max() < 1e-12
    p32 = nc.surface_points32(depth.astype(np.float32))
    assert p32.dtype == np.float32 and np.abs(p32 - nc.surface_points(depth.astype(np.float32))).max() < 2e-6


def test_composite_with_factor_one_is_the_nerf_pass_composite(oracle, scene_unit):
    """f = 1: the restated composite equals n + m (1 - a) array for array, and that is the frame the oracle's NeRF pass leaves when it
    composites over the mesh pass itself"""
    fr = oracle_frames(oracle, scene_unit)
    n, m = fr["n"], fr["m"]
    one = np.ones(n.shape[:2], np.float32)
    got = nc.composite(n, m, one)
    k = (np.float32(1) - n[..., 3:4]).astype(np.float32)
    want = np.where(n[..., 3:4] == 0, m, (n + (m * k).astype(np.float32)).astype(np.float32))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(got, fr["full"]) and (n[..., 3] > 0).sum() > 500 and ((n[..., 3] > 0) & (fr["mesh_depth"] >= 0.01)).sum() > 50


def test_a_factor_only_takes_away(oracle, scene_unit):
    """f <= 1 never brightens a pixel and leaves alpha and depth alone; pixels that are not blocked keep the option-off bits; strength 1
    leaves a blocked pixel over nothing black"""
    fr, sh = oracle_frames(oracle, scene_unit), oracle_shadow(oracle, scene_unit)
    n, m, off = fr["n"], fr["m"], fr["full"]
    assert sh["f"].dtype == np.float32 and np.all(sh["f"][~sh["blocked"]] == 1) and np.all(sh["f"][sh["blocked"]] == np.float32(0.5))
    on = nc.composite(n, m, sh["f"])
    assert np.all(on <= off) and np.array_equal(on[..., 3], off[..., 3])
    assert np.array_equal(on[~sh["blocked"]], off[~sh["blocked"]])
    lit = sh["blocked"] & (n[..., :3].sum(-1) > 0)
    assert lit.sum() > 50 and np.all(on[..., :3][lit].sum(-1) < off[..., :3][lit].sum(-1))
    black = nc.shadow(n[..., 3], fr["depth"], nc.meshes(), strength=1.0)
    assert np.array_equal(black["blocked"], sh["blocked"]) and np.all(black["f"][sh["blocked"]] == 0)
    dark = nc.composite(n, m, black["f"])
    alone = sh["blocked"] & (fr["mesh_depth"] < 0.01)
    assert alone.sum() > 20 and np.all(dark[..., :3][alone] == 0) and np.array_equal(dark[..., 3], off[..., 3])
    same = nc.shadow(n[..., 3], fr["depth"], nc.meshes(), strength=0.0)
    assert np.array_equal(nc.composite(n, m, same["f"]), off)


# ------------------------------------------------------------------------------------------------------------ the library
def test_option_round_trip_and_refusals_on_a_host_only_context(native):
    L = native.load_library()
    for name in ("ngp_set_mesh_shadow_on_nerf", "ngp_get_mesh_shadow_on_nerf", "ngp_get_frame_mesh_shadow", "ngp_get_frame_mesh_shadow_ms"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    try:
        assert ctx.mesh_shadow_on_nerf() is None  # off by default
        ctx.set_mesh_shadow_on_nerf(True)
        assert ctx.mesh_shadow_on_nerf() == dict(strength=0.5, bias=np.float32(1e-2))
        ctx.set_mesh_shadow_on_nerf(dict(strength=0.25, bias=0.125))
        assert ctx.mesh_shadow_on_nerf() == dict(strength=0.25, bias=0.125)
        ctx.set_mesh_shadow_on_nerf(dict(strength=1.0))
        assert ctx.mesh_shadow_on_nerf() == dict(strength=1.0, bias=np.float32(1e-2))
        ctx.set_mesh_shadow_on_nerf(dict(strength=0.0, bias=0.0))
        assert ctx.mesh_shadow_on_nerf() == dict(strength=0.0, bias=0.0)
        nan, inf = float("nan"), float("inf")
        ctx.set_mesh_shadow_on_nerf(dict(strength=0.75, bias=0.5))
        for shadow, message in ((dict(strength=nan), "strength must lie in"), (dict(strength=-1e-3), "strength"), (dict(strength=1.001), "strength"), (dict(strength=inf), "strength"),
                                (dict(bias=-1e-3), "bias must be finite and >= 0"), (dict(bias=nan), "bias"), (dict(bias=inf), "bias"), (dict(bias=-inf), "bias")):
            with pytest.raises(RuntimeError, match="invalid mesh shadow descriptor: " + message):
                ctx.set_mesh_shadow_on_nerf(shadow)
            assert ctx.mesh_shadow_on_nerf() == dict(strength=0.75, bias=0.5)  # a refused call leaves the option alone
        with pytest.raises(ValueError, match="mesh_shadow_on_nerf"):
            ctx.set_mesh_shadow_on_nerf(dict(strenght=0.5))
        for off in (None, False):
            ctx.set_mesh_shadow_on_nerf(True)
            ctx.set_mesh_shadow_on_nerf(off)
            assert ctx.mesh_shadow_on_nerf() is None
        with pytest.raises(RuntimeError, match="null argument"):
            ctx._check(L.ngp_get_mesh_shadow_on_nerf(ctx.h, None, None))
        # the stage entries read a frame: they need a device
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_mesh_shadow(16)
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_mesh_shadow_ms()
    finally:
        ctx.close()
