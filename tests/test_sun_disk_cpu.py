"""The sun's disk without a GPU (include/ngp_hip.h, "sun: the sun's disk"): the library's table of shadow directions against the float64
restatement, the conditions the two cases have to meet through the float64 tracer and the oracle's depth, what V and f can do to a pixel,
and the option's descriptor, defaults and refusals on a host-only context."""
import numpy as np
import pytest

import nerf_mesh_shadow_cases as nc
import sun_disk_cases as sd

SUNS = ((1.0, 1.0, 1.0), (0.0, 0.0, 1.0), (-0.3, 0.9, 0.2))  # the case's, an axis, a general one
_cache = {}


@pytest.fixture(scope="module")
def host(native):
    c = native.Context(-1)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("n_rays", sd.ALLOWED_RAYS)
def test_table_is_the_float64_restatement(n_rays, host):
    """for three sun directions and spp indices 0, 1, 7: the library's table equals the restatement after rounding to float32; every
    direction has unit length to 1e-7 and lies within the radius (1 + 1e-6) of s^; radius 0 gives K copies of fl(s^); K = 1 gives fl(s^)"""
    for sun in SUNS:
        s64 = np.asarray(sun, np.float32).astype(np.float64)
        s64 = s64 / np.sqrt((s64 * s64).sum())
        for s in (0, 1, 7):
            host.set_sun_disk(dict(angular_radius=sd.RADIUS, n_rays=n_rays))
            got = host.sun_disk_directions(sun, s)
            want = sd.directions(sun, sd.RADIUS, n_rays, s)
            assert got.dtype == np.float32 and got.shape == (n_rays, 3) and got.tobytes() == want.tobytes(), (sun, s)
            g64 = got.astype(np.float64)
            assert np.abs(np.sqrt((g64 * g64).sum(1)) - 1.0).max() <= 1e-7
            angle = np.arccos(np.clip(g64 @ s64, -1.0, 1.0))
            assert angle.max() <= float(np.float32(sd.RADIUS)) * (1.0 + 1e-6), (sun, s, angle.max())
            if n_rays == 1:
                assert got.tobytes() == s64.astype(np.float32)[None].tobytes()
            else:
                assert np.unique(got, axis=0).shape[0] == n_rays and angle.max() > 0.9 * sd.RADIUS * np.sqrt((n_rays - 0.5) / n_rays)
                if s:
                    assert got.tobytes() != host.sun_disk_directions(sun, 0).tobytes()  # successive samples use rotated tables
            host.set_sun_disk(dict(angular_radius=0.0, n_rays=n_rays))
            assert host.sun_disk_directions(sun, s).tobytes() == np.tile(s64.astype(np.float32), (n_rays, 1)).tobytes()
    host.set_sun_disk(None)


def test_table_refusals(host, native):
    host.set_sun_disk(None)
    with pytest.raises(RuntimeError, match="the sun has no disk"):
        host.sun_disk_directions((1, 1, 1), 0)
    host.set_sun_disk(True)
    try:
        for sun in ((0.0, 0.0, 0.0), (float("nan"), 0.0, 1.0), (float("inf"), 0.0, 1.0)):
            with pytest.raises(RuntimeError, match="sun direction must be finite and have a length"):
                host.sun_disk_directions(sun, 0)
        with pytest.raises(RuntimeError, match="null argument"):
            host._check(native.load_library().ngp_sun_disk_directions(host.h, None, 0, None))
    finally:
        host.set_sun_disk(None)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _check_classes(name, count, owner, flagged):
    o, p, f = sd.classes(count, owner)
    n = int(owner.sum())
    print("\n%s: %d owners; open %d, partial %d, full %d; owner pixels with a flagged ray %d (%.2f %%)" % (name, n, o, p, f, (flagged & owner).sum(), 100.0 * (flagged & owner).sum() / n))
    assert o + p + f == n and n >= 200
    assert min(o, p, f) >= sd.CLASS_SHARE * n, (o, p, f, n)
    assert (flagged & owner).sum() <= sd.UNSAFE_CAP * n
    return n, o, p, f


def test_mesh_case_has_open_partial_and_full_pixels():
    """conditions on the mesh side through mesh_reference with the restated table, s = 0: each of open, partial and full is at least 10 %
    of the owners; owner pixels with a flagged disk ray are at most 3 %; no primary ray is flagged. M4's one-mesh rule alone leaves the
    whole floor in the sun: what the option changes."""
    c = sd.mesh_case()
    owner = c["owner"].reshape(c["shape"])
    n, o, p, f = _check_classes("mesh side", c["count"], owner, c["flagged"])
    assert not c["primary_unsafe"].any()
    assert np.all(c["count"][~owner] == 0) and np.all(c["q"][~c["owner"]] == 0)
    hidden = c["owner"] & ~c["shadowed"] & (c["count"].reshape(-1) == sd.K)
    print("owners M4 calls shadowed %d; fully blocked owners that M4 leaves in the sun %d" % ((c["owner"] & c["shadowed"]).sum(), hidden.sum()))
    assert hidden.sum() >= 50  # the plate's shadow on the floor, which M3's one-mesh rule cannot see
    assert c["V"].dtype == np.float32 and np.all(c["V"] <= 1) and np.all(c["V"] >= 0) and np.array_equal(c["V"].astype(np.float64) * sd.K, sd.K - c["count"])


def _oracle_frames(oracle, scene_unit, matrix):
    key = np.asarray(matrix, np.float32).tobytes()
    if key not in _cache:
        h = oracle.mesh_scene(nc.scene())
        cam = oracle.make_camera(matrix, nc.WIDTH, nc.HEIGHT, nc.FOCAL)
        m, mesh_depth = oracle.render_mesh(h, cam, oracle.make_mesh_opts(sun_dir=nc.SUN))
        lo, hi = oracle.mesh_scene_aabb(h)
        model = oracle.make_model(dict(scene_unit, render_aabb=(tuple(lo.tolist()), tuple(hi.tolist()))))
        n, depth, _ = oracle.render_nerf(model, cam, oracle.make_opts(depth_test=True), depth_buffer=mesh_depth)
        oracle.release(model)
        oracle.mesh_scene_destroy(h)
        _cache[key] = dict(m=m, n=n, depth=depth)
    return _cache[key]


@pytest.mark.parametrize("view", ["CAMERA", "CAMERA_ABOVE"])
def test_nerf_case_has_open_partial_and_full_pixels(view, oracle, scene_unit):
    """the same conditions on the NeRF side, through the oracle's depth, for both of nerf_mesh_shadow_cases' cameras; and what f does: it
    never exceeds 1, open pixels keep f = 1 as bits, count = K gives the hard pass's f as bits, the restated composite only takes away"""
    matrix = getattr(nc, view)
    fr = _oracle_frames(oracle, scene_unit, matrix)
    sh = sd.nerf_shadow(fr["n"][..., 3], fr["depth"], sd.directions(nc.SUN, sd.RADIUS, sd.K, 0), matrix_3x4=matrix)
    _check_classes("NeRF side, " + view, sh["count"], sh["owner"], sh["flagged"])
    hard = nc.shadow(fr["n"][..., 3], fr["depth"], nc.meshes(), matrix_3x4=matrix)
    full, open_ = sh["count"] == sd.K, sh["owner"] & (sh["count"] == 0)
    assert sh["f"].dtype == np.float32 and np.all(sh["f"] <= 1) and np.all(sh["f"][~sh["owner"]] == 1) and np.all(sh["f"][open_] == 1)
    assert full.sum() >= 20 and sh["f"][full].tobytes() == hard["f"][full].tobytes() and np.all(hard["blocked"][full])
    assert np.all(sh["f"] >= hard["f"].min())
    on, off = nc.composite(fr["n"], fr["m"], sh["f"]), nc.composite(fr["n"], fr["m"], np.ones_like(sh["f"]))
    assert np.all(on <= off) and np.array_equal(on[~(sh["count"] > 0)], off[~(sh["count"] > 0)])


def test_visibility_and_factor_restated():
    """V = (K - count) / K and f = 1 - strength (count / K) for every allowed K and count: V is exact, neither exceeds 1, count = K gives
    V = 0 and f = fl(1 - strength) as bits, count = 0 gives 1"""
    for n_rays in sd.ALLOWED_RAYS:
        count = np.arange(n_rays + 1)
        V = sd.visibility(count, n_rays)
        assert V.dtype == np.float32 and np.array_equal(V.astype(np.float64), (n_rays - count) / n_rays) and V[0] == 1 and V[-1] == 0
        for strength in (0.0, 0.3, 0.5, 1.0):
            f = sd.factor(count, n_rays, strength)
            assert f.dtype == np.float32 and np.all(f <= 1) and f[0] == 1 and np.all(np.diff(f) <= 0)
            assert f[-1].tobytes() == (np.float32(1) - np.float32(strength)).tobytes()


# ------------------------------------------------------------------------------------------------------------ the library
def test_option_round_trip_defaults_and_refusals_on_a_host_only_context(native):
    L = native.load_library()
    for name in ("ngp_set_sun_disk", "ngp_get_sun_disk", "ngp_sun_disk_directions", "ngp_get_frame_sun_disk", "ngp_get_frame_sun_disk_ms"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    try:
        assert ctx.sun_disk() is None  # off by default
        ctx.set_sun_disk(True)
        assert ctx.sun_disk() == dict(angular_radius=np.float32(sd.REAL_SUN), n_rays=16)
        for k in sd.ALLOWED_RAYS:
            ctx.set_sun_disk(dict(angular_radius=0.125, n_rays=k))
            assert ctx.sun_disk() == dict(angular_radius=0.125, n_rays=k)
        ctx.set_sun_disk(dict(n_rays=4))
        assert ctx.sun_disk() == dict(angular_radius=np.float32(sd.REAL_SUN), n_rays=4)
        for radius in (0.0, 0.5):
            ctx.set_sun_disk(dict(angular_radius=radius))
            assert ctx.sun_disk() == dict(angular_radius=radius, n_rays=16)
        nan, inf = float("nan"), float("inf")
        ctx.set_sun_disk(dict(angular_radius=0.25, n_rays=8))
        for disk, message in ((dict(angular_radius=nan), "angular_radius must be finite"), (dict(angular_radius=inf), "angular_radius"), (dict(angular_radius=-inf), "angular_radius"),
                              (dict(angular_radius=-1e-6), "angular_radius"), (dict(angular_radius=0.5001), "angular_radius"), (dict(n_rays=0), "n_rays must be 1, 2, 4, 8 or 16"),
                              (dict(n_rays=3), "n_rays"), (dict(n_rays=12), "n_rays"), (dict(n_rays=32), "n_rays"), (dict(n_rays=64), "n_rays"), (dict(n_rays=2 ** 32 - 1), "n_rays")):
            with pytest.raises(RuntimeError, match="invalid sun disk descriptor: " + message):
                ctx.set_sun_disk(disk)
            assert ctx.sun_disk() == dict(angular_radius=0.25, n_rays=8)  # a refused call leaves the option alone
        for bad in (dict(radius=0.1), dict(n_rays=-1), dict(n_rays=2.5), 3):
            with pytest.raises(ValueError, match="sun_disk"):
                ctx.set_sun_disk(bad)
        for off in (None, False):
            ctx.set_sun_disk(True)
            ctx.set_sun_disk(off)
            assert ctx.sun_disk() is None
        with pytest.raises(RuntimeError, match="null argument"):
            ctx._check(L.ngp_get_sun_disk(ctx.h, None, None))
        # the stage entries read a frame: they need a device
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_sun_disk(16)
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.frame_sun_disk_ms()
    finally:
        ctx.close()
