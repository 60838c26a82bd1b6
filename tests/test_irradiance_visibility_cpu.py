"""Probe visibility without a GPU: the float64 reference's own properties (the octahedral map and its seams, a constant distance, the
slab example's two inequalities), what the GPU tests' points and frames reach on safe points, and the library's refusals, argument
checks and layouts on a host-only context."""
import re

import numpy as np
import pytest

import irradiance_sh_reference as sh_ref
import irradiance_visibility_reference as vr
import mesh_cases as mc
import mesh_reference as ref
import mesh_visibility_cases as vc
import mesh_volume_cases as mv


def test_encode_decode_round_trip():
    d = ref._unit(np.random.default_rng(0).normal(size=(1000, 3)))
    a, b = vr.encode(d)
    assert np.abs(a).max() <= 1 and np.abs(b).max() <= 1
    assert np.abs(vr.decode(a, b) - d).max() < 1e-14
    # the texel centres: the decode of the contract, and its inverse gives the centres back
    w = vr.texel_dirs()
    q = np.arange(64)
    a, b = vr.encode(w)
    assert np.abs(np.linalg.norm(w, axis=1) - 1).max() < 1e-15
    assert np.abs(a - (2 * (q % 8 + 0.5) / 8 - 1)).max() < 1e-15 and np.abs(b - (2 * (q // 8 + 0.5) / 8 - 1)).max() < 1e-15
    assert (w[:, 2] > 0).sum() == 24 and (w[:, 2] == 0).sum() == 16 and np.allclose(w[0], ref._unit(np.array([[-0.125, -0.125, -0.75]]))[0])  # texel 0: a corner of the square, next to -z


def _arc(d0, u, half=0.2, n=81):
    th = np.linspace(-half, half, n)[:, None]
    return ref._unit(np.cos(th) * d0 + np.sin(th) * u)


def test_wrapped_read_is_continuous_across_edges_and_corners():
    """a map holding a smooth function of the direction (the direction itself, three channels) read along short arcs across the four edges
    of the square (the meridians x = 0 and y = 0 of the lower hemisphere) and through its four corners (all of them the direction -z). A
    wrong neighbour across a seam is a texel from elsewhere on the sphere: a jump of the order of the function's range. The largest step
    along each arc must stay below four times the arc's mean step (bilinear interpolation between texels a quarter of the arc apart lets
    the steps vary by a small factor, not by the arc's 80 steps)."""
    maps = vr.texel_dirs()[None]
    arcs = {}
    for name, (a, b) in {"a=+1": (1.0, 0.37), "a=-1": (-1.0, -0.21), "b=+1": (0.45, 1.0), "b=-1": (-0.63, -1.0)}.items():
        d0 = vr.decode(a, b)
        across = np.cross(d0, [0.0, 0.0, 1.0])  # leaves the meridian's plane: the arc crosses the edge
        arcs[name] = _arc(d0, ref._unit(across[None])[0])
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            arcs["corner %+d%+d" % (sx, sy)] = _arc(np.array([0.0, 0.0, -1.0]), np.array([sx, 0.6 * sy, 0.0]) / np.hypot(1.0, 0.6), half=0.3)
    for name, d in arcs.items():
        a, b = vr.encode(d)
        v = vr.read_map(np.repeat(maps, d.shape[0], 0), d)
        step = np.linalg.norm(np.diff(v, axis=0), axis=1)
        print("%-12s largest step %.4f, mean %.4f, |read - direction| <= %.3f" % (name, step.max(), step.mean(), np.linalg.norm(v - d, axis=1).max()))
        assert step.max() <= 4 * step.mean(), (name, step.max(), step.mean())
        assert np.linalg.norm(v - d, axis=1).max() < 0.25  # (and the read follows the function to within a texel's width, 0.25 of the square)
        if name[0] in "ab":
            assert (np.abs(a) > 0.9).any() or (np.abs(b) > 0.9).any()
    # every wrapped index is inside the map, and wrapping is the identity inside
    i, j = np.meshgrid(np.arange(-1, 9), np.arange(-1, 9), indexing="ij")
    wi, wj = vr.wrap(i, j)
    assert wi.min() == 0 and wi.max() == 7 and wj.min() == 0 and wj.max() == 7
    assert np.array_equal(wi[1:9, 1:9], i[1:9, 1:9]) and np.array_equal(wj[1:9, 1:9], j[1:9, 1:9])


def test_constant_distance():
    dirs = vr.sphere_dirs(9, 9)
    D = 0.8
    for e in (0, 5, 6):
        maps, S = vr.maps_from_rays(dirs, np.full((3, 81), np.inf), e, D)
        assert (S > 0).all() and np.abs(maps[..., 0] - D).max() < 1e-14 and np.abs(maps[..., 1] - D * D).max() < 1e-14
        near, _ = vr.maps_from_rays(dirs, np.full((3, 81), 0.3), e, D)
        assert np.abs(near[..., 0] - 0.3).max() < 1e-14 and np.abs(near[..., 1] - 0.09).max() < 1e-14
    # one ray: the texels facing away from it have no weight and store (D, D^2), the others hold that ray's distance
    one, S = vr.maps_from_rays(vr.sphere_dirs(1, 1), np.full((1, 1), 0.25), 0, D)
    assert 0 < (S == 0).sum() < 64 and np.all(one[S == 0] == (D, D * D)) and np.allclose(one[S > 0], (0.25, 0.0625))
    # no occluder: every vis is 1 inside the box and the visible lookup is the plain one
    sh, res, lo, hi = mv.varying_volume()
    Dv = vr.default_max_distance(res, lo, hi)
    maps, _ = vr.maps_from_rays(vr.sphere_dirs(16, 16), np.full((36, 256), np.inf), 5, Dv)
    p, n = vc.seeded_points(lo, hi, outside=0.0)
    E, W, info = vr.lookup_visible(sh, res, lo, hi, maps.astype(np.float32), Dv, 0.0, p, n)
    E0, W0 = sh_ref.lookup(sh, res, lo, hi, p, n)
    assert np.all(info["vis"] == 1) and np.abs(E - E0).max() < 1e-12 and np.abs(W - W0).max() < 1e-14
    # the default D: 1.5 cell diagonals, an axis of one probe not counted, one probe in all: the box
    assert np.isclose(vr.default_max_distance((2, 2, 2), [-0.5] * 3, [0.5] * 3), 1.5 * np.sqrt(3))
    assert np.isclose(vr.default_max_distance((3, 1, 2), [0, 0, 0], [1, 5, 2]), 1.5 * np.sqrt(0.25 + 4))
    assert np.isclose(vr.default_max_distance((1, 1, 1), [0, 0, 0], [1, 2, 2]), 4.5)


def test_slab_stops_the_leak():
    """the contract's example, from the reference alone (the analytic wall): behind the wall the visible E is at most a third of the plain
    one, on the bright side at least 0.95 of the bright probes' pi L"""
    sh, res, lo, hi, D, maps = vc.slab_volume()
    assert np.isclose(D, 1.5 * np.sqrt(3))
    n = np.float32([[0.0, 0.0, 1.0]])
    out = {}
    for name, pt in (("behind", vc.BEHIND), ("lit", vc.LIT)):
        p = np.float32([pt])
        out[name] = (sh_ref.lookup(sh, res, lo, hi, p, n)[0][0, 0], vr.lookup_visible(sh, res, lo, hi, maps, D, 0.0, p, n)[0][0, 0])
    print("\nbehind the wall: plain %.4f, visible %.4f (x pi); bright side: plain %.4f, visible %.4f" % tuple(x / np.pi for x in out["behind"] + out["lit"]))
    assert out["behind"][1] <= out["behind"][0] / 3
    assert out["lit"][1] >= 0.95 * np.pi * vc.LEFT_RADIANCE
    # the loaded slab's frame is a similar copy: the same numbers
    sh2, _, lo2, hi2, D2, maps2 = vc.slab_volume(example=False)
    fr = vc.SlabFrame()
    assert np.isclose(D2, fr.sigma * D, rtol=1e-6)
    tris = mc.normalised(vc.slab_scene())[0]
    assert tris.shape == (12, 3, 3) and np.allclose(ref.mesh_box(tris)[0][0], fr.x[0]) and np.isclose(fr.x[1] - fr.x[0], 0.04 * fr.sigma)
    for name, pt in (("behind", vc.BEHIND), ("lit", vc.LIT)):
        E = vr.lookup_visible(sh2, res, lo2, hi2, maps2, D2, 0.0, fr.points([pt]), n)[0][0, 0]
        assert abs(E - out[name][1]) < 1e-4 * np.pi, (name, E, out[name][1])  # (float32 positions of the copy)
    # the analytic wall is the mesh: the brute-force nearest hit of the loaded slab from its probes
    dirs = vr.sphere_dirs(*vc.SLAB_RAYS)
    pos = vr.probe_positions(res, lo2, hi2).astype(np.float64)
    t, unsafe = ref.global_nearest([tris], np.repeat(pos, 256, 0), np.tile(dirs, (8, 1)))
    want = vc.slab_t_max(pos, dirs, x=fr.x, half=fr.half, centre=(fr.origin[1], fr.origin[2])).reshape(-1)
    ok = ~unsafe
    assert np.array_equal(np.isfinite(t[ok]), np.isfinite(want[ok])) and np.abs(t[ok & np.isfinite(t)] - want[ok & np.isfinite(t)]).max() < 1e-6


@pytest.mark.parametrize("res", [mv.VARYING_RES, (1, 1, 1), (2, 1, 3)])
def test_lookup_points_are_mostly_safe(res):
    """the GPU lookup test's points, from the reference alone: the unsafe share is under the cap, the Chebyshev branch, vis = 1 and dead
    probes all occur on safe points, and the float32 restatement's deviation is a rounding error, not a licence"""
    sh, _, lo, hi = mv.varying_volume()
    n_probes = res[0] * res[1] * res[2]
    sh = sh[:n_probes] if res != mv.VARYING_RES else sh
    D = vr.default_max_distance(res, lo, hi)
    maps = vc.seeded_maps(res, D)
    p, n = vc.seeded_points(lo, hi)
    for bias in (0.0, 0.05):
        E, W, scale, unsafe, tol, tol_w, info = vc.lookup_allowance(sh, res, lo, hi, maps, D, bias, p, n)
        safe = ~unsafe
        live = info["wgt"] > 0
        print("\nres %s bias %g: unsafe %.2f %%, corners with vis < 1: %d, < 0.5: %d, allowance / scale at most %.2e" %
              (res, bias, 100 * unsafe.mean(), (live & (info["vis"] < 1))[safe].sum(), (live & (info["vis"] < 0.5))[safe].sum(), (tol / np.maximum(scale, 1e-30))[safe].max()))
        assert unsafe.mean() <= mc.UNSAFE_CAP
        assert (live & (info["vis"] < 0.5))[safe].sum() > 20 and (live & (info["vis"] == 1))[safe].sum() > 100  # (one probe: one corner a point, its D the box's 1.5 diagonals)
        assert (tol / np.maximum(scale, 1e-30))[safe].max() < 1e-3


def test_visible_frame_reaches_its_branches_on_safe_pixels():
    D, maps = vc.varying_visibility()
    assert maps.shape == (36, 64, 2) and (maps[..., 0] < 0.99 * D).any() and maps[..., 0].max() <= D  # (some texels see the meshes)
    for metallic in (0.0, 1.0):
        fr = vc.varying_visible_frame(metallic)
        share = fr["unsafe_volume"].mean()
        safe = ~fr["unsafe_volume"] & fr["covered"]
        lit, clamped, hidden = (safe & fr["lit"]).sum(), (safe & fr["clamped"]).sum(), (safe & (fr["min_vis"] < 0.5)).sum()
        print("\nmetallic %g: unsafe %.2f %%, safe covered %d, lit %d, a channel clamped %d, a corner with vis < 0.5 %d, bound at most %.2e"
              % (metallic, 100 * share, safe.sum(), lit, clamped, hidden, fr["bound"][safe].max()))
        assert share <= mc.UNSAFE_CAP, share
        assert lit > 100 and clamped > 30 and hidden > 100, (lit, clamped, hidden)
        assert fr["bound"][safe].max() < 1e-4  # (a colour tolerance, not a licence)
        plain = mv.varying_frame(metallic)
        assert np.abs(fr["rgba"][..., :3][safe] - plain["rgba"][..., :3][safe]).max() > 100 * fr["bound"][safe].max()  # visibility shows in the colour, far above the bound


# ------------------------------------------------------------------------------------------------------------ the library
def test_visibility_desc_layout(native):
    C = native.C
    s = native.IrradianceVisibilityDesc
    names = ["n_u", "n_v", "sharpness_log2", "max_distance", "normal_bias"]
    assert [f for f, _ in s._fields_] == names
    assert C.sizeof(s) == 20 and [getattr(s, f).offset for f in names] == [0, 4, 8, 12, 16]
    with open(native.HEADER_PATH) as f:
        h = f.read()
    body = re.search(r"typedef struct ngp_irradiance_visibility_desc \{(.*?)\} ngp_irradiance_visibility_desc;", h, re.S).group(1)
    assert re.findall(r"\b(n_u|n_v|sharpness_log2|max_distance|normal_bias)\b(?=[,;])", body) == names


def test_visibility_entries_refuse_host_only(native):
    L = native.load_library()
    names = ("ngp_irradiance_distance_maps", "ngp_compute_irradiance_volume_visibility", "ngp_get_irradiance_volume_visibility", "ngp_set_irradiance_volume_visibility",
             "ngp_clear_irradiance_volume_visibility", "ngp_irradiance_volume_at_visible")
    for name in names:
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    p, n = np.float32([[0.5, 0.5, 0.5]]), np.float32([[0.0, 0.0, 1.0]])
    d = native.IrradianceVisibilityDesc()
    d.max_distance = 1.0
    maps = np.ones((1, 64, 2), np.float32)
    calls = [lambda: ctx.irradiance_distance_maps(p, 4, 4), lambda: ctx.compute_irradiance_volume_visibility(4, 4), lambda: ctx.clear_irradiance_volume_visibility(),
             lambda: ctx.irradiance_volume_at(p, n, visible=True), lambda: ctx._check(L.ngp_get_irradiance_volume_visibility(ctx.h, native.C.byref(d), None)),
             lambda: ctx._check(L.ngp_set_irradiance_volume_visibility(ctx.h, native.C.byref(d), maps.ctypes.data))]
    for call in calls:
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    # the argument checks of native.py come before the library
    with pytest.raises(ValueError, match="n x 3 each"):
        ctx.irradiance_volume_at(np.zeros((2, 3), np.float32), np.zeros((3, 3), np.float32), visible=True)
    with pytest.raises(ValueError, match=r"\(rz, ry, rx, 64, 2\)"):
        ctx.set_irradiance_volume_visibility(np.ones((2, 2, 2, 64), np.float32), 1.0)
    ctx.close()
