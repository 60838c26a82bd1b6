"""Probe visibility on the GPU: the distance maps against the float64 reference fed the GPU's own ray distances, the visible lookup against
the reference fed the same float32 maps, the slab example end to end, the lifetime rules and refusals, ShadeIrradianceVolume frames with
visibility through sharding, several devices and the hybrid frame, and pyngp and the command line. Tolerances: the docstrings of
irradiance_visibility_reference.py and mesh_visibility_cases.py; none comes from the code under test."""
import json

import numpy as np
import pytest

from conftest import pkg

import irradiance_sh_reference as sh_ref
import irradiance_visibility_reference as vr
import mesh_cases as mc
import mesh_visibility_cases as vc
import mesh_volume_cases as mv

pytestmark = pytest.mark.gpu

NO_VOLUME = "no irradiance volume"
NO_VISIBILITY = "no irradiance visibility: call ngp_compute_irradiance_volume_visibility or ngp_set_irradiance_volume_visibility first"
RAY_SHAPES = [(1, 1), (3, 5), (8, 8), (9, 9), (16, 16)]  # texels without weight; K < 64; one full chunk; a chunk and a tail of 17; four chunks
SHARPNESS = [0, 5, 6]


@pytest.fixture(scope="module")
def ctx(gpu_ctx, native):
    """meshes only, a context of this module's own"""
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF and the render scene's meshes"""
    c = native.Context(0)
    c.set_model(scene_unit)
    _load(c, mc.render_scene())
    yield c
    c.close()


def _load(c, scene):
    c.clear_meshes()
    for tris, center in scene:
        c.add_mesh(tris, center)


def _opts(native, mode=None, **kw):
    return native.make_opts(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0), render_mode=native.RENDER_SHADE_IRRADIANCE_VOLUME if mode is None else mode, **kw)


def _camera(native, name="defaults", w=mc.WIDTH, h=mc.HEIGHT):
    return native.make_camera(mc.camera_matrix(name), w, h, mc.focal(name))


def _set_volume(c, sh, res, lo, hi):
    c.set_irradiance_volume(mv.as_grid(sh, res), (lo, hi))


def _probes(scene):
    """five probes: far outside, beside, between and inside the meshes; five make two workgroups, the second with one live wave"""
    if scene == "render":  # the cube fills [0, 1]^3, the icosphere hovers over it around (0.8, 2.1, 0.8), the torus stands around (1.65, 0.8, 0.5)
        return mc.render_scene(), np.float32([[-2.0, 0.5, 0.5], [1.2, 0.45, 0.5], [0.6, 1.35, 0.7], [0.5, 0.5, 0.5], [3.0, 3.0, 3.0]]), 1.5
    fr = vc.SlabFrame()
    return vc.slab_scene(), fr.points([(-0.5, -0.5, -0.5), (0.5, 0.2, 0.1), (0.1, 0.0, 0.0), (0.0, 0.3, -0.2), (-2.0, 0.0, 0.0)]), float(np.float32(0.6 * fr.sigma * 2.6))


def _check_maps(got, t_max, nu, nv, e, D, what):
    """maps (P, 64, 2) from the GPU against the float64 maps of the same t_max. The allowance is GPU_FACTOR x the deviation of the float32
    restatement from float64 on these inputs and must stay under the condition 1e-4 D (m1), 1e-4 D^2 (m2). Texels whose float64 weight sum
    lies in (0, 2^-100) are left out: there float32's weights underflow (irradiance_visibility_reference.S_UNDERFLOW); a sum of exactly 0
    must give (D, D^2) as bytes."""
    want, S = vr.maps_from_rays(vr.sphere_dirs(nu, nv), t_max, e, D)
    f32, _ = vr.maps_from_rays(vr.sphere_dirs(nu, nv, np.float32), t_max, e, D, np.float32)
    skip = (S > 0) & (S < vr.S_UNDERFLOW)
    empty = S == 0
    Df = np.float32(D)
    assert np.all(got[empty] == np.float32([Df, Df * Df])), what
    ok = ~skip & ~empty
    dev = [float(np.abs(f32[..., c].astype(np.float64) - want[..., c])[ok].max()) if ok.any() else 0.0 for c in (0, 1)]
    err = [float(np.abs(got[..., c].astype(np.float64) - want[..., c])[ok].max()) if ok.any() else 0.0 for c in (0, 1)]
    allow = [mc.GPU_FACTOR * dev[0], mc.GPU_FACTOR * dev[1]]
    print("%-28s texels left out %3d, without weight %3d; m1 error %.2e (allowed %.2e, condition %.2e); m2 error %.2e (allowed %.2e, condition %.2e)"
          % (what, skip.sum(), empty.sum(), err[0], allow[0], 1e-4 * D, err[1], allow[1], 1e-4 * D * D))
    assert allow[0] < 1e-4 * D and allow[1] < 1e-4 * D * D, (what, "the float32 deviation itself breaks the condition", dev)
    assert err[0] <= allow[0] and err[1] <= allow[1], (what, err, allow)
    return skip.sum(), empty.sum()


@pytest.mark.parametrize("scene", ["render", "slab"])
def test_maps_match_reference(scene, ctx):
    meshes, probes, D = _probes(scene)
    _load(ctx, meshes)
    left_out = without = 0
    try:
        for nu, nv in RAY_SHAPES:
            _, _, t_max = ctx.irradiance_sphere_rays(probes, nu, nv)
            hits = np.isfinite(t_max)
            if nu * nv >= 64:
                assert hits[3].all() if scene == "render" else hits[2].all()  # the probe inside a mesh
                assert hits.any(1).sum() >= 3 and (~hits).any(1).sum() >= 3 and (t_max[hits] < D).any()  # probes that see meshes and sky, hits below the cap ...
                assert nu * nv < 256 or (t_max[hits] > D).any()                                           # ... and beyond it
            for e in SHARPNESS:
                got = ctx.irradiance_distance_maps(probes, nu, nv, e, D)
                assert got.shape == (5, 64, 2) and got.dtype == np.float32 and np.isfinite(got).all()
                a, b = _check_maps(got, t_max, nu, nv, e, D, "%s %dx%d e=%d" % (scene, nu, nv, e))
                left_out += a
                without += b
                assert np.all(got[..., 0] <= np.float32(D) * (1 + 1e-6)) and np.all(got[..., 0] >= 0)
    finally:
        ctx.clear_meshes()
    assert without > 0  # (1 x 1: the texels facing away from the one ray)


def test_maps_are_deterministic_and_independent_of_the_split(ctx):
    meshes, probes, D = _probes("render")
    _load(ctx, meshes)
    try:
        for nu, nv in ((9, 9), (16, 16)):
            whole = ctx.irradiance_distance_maps(probes, nu, nv, 5, D)
            again = ctx.irradiance_distance_maps(probes, nu, nv, 5, D)
            parts = np.concatenate([ctx.irradiance_distance_maps(probes[:2], nu, nv, 5, D), ctx.irradiance_distance_maps(probes[2:], nu, nv, 5, D)])
            assert whole.tobytes() == again.tobytes() and whole.tobytes() == parts.tobytes()
            assert np.unique(whole[..., 0]).size > 50  # (the maps are not flat)
    finally:
        ctx.clear_meshes()


def _small_scene():
    """32 triangles: an icosahedron in [0, 1]^3 and a cube beside it"""
    return [(pkg("meshio").icosphere(0), (0.0, 0.0, 0.0)), (mc.cube(), (1.2, 0.3, 0.1))]


def _many_probes(n=600, seed=41):
    """probes around and inside _small_scene's meshes. 600 of them with 64 x 64 rays each are 2.46 M rays: more than the 2^21 rays the host
    sends in one launch, so a call runs a chunk of 512 whole probes and a tail of 88"""
    return np.random.default_rng(seed).uniform(-0.4, 2.0, (n, 3)).astype(np.float32)


def test_maps_over_two_host_chunks(ctx):
    """every one of the 600 probes' maps from one call (two host chunks) is the bytes of the same probe asked for in calls of 100 probes (one
    chunk each): a probe's map does not depend on which probes share its launch, so the small calls are the reference"""
    _load(ctx, _small_scene())
    try:
        probes = _many_probes()
        whole = ctx.irradiance_distance_maps(probes, 64, 64, 5, 1.5)
        parts = np.concatenate([ctx.irradiance_distance_maps(probes[i:i + 100], 64, 64, 5, 1.5) for i in range(0, 600, 100)])
        assert whole.shape == (600, 64, 2) and np.isfinite(whole).all()
        assert np.array_equal(whole, parts)
        assert np.unique(whole[:512, :, 0]).size > 50 and np.unique(whole[512:, :, 0]).size > 50  # (neither chunk's maps are flat)
    finally:
        ctx.clear_meshes()


def test_no_meshes_is_the_plain_lookup(ctx):
    ctx.clear_meshes()
    sh, res, lo, hi = mv.varying_volume()
    _set_volume(ctx, sh, res, lo, hi)
    try:
        ctx.compute_irradiance_volume_visibility()
        d, maps = ctx.get_irradiance_volume_visibility()
        D = vr.default_max_distance(res, lo, hi)
        assert maps.shape == (3, 3, 4, 64, 2) and (d.n_u, d.n_v, d.sharpness_log2, d.normal_bias) == (16, 16, 5, 0.0)
        assert abs(d.max_distance - D) <= 2.0 ** -23 * D, (d.max_distance, D)
        _check_maps(maps.reshape(36, 64, 2), np.full((36, 256), np.inf), 16, 16, 5, d.max_distance, "no meshes 16x16 e=5")
        p, n = vc.seeded_points(lo, hi, outside=0.0)
        assert ctx.irradiance_volume_at(p, n, visible=True).tobytes() == ctx.irradiance_volume_at(p, n).tobytes()
    finally:
        ctx.clear_irradiance_volume()


@pytest.mark.parametrize("res", [mv.VARYING_RES, (1, 1, 1), (2, 1, 3)])
def test_visible_lookup_matches_reference(res, ctx):
    sh, _, lo, hi = mv.varying_volume()
    sh = sh[:res[0] * res[1] * res[2]]
    D = vr.default_max_distance(res, lo, hi)
    maps = vc.seeded_maps(res, D)
    p, n = vc.seeded_points(lo, hi)
    n_scaled = (n * np.linspace(0.5, 3.0, n.shape[0], dtype=np.float32)[:, None]).astype(np.float32)  # (the entry normalises)
    _set_volume(ctx, sh, res, lo, hi)
    try:
        for bias in (0.0, 0.05):
            ctx.set_irradiance_volume_visibility(vc.as_map_grid(maps, res), D, normal_bias=bias)
            got = ctx.irradiance_volume_at(p, n_scaled, visible=True).astype(np.float64)
            E, W, scale, unsafe, tol, tol_w, info = vc.lookup_allowance(sh, res, lo, hi, maps, D, bias, p, n_scaled)
            safe = ~unsafe
            assert unsafe.mean() <= mc.UNSAFE_CAP
            ratio = (np.abs(got[:, :3] - E) / np.maximum(tol, 1e-300))[safe].max()
            dw = np.abs(got[:, 3] - W)[safe].max()
            print("\nres %s bias %g: safe points %d, largest |dE| / allowance %.3f (allowance / scale at most %.2e), |dW'| %.2e (allowed %.2e)"
                  % (res, bias, safe.sum(), ratio, (tol / np.maximum(scale, 1e-30))[safe].max(), dw, tol_w))
            assert ratio <= 1.0 and dw <= tol_w, (ratio, dw, tol_w)
            assert np.all(got[W == 0] == 0)  # (every corner dead or out of sight)
        plain = ctx.irradiance_volume_at(p, n_scaled)
        assert np.abs(plain - got).max() > 0.1  # visibility is in the numbers (one probe: in W' alone, the blend of one record is that record)
    finally:
        ctx.clear_irradiance_volume()


def test_slab_end_to_end(ctx):
    sh, res, lo, hi, D, _ = vc.slab_volume(example=False)
    fr = vc.SlabFrame()
    _load(ctx, vc.slab_scene())
    _set_volume(ctx, sh, res, lo, hi)
    try:
        ctx.compute_irradiance_volume_visibility(*vc.SLAB_RAYS, vc.SLAB_SHARPNESS)
        d, grid = ctx.get_irradiance_volume_visibility()
        assert abs(d.max_distance - D) <= 2.0 ** -23 * D
        maps = grid.reshape(8, 64, 2)
        # the maps are those of the GPU's own rays
        _, _, t_max = ctx.irradiance_sphere_rays(vr.probe_positions(res, lo, hi), *vc.SLAB_RAYS)
        _check_maps(maps, t_max, *vc.SLAB_RAYS, vc.SLAB_SHARPNESS, d.max_distance, "slab volume")
        rng = np.random.default_rng(7)
        p = np.concatenate([fr.points([vc.BEHIND, vc.LIT]), fr.points(rng.uniform(-0.5, 0.5, (500, 3)))])
        n = np.concatenate([np.float32([[0, 0, 1], [0, 0, 1]]), mc._unit(rng.normal(size=(500, 3))).astype(np.float32)])
        got = ctx.irradiance_volume_at(p, n, visible=True).astype(np.float64)
        plain = ctx.irradiance_volume_at(p, n).astype(np.float64)
        E, W, scale, unsafe, tol, tol_w, _ = vc.lookup_allowance(sh, res, lo, hi, maps, d.max_distance, 0.0, p, n)
        safe = ~unsafe
        assert safe[:2].all() and unsafe.mean() <= mc.UNSAFE_CAP
        ratio = (np.abs(got[:, :3] - E) / tol)[safe].max()
        print("\nslab: behind the wall plain %.4f, visible %.4f (x pi); bright side plain %.4f, visible %.4f; largest |dE| / allowance %.3f"
              % (plain[0, 0] / np.pi, got[0, 0] / np.pi, plain[1, 0] / np.pi, got[1, 0] / np.pi, ratio))
        assert ratio <= 1.0 and np.abs(got[:, 3] - W)[safe].max() <= tol_w
        assert got[0, 0] <= plain[0, 0] / 3
        assert got[1, 0] >= 0.95 * np.pi * vc.LEFT_RADIANCE
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()


def test_lifetime_and_refusals(ctx, native):
    sh, res, lo, hi = mv.varying_volume()
    p, n = vc.seeded_points(lo, hi, n=64)
    one = np.float32([[0.5, 0.5, 0.5]])
    _load(ctx, mc.render_scene())
    try:
        # no volume
        for call in (lambda: ctx.compute_irradiance_volume_visibility(), lambda: ctx.get_irradiance_volume_visibility(), lambda: ctx.irradiance_volume_at(p, n, visible=True),
                     lambda: ctx.set_irradiance_volume_visibility(np.ones((3, 3, 4, 64, 2), np.float32), 1.0)):
            with pytest.raises(RuntimeError, match=NO_VOLUME):
                call()
        ctx.clear_irradiance_volume_visibility()  # (nothing to clear: no refusal)
        _set_volume(ctx, sh, res, lo, hi)
        # no visibility
        for call in (lambda: ctx.get_irradiance_volume_visibility(), lambda: ctx.irradiance_volume_at(p, n, visible=True)):
            with pytest.raises(RuntimeError, match=NO_VISIBILITY):
                call()
        # get after compute returns what set then reproduces
        ctx.compute_irradiance_volume_visibility(8, 8, 4, 5.0, 0.02)
        d, maps = ctx.get_irradiance_volume_visibility()
        assert (d.n_u, d.n_v, d.sharpness_log2) == (8, 8, 4) and d.max_distance == 5.0 and d.normal_bias == np.float32(0.02)
        before = ctx.irradiance_volume_at(p, n, visible=True)
        ctx.clear_irradiance_volume_visibility()
        with pytest.raises(RuntimeError, match=NO_VISIBILITY):
            ctx.irradiance_volume_at(p, n, visible=True)
        ctx.set_irradiance_volume_visibility(maps, d.max_distance, d.sharpness_log2, d.normal_bias)
        assert ctx.irradiance_volume_at(p, n, visible=True).tobytes() == before.tobytes()
        assert before.tobytes() != ctx.irradiance_volume_at(p, n).tobytes()
        # setting, computing and clearing the volume each drop the visibility
        _set_volume(ctx, sh, res, lo, hi)
        with pytest.raises(RuntimeError, match=NO_VISIBILITY):
            ctx.get_irradiance_volume_visibility()
        ctx.set_irradiance_volume_visibility(maps, 5.0)
        ctx.clear_irradiance_volume()
        with pytest.raises(RuntimeError, match=NO_VOLUME):
            ctx.get_irradiance_volume_visibility()
        _set_volume(ctx, sh, res, lo, hi)
        with pytest.raises(RuntimeError, match=NO_VISIBILITY):
            ctx.get_irradiance_volume_visibility()
        # descriptors
        ctx.set_irradiance_volume_visibility(maps, 5.0)
        bad = [(dict(sharpness_log2=7), "sharpness_log2"), (dict(max_distance=float("nan")), "max_distance"), (dict(max_distance=float("inf")), "max_distance"),
               (dict(normal_bias=-0.1), "normal_bias"), (dict(normal_bias=float("nan")), "normal_bias"), (dict(n_u=0), "n_u and n_v"), (dict(n_u=2048, n_v=2048), "too large")]
        for kw, message in bad:
            with pytest.raises(RuntimeError, match=message):
                ctx.compute_irradiance_volume_visibility(**kw)
        for kw, message in bad[:3] + [(dict(max_distance=0.0), "max_distance"), (dict(n_u=0), "n_u and n_v"), (dict(n_u=2048, n_v=2048), "too large")]:
            with pytest.raises(RuntimeError, match=message):
                ctx.irradiance_distance_maps(one, **kw)
        with pytest.raises(RuntimeError, match="is not finite"):
            ctx.irradiance_distance_maps(np.float32([[0.5, np.nan, 0.5]]), 4, 4)
        for m, message in ((np.nan, "is not finite"), (np.inf, "is not finite"), (-1.0, "is negative")):
            for c in (0, 1):
                wrong = maps.copy()
                wrong[1, 2, 3, 17, c] = m
                with pytest.raises(RuntimeError, match="m%d of texel 17 of probe %d %s" % (c + 1, 3 + 4 * (2 + 3 * 1), message)):
                    ctx.set_irradiance_volume_visibility(wrong, 5.0)
        for kw, message in ((dict(max_distance=0.0), "max_distance"), (dict(max_distance=-1.0), "max_distance"), (dict(sharpness_log2=9), "sharpness_log2"), (dict(normal_bias=-1.0), "normal_bias")):
            with pytest.raises(RuntimeError, match=message):
                ctx.set_irradiance_volume_visibility(maps, **dict(dict(max_distance=5.0), **kw))
        # the failed calls left the held maps alone
        assert ctx.get_irradiance_volume_visibility()[1].tobytes() == maps.tobytes()
        # points
        with pytest.raises(RuntimeError, match="position 1 is not finite"):
            ctx.irradiance_volume_at(np.float32([[0, 0, 0], [np.inf, 0, 0]]), n[:2], visible=True)
        for wrong in ([0, 0, 0], [np.nan, 0, 1]):
            with pytest.raises(RuntimeError, match="normal 1 is zero or not finite"):
                ctx.irradiance_volume_at(p[:2], np.float32([[0, 0, 1], wrong]), visible=True)
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()


# ----------------------------------------------------------------------------------------------------------------- frames
def _compute_varying(c):
    _set_volume(c, *mv.varying_volume())
    c.compute_irradiance_volume_visibility(*vc.VARYING_RAYS, vc.VARYING_SHARPNESS, vc.VARYING_MAX_DISTANCE)


@pytest.mark.parametrize("metallic", [0.0, 1.0])
def test_visible_frame_matches_reference(metallic, ctx, native):
    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts(metallic=metallic)
    try:
        _set_volume(ctx, *mv.varying_volume())
        plain = ctx.render(_camera(native), _opts(native), want_depth=True)
        _compute_varying(ctx)
        d, grid = ctx.get_irradiance_volume_visibility()
        img, depth = ctx.render(_camera(native), _opts(native), want_depth=True)
        ctx.clear_irradiance_volume_visibility()
        cleared = ctx.render(_camera(native), _opts(native), want_depth=True)
    finally:
        ctx.set_geometry_opts()
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()
    fr = vc.varying_visible_frame(metallic, maps=grid.reshape(36, 64, 2), D=d.max_distance)  # the reference fed the renderer's own maps
    dd, ratio, n = mv.check_volume_frame(fr, img, depth)
    safe = ~fr["unsafe_volume"] & fr["covered"]
    print("\nmetallic %g: safe covered pixels %d, a corner with vis < 0.5 on %d, ddepth %.2e, largest colour deviation / bound %.3f"
          % (metallic, n, (safe & (fr["min_vis"] < 0.5)).sum(), dd, ratio))
    assert fr["unsafe_volume"].mean() <= mc.UNSAFE_CAP and (safe & (fr["min_vis"] < 0.5)).sum() > 100
    assert dd <= mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][0] and ratio <= 1.0, (dd, ratio)
    # clearing the visibility gives the frame rendered before it was computed back, as bytes
    assert cleared[0].tobytes() == plain[0].tobytes() and cleared[1].tobytes() == plain[1].tobytes()
    assert img.tobytes() != plain[0].tobytes() and depth.tobytes() == plain[1].tobytes()


def test_other_modes_do_not_see_the_visibility(hybrid, native):
    cam = _camera(native)
    hybrid.set_geometry_opts(ambientcolor=mv.SKY_AMBIENT)
    hybrid.compute_envmap_grid(2, 2, 16, 8)
    modes = (native.RENDER_SHADE, native.RENDER_SHADE_GRID_ENVMAP)
    try:
        _set_volume(hybrid, *mv.varying_volume())
        without = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
        _compute_varying(hybrid)
        held = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.set_geometry_opts()
    for (a, ad), (b, bd) in zip(held, without):
        assert (a[..., 3] > 0).sum() > 500 and a.tobytes() == b.tobytes() and ad.tobytes() == bd.tobytes()


def _tiles(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // 8) * ((w + 7) // 8) + xs // 8, (xs % 8) + 8 * (ys % 8)


def test_tile_sharding_covers_frame(ctx, native):
    import torch

    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts()
    try:
        _compute_varying(ctx)
        w, h, world = 60, 36, 3
        cam = _camera(native, w=w, h=h)
        full, full_depth = ctx.render(cam, _opts(native), want_depth=True)
        assert (full[..., 3] == 1).sum() > 500
        tile, slot = _tiles(w, h)
        total, total_depth = np.zeros_like(full), np.zeros_like(full_depth)
        packed, packed_depth = np.zeros_like(full), np.zeros_like(full_depth)
        for r in range(world):
            mine = tile % world == r
            part, part_depth = ctx.render(cam, _opts(native, shard_index=r, shard_count=world), want_depth=True)
            assert not np.any(part[~mine])
            total[mine], total_depth[mine] = part[mine], part_depth[mine]
            n = native.load_library().ngp_packed_tiles(w, h, r, world) * 64
            rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
            ctx.render_device(cam, _opts(native, shard_index=r, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
            ctx.render_stats()  # synchronises the context's stream
            src = (tile // world) * 64 + slot
            packed[mine], packed_depth[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]]
    finally:
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes()


def test_multi_device_replicas_follow_the_visibility(ctx, native):
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        for c in (ctx, multi):
            _load(c, mc.render_scene())
            c.set_geometry_opts()
        cam = _camera(native)
        sh, res, lo, hi = mv.varying_volume()
        frames = []

        def both():
            one, one_depth = ctx.render(cam, _opts(native), want_depth=True)
            two, two_depth = multi.render(cam, _opts(native), want_depth=True)
            assert (one[..., 3] == 1).sum() > 500
            assert one.tobytes() == two.tobytes() and one_depth.tobytes() == two_depth.tobytes()
            frames.append(one)

        for c in (ctx, multi):
            _compute_varying(c)
        both()
        D = vr.default_max_distance(res, lo, hi)
        for c in (ctx, multi):  # a second set: other maps, a bias
            c.set_irradiance_volume_visibility(vc.as_map_grid(vc.seeded_maps(res, D), res), D, normal_bias=0.05)
        both()
        for c in (ctx, multi):
            c.clear_irradiance_volume_visibility()
        both()
        assert len({f.tobytes() for f in frames}) == 3
    finally:
        multi.close()
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()


def test_hybrid_multi_sample_frame(hybrid, native):
    """NeRF and meshes, two samples a pixel: the frame runs, equals itself on a second render and differs from the plain volume's"""
    cam = _camera(native)
    hybrid.set_geometry_opts()
    try:
        _set_volume(hybrid, *mv.varying_volume())
        plain = hybrid.render(cam, _opts(native, spp=2))
        _compute_varying(hybrid)
        a = hybrid.render(cam, _opts(native, spp=2))
        b = hybrid.render(cam, _opts(native, spp=2))
    finally:
        hybrid.clear_irradiance_volume()
    assert np.isfinite(a).all() and (a[..., 3] > 0).sum() > 500 and a.tobytes() == b.tobytes() and a.tobytes() != plain.tobytes()


# ------------------------------------------------------------------------------------------------- pyngp and the command line
# The default volume of a Testbed spans the render box, the unit cube the NeRF fills, and the NeRF hides whatever mesh stands inside it. So the
# wall stands just outside the box's face x = 1 (x in [1.095, 1.105], spanning the face) and a floor (a cube scaled to (4, 0.04, 4): y near
# 0.3, x in [1.21, 2.19]) lies behind it. A point of the floor is looked up with the four probes of the face x = 1 (the position clamped
# for the weights, not for the visibility), and each of them sees it through the wall, by another amount: visibility changes the floor's
# ambient light. The camera looks straight down on the floor; none of its rays crosses the NeRF.
SLAB_CAMERA = mc.look_at((1.7, 1.6, 0.5), (1.7, 0.3, 0.5))


def _wall_and_floor():
    floor = (mc.cube().astype(np.float64) * np.array([4.0, 0.04, 4.0])).astype(np.float32)
    return [(vc.slab_scene()[0][0], (0.6, 0.0, 0.0)), (floor, (1.2, -0.2, 0.0))]


def _write_slab_scene(tmp_path, hybrid):
    """the wall and the floor as .obj files, the unit NeRF as a snapshot, and the scene file that names them"""
    mi = pkg("meshio")
    entries = []
    for i, (tris, center) in enumerate(_wall_and_floor()):
        mi.save_obj(str(tmp_path / ("slab%d.obj" % i)), tris)
        entries.append({"center": [float(x) for x in center], "path": "slab%d.obj" % i, "type": "Mesh"})
    hybrid.save_snapshot_file(str(tmp_path / "unit.ingp"))
    entries.append({"center": [0, 0, 0], "path": "unit.ingp", "type": "Nerf"})
    path = tmp_path / "slab_geometry_scene.json"  # (the Testbed takes a scene file for a Geometry scene by the word in its name)
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def _testbed(pyngp, scene, visibility=None, camera=True):
    tb = pyngp.Testbed()
    tb.load_training_data(scene)
    assert tb.mode == pyngp.TestbedMode.Geometry
    tb.background_color = [0.0, 0.0, 0.0, 0.0]
    tb.render_mode = pyngp.RenderMode.ShadeIrradianceVolume
    if camera:  # (else the default camera, the command line's)
        tb.snap_to_pixel_centers = True
        tb.sun_dir = [1.0, 1.0, 1.0]
        tb.fov_axis = 0
        tb.relative_focal_length = [100.0 / mc.WIDTH, 100.0 / mc.WIDTH]
        tb.camera_matrix = SLAB_CAMERA
    tb.irradiance_volume_res = 2
    if visibility is not None:
        tb.irradiance_volume_visibility = visibility
    return tb


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    import subprocess
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    scene = _write_slab_scene(tmp_path, hybrid)
    w, h = mc.WIDTH, mc.HEIGHT
    cam = native.make_camera(SLAB_CAMERA, w, h, (100.0, 100.0))
    # the flag off (its default): the frame of the default volume alone, which is what a context without visibility renders
    tb = _testbed(pyngp, scene)
    assert tb.irradiance_volume_visibility is False
    off = tb.render(w, h, 1, True)
    vol = tb.get_irradiance_volume()
    assert vol["sh"].shape == (2, 2, 2, 28)
    with pytest.raises(RuntimeError, match="no irradiance visibility"):
        tb.irradiance_volume_lookup(np.float32([[0.7, 0.5, 0.5]]), np.float32([[1, 0, 0]]), visible=True)
    del tb
    tb = _testbed(pyngp, scene, visibility=False)
    assert tb.render(w, h, 1, True).tobytes() == off.tobytes()
    # the explicit call: the maps' shape, and the lookup is native's
    maps = tb.compute_irradiance_volume_visibility(8, 8, 4, 0.0, 0.01)
    assert maps.shape == (2, 2, 2, 64, 2) and maps.dtype == np.float32 and np.isfinite(maps).all()
    p, n = vc.seeded_points(np.float32(vol["aabb"][0]), np.float32(vol["aabb"][1]), n=200)
    seen = tb.irradiance_volume_lookup(p, n, visible=True)
    assert np.array_equal(tb.irradiance_volume_lookup(p, n, False), tb.irradiance_volume_lookup(p, n)) and not np.array_equal(seen, tb.irradiance_volume_lookup(p, n))
    del tb
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        box = (np.float32(vol["aabb"][0]), np.float32(vol["aabb"][1]))
        c.set_irradiance_volume(vol["sh"], box)
        direct_off = c.render(cam, _opts(native))
        c.compute_irradiance_volume_visibility(8, 8, 4, 0.0, 0.01)
        assert c.get_irradiance_volume_visibility()[1].tobytes() == maps.tobytes()
        assert c.irradiance_volume_at(p, n, visible=True).tobytes() == seen.tobytes()
        c.compute_irradiance_volume_visibility()
        direct_on = c.render(cam, _opts(native))
    finally:
        c.close()
    assert (off[..., 3] > 0).sum() > 500 and off.tobytes() == direct_off.tobytes()
    # the flag on: the default volume gets visibility with the defaults, and the frame changes
    tb = _testbed(pyngp, scene, visibility=True)
    on = tb.render(w, h, 1, True)
    assert np.array_equal(tb.get_irradiance_volume()["sh"], vol["sh"])
    assert tb.render(w, h, 1, True).tobytes() == on.tobytes()
    del tb
    changed = np.abs(on - off).max(-1) > 0
    print("\npyngp: irradiance_volume_visibility changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(on - off).max()))
    assert on.tobytes() == direct_on.tobytes()
    assert changed.sum() > 100
    # the command line writes that frame: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit)
    tb = _testbed(pyngp, scene, visibility=True, camera=False)
    want = tb.render(w, h, 1, True)
    del tb
    exe = pkg("build").build_main()
    out = tmp_path / "shot.png"
    args = [exe, "--no-gui", "--scene", scene, "--render_mode", "ShadeIrradianceVolume", "--irradiance_volume_res", "2", "--width", str(w), "--height", str(h), "--screenshot", str(out)]
    pngs = []
    for flag in ([], ["--irradiance_volume_visibility"]):
        r = subprocess.run(args + flag, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        pngs.append(np.asarray(Image.open(out)).astype(np.int64))
    a = np.clip(want[..., 3:4], 0, 1)
    v = np.clip(np.where(a > 0, want[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
    srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
    expect = np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)
    png = pngs[1]
    assert png.shape == (h, w, 4) and np.abs(png - expect).max() <= 1 and (png != expect).mean() < 0.01, (np.abs(png - expect).max(), (png != expect).mean())
    assert (png[..., 3] > 0).sum() > 100
