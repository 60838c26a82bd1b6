"""The mesh kernels (BVH4 traversal, mesh selection, shadow ray, BRDF, the hemisphere-ray generator's occlusion and the tile sharding of
the mesh pass) against the float64 brute force of mesh_reference.py, on the meshes, rays and frames of mesh_cases.py.

Tolerances: 4 x the deviation of the oracle's plain float32 C from the same reference, per mesh and ray class and per frame (the tables
of mesh_cases.py, measured by test_mesh_reference_cpu.py); no position looser than 1e-4.
"""
import numpy as np
import pytest

import mesh_cases as mc
import mesh_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu_ctx, native):
    """a context of this module's own: the meshes loaded here leave the shared session context alone"""
    c = native.Context(0)
    yield c
    c.close()


def _load(ctx, scene):
    ctx.clear_meshes()
    for tris, center in scene:
        ctx.add_mesh(tris, center)


def _trace_and_check(ctx, name, cls, o, d, expect, meshes, dev, report):
    p, n = ctx.trace_mesh_rays(o, d)
    _, dn, err, t, safe = mc.compare_trace(name, cls, o, d, expect, p, n, meshes, report)
    print(report[-1])
    tol = mc.position_tolerance(dev, t)  # (covers hits and the rays that end at o + 100 d alike)
    bad = np.nonzero(safe & (err > tol))[0]
    assert bad.size == 0, (name, cls, "%d positions off" % bad.size, bad[:5], err[bad[:5]], tol[bad[:5]])
    assert dn <= mc.GPU_FACTOR * mc.ORACLE_DEV_NORMAL, (name, cls, dn)


@pytest.mark.parametrize("name", mc.MESH_NAMES)
def test_trace_matches_brute_force(name, ctx):
    tris, center, convex = mc.meshes()[name]
    T = ref.normalise(tris, center)
    _load(ctx, [(tris, center)])
    report = []
    for cls, (o, d, expect) in mc.ray_classes(name, T, convex).items():
        _trace_and_check(ctx, name, cls, o, d, expect, [T], mc.ORACLE_DEV_POS[name, cls], report)
    ctx.clear_meshes()


def test_trace_follows_the_reference_rule_on_overlapping_boxes(ctx):
    scene = mc.overlap_scene()
    Ts = mc.normalised(scene)
    _load(ctx, scene)
    o, d = mc.overlap_rays(Ts)
    _trace_and_check(ctx, "overlap", "random", o, d, None, Ts, mc.ORACLE_DEV_OVERLAP, [])
    ctx.clear_meshes()


def test_irradiance_rays_stop_at_the_nearest_triangle_of_any_mesh(ctx):
    scene = mc.overlap_scene()
    Ts = mc.normalised(scene)
    _load(ctx, scene)
    pts, nrm = mc.irradiance_points(Ts)
    o, d, t_max = ctx.irradiance_rays(pts, nrm, n_u=4, n_v=4, offset=1e-3, occlude_by_meshes=True)
    o, d, t_max = o.reshape(-1, 3), d.reshape(-1, 3), t_max.reshape(-1)
    unit = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    assert np.all((d.reshape(-1, 16, 3) * unit[:, None]).sum(-1) > 0) and np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    t, unsafe = ref.global_nearest(Ts, o, d)
    assert unsafe.mean() <= mc.UNSAFE_CAP
    safe = ~unsafe
    assert np.array_equal(np.isfinite(t_max)[safe], np.isfinite(t)[safe])
    assert np.all(t_max[safe & ~np.isfinite(t)] == np.inf)
    both = safe & np.isfinite(t)
    assert both.sum() > 500
    tol = mc.position_tolerance(mc.ORACLE_DEV_OVERLAP, t[both])  # (the same two meshes, rays within them)
    assert np.all(np.abs(t_max[both] - t[both]) <= tol), np.abs(t_max[both] - t[both]).max()
    # rays whose nearest blocker the reference's rule would not have looked at (the other mesh's box comes first)
    t_rule, _, _, _, unsafe_rule, _ = ref.reference_rule_hit(Ts, o, d)
    other = both & ~unsafe_rule & (~np.isfinite(t_rule) | (np.abs(np.where(np.isfinite(t_rule), t_rule, 0) - t) > 1e-3))
    print("\nrays %d, blocked %d, blocker outside the first box %d" % (o.shape[0], both.sum(), other.sum()))
    assert other.sum() >= 20
    ctx.clear_meshes()


@pytest.mark.parametrize("name", list(mc.FRAMES))
def test_render_matches_reference(name, ctx, native):
    fr = mc.reference_frame(name)
    assert fr["unsafe"].mean() <= mc.UNSAFE_CAP
    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts(**mc.FRAMES[name])
    cam = native.make_camera(mc.camera_matrix(name), mc.WIDTH, mc.HEIGHT, mc.focal(name))
    img, depth = ctx.render(cam, native.make_opts(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0)), want_depth=True)
    ctx.set_geometry_opts()
    ctx.clear_meshes()
    dd, dc = mc.compare_frame(name, fr, img, depth)
    print("\n%-15s ddepth %.2e  drgb/max(1,|rgb|) %.2e" % (name, dd, dc))
    assert dd <= mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME[name][0] and dc <= mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME[name][1], (dd, dc)
    mc.check_frame_reaches_its_branch(name, fr)


def _tiles(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // 8) * ((w + 7) // 8) + xs // 8, (xs % 8) + 8 * (ys % 8)


def test_mesh_pass_tile_sharding_covers_frame(ctx, native):
    """three shards of a meshes-only frame are the whole frame, byte for byte; so are their tile-packed forms, unpacked by the rule of
    include/ngp_hip.h (local tile q = tile / shard_count at pixels [64 q, 64 q + 64), slot (x & 7) + 8 (y & 7))"""
    import torch

    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts()
    w, h, world = 60, 36, 3  # (a last tile column of 4 pixels, a last tile row of 4)
    cam = native.make_camera(mc.camera_matrix(), w, h, mc.focal())
    kw = dict(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0))
    full, full_depth = ctx.render(cam, native.make_opts(**kw), want_depth=True)
    assert (full[..., 3] == 1).sum() > 500
    tile, slot = _tiles(w, h)
    total, total_depth = np.zeros_like(full), np.zeros_like(full_depth)
    packed, packed_depth = np.zeros_like(full), np.zeros_like(full_depth)
    for r in range(world):
        mine = tile % world == r
        part, part_depth = ctx.render(cam, native.make_opts(shard_index=r, shard_count=world, **kw), want_depth=True)
        assert not np.any(part[~mine])
        total[mine], total_depth[mine] = part[mine], part_depth[mine]
        n = native.load_library().ngp_packed_tiles(w, h, r, world) * 64
        rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
        ctx.render_device(cam, native.make_opts(shard_index=r, shard_count=world, packed_output=True, **kw), rgba.data_ptr(), dep.data_ptr(), None)
        ctx.render_stats()  # synchronises the context's stream
        src = (tile // world) * 64 + slot
        packed[mine], packed_depth[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]]
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes()
    ctx.clear_meshes()
