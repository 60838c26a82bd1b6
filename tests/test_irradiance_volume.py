"""SH9 irradiance volumes (include/ngp_hip.h, "SH9 irradiance volumes"): the sphere-ray generator, the projection, the volume and its
lookup, checked against the float64 restatement in irradiance_sh_reference.py, the brute-force mesh reference and the oracle's trace."""
import numpy as np
import pytest

import irradiance_sh_reference as ref
import mesh_reference as mref
from irradiance_volume_cases import GEN_POINTS, GEN_SHAPES, UNSAFE_CAP, gen_meshes
from conftest import pkg
from test_irradiance_traced import _box_start, _cam_along, _linear, _oracle_payloads

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
ULP = 2.0 ** -24

@pytest.fixture(scope="module")
def ctx(gpu_ctx, native):
    """a context of this module's own: the models and meshes loaded here leave the shared session context alone"""
    c = native.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("nu,nv", GEN_SHAPES)
def test_generator(nu, nv, ctx):
    ctx.clear_meshes()
    p, n, K = GEN_POINTS, GEN_POINTS.shape[0], nu * nv
    o, d, t = ctx.irradiance_sphere_rays(p, nu, nv)
    assert o.shape == (n, K, 3) and d.shape == (n, K, 3) and t.shape == (n, K)
    assert np.abs(d[0] - ref.sphere_dirs(nu, nv)).max() < 1e-6
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1).max() < 1e-6
    assert all(np.array_equal(d[i].view(np.uint32), d[0].view(np.uint32)) for i in range(n))
    assert np.array_equal(o.view(np.uint32), np.repeat(p[:, None, :], K, 1).view(np.uint32))
    assert np.all(t == INF)
    meshes = gen_meshes()
    for tris, c in meshes:
        ctx.add_mesh(tris, c)
    _, d_off, t_off = ctx.irradiance_sphere_rays(p, nu, nv, occlude_by_meshes=False)
    assert np.all(t_off == INF) and np.array_equal(d_off, d)
    o2, d2, t2 = ctx.irradiance_sphere_rays(p, nu, nv)
    ctx.clear_meshes()
    assert np.array_equal(o2, o) and np.array_equal(d2, d)
    want, unsafe = mref.global_nearest([mref.normalise(tris, c) for tris, c in meshes], o2.reshape(-1, 3), d2.reshape(-1, 3))
    assert unsafe.mean() <= UNSAFE_CAP  # (for the float64 directions: test_generator_points_are_unambiguous, without a device)
    got, safe = t2.reshape(-1), ~unsafe
    assert np.array_equal(np.isinf(got)[safe], np.isinf(want)[safe])
    both = safe & np.isfinite(want)
    if K > 1:
        assert both.any() and np.isinf(got).any()
    assert both.sum() == 0 or np.abs(got[both] - want[both]).max() < 1e-4


PROJ_POINTS = np.float32([[0.5, 0.5, 0.5], [0.3, 0.6, 0.45], [0.7, 0.35, 0.55], [0.42, 0.48, 0.78], [0.62, 0.7, 0.3]])


@pytest.mark.parametrize("nu,nv", [(1, 1), (3, 3), (12, 10), (16, 16)])
def test_projection_of_the_traced_rays(nu, nv, ctx, scene_unit):
    """K < 64, K no multiple of 64, n no multiple of the 4 waves of a workgroup; a ring above the points blocks part of every sphere"""
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    ctx.add_mesh(pkg("meshio").torus(32, 16, R=1.0, r=0.3), (0.0, 0.0, 0.9))
    p, K = PROJ_POINTS, nu * nv
    sh, rays = ctx.irradiance_sh_traced(p, nu, nv, return_rays=True)
    _, _, t = ctx.irradiance_sphere_rays(p, nu, nv)
    again = ctx.irradiance_sh_traced(p, nu, nv)
    split = np.concatenate([ctx.irradiance_sh_traced(p[:2], nu, nv), ctx.irradiance_sh_traced(p[2:], nu, nv)])
    ctx.clear_meshes()
    assert sh.shape == (5, 28) and rays.shape == (5, K, 4)
    want = ref.project(rays[..., :3], ref.sphere_dirs(nu, nv)).reshape(5, 27)
    # fp32: a lane sums <= 4 terms and the butterfly adds 6 levels (about 2e-6), Y comes from fp32 directions (about 3e-6); doubled
    bound = 1e-5 * (4 * np.pi / K) * np.abs(rays[..., :3].astype(np.float64)).sum(1)  # (5, 3): per channel
    err = np.abs(sh[:, :27].astype(np.float64) - want).reshape(5, 9, 3)
    print("projection %d x %d: max |dc| = %.3e, max |dc| / bound = %.3f, max |c| = %.3f" % (nu, nv, err.max(), (err / np.maximum(bound[:, None, :], 1e-30)).max(), np.abs(want).max()))
    assert np.all(err <= bound[:, None, :])
    assert np.array_equal(sh[:, 27], np.isinf(t).mean(1).astype(np.float32))
    if K >= 120:  # (the ring, 17 to 29 degrees from the pole, falls between the directions of the two small spheres)
        assert rays[..., :3].max() > 1e-2 and ((sh[:, 27] > 0) & (sh[:, 27] < 1)).any()
    assert np.array_equal(again.view(np.uint32), sh.view(np.uint32))
    assert np.array_equal(split.view(np.uint32), sh.view(np.uint32))


def _oracle_rays(oracle, m, box, o, d):
    """the oracle's trace of the stage's rays, linear premultiplied rgb (n, K, 3). The geometry puts every mesh hit beyond the occupancy
    grid, where no sample lies: cutting a ray there changes nothing, so the uncut trace is exact."""
    oo, dd = o.reshape(-1, 3), d.reshape(-1, 3)
    t0, alive = _box_start(oo, dd, box[0], box[1], np.zeros(oo.shape[0], np.float32))
    rgba, _, _ = oracle.trace_payloads(m, _cam_along(np.zeros(3), np.zeros(3)), _oracle_payloads(oo, dd, t0, alive), oracle.make_opts(capped_skip=True))
    return _linear(oracle, rgba)[:, :3].astype(np.float64).reshape(o.shape)


def _check_against_oracle(ctx, oracle, m, box, p, nu, nv):
    sh, rays = ctx.irradiance_sh_traced(p, nu, nv, return_rays=True)
    o, d, t = ctx.irradiance_sphere_rays(p, nu, nv)
    L = _oracle_rays(oracle, m, box, o, d)
    want = ref.project(L, ref.sphere_dirs(nu, nv)).reshape(-1, 27)
    err = np.abs(sh[:, :27] - want)
    dray = np.abs(rays[..., :3] - L)
    print("coefficients vs oracle: max |dc| = %.3e (max |c| = %.3f); per ray |d rgb|: mean %.3e, max %.3e, rays above 1e-2: %d of %d"
          % (err.max(), np.abs(want).max(), dray.mean(), dray.max(), int((dray.max(-1) > 1e-2).sum()), dray.shape[0] * dray.shape[1]))
    # the project's per-ray bound, mean |d rgba| < 2e-4 (test_caller_rays_match_oracle): 4 pi 1.09 2e-4 = 2.7e-3, doubled for a probe's small sample
    assert err.max() < 5e-3
    assert np.abs(want).max() > 1e-2
    return sh, t


@pytest.mark.parametrize("arch", ["base", "frequency"])
def test_coefficients_match_oracle(arch, ctx, oracle, scene_mod, scene_unit):
    sc = scene_unit if arch == "base" else dict(pkg("synthetic").make_scene(aabb_scale=1, seed=7, cfg=scene_mod.frequency_network_config(n_neurons=128, n_hidden_density=3)),
                                                density_grid_bitfield=scene_unit["density_grid_bitfield"])
    ctx.set_model(sc)
    ctx.clear_meshes()
    m = oracle.make_model(sc)
    rng = np.random.default_rng(2)
    n = 6 if arch == "base" else 4
    p = np.float32([0.5, 0.5, 0.5]) + rng.uniform(-0.45, 0.45, (n, 3)).astype(np.float32)
    nu, nv = (12, 10) if arch == "base" else (8, 8)
    sh, _ = _check_against_oracle(ctx, oracle, m, sc["render_aabb"], p, nu, nv)
    assert np.all(sh[:, 27] == 1)
    if arch == "base":
        # a ball beside the object's grid (x in [1.1, 2.1]) blocks part of the sphere of the points that face it
        mi = pkg("meshio")
        ctx.add_mesh(mi.icosphere(2), (1.1, 0.0, 0.0))
        q = np.float32([[0.8, 0.5, 0.5], [0.7, 0.4, 0.6], [0.9, 0.55, 0.45]])
        h = oracle.mesh_scene([(mi.icosphere(2), (1.1, 0.0, 0.0))])
        lo, hi = oracle.mesh_scene_aabb(h)
        oracle.mesh_scene_destroy(h)
        sh2, t2 = _check_against_oracle(ctx, oracle, m, (lo - 4, hi + 4), q, nu, nv)
        w2 = np.isinf(t2).mean(1)
        assert np.all((w2 > 0) & (w2 < 1)) and np.array_equal(sh2[:, 27], w2.astype(np.float32))
        ctx.clear_meshes()
    oracle.release(m)


def test_sh_truncation(ctx, native, scene_unit):
    """what nine coefficients lose: E from the records against the direct cosine quadrature of the same traced rays"""
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    rng = np.random.default_rng(2)
    p = (0.5 + rng.uniform(-0.45, 0.45, (6, 3))).astype(np.float32)
    nrm = rng.normal(size=(50, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nu = nv = 16
    sh, rays = ctx.irradiance_sh_traced(p, nu, nv, return_rays=True)
    E = native.irradiance_sh_eval(np.repeat(sh, 50, 0), np.tile(nrm, (6, 1))).reshape(6, 50, 3)
    cos = np.maximum(0.0, nrm @ ref.sphere_dirs(nu, nv).T)  # (50, K)
    direct = np.einsum("pkc,nk->pnc", rays[..., :3].astype(np.float64), cos) * (4 * np.pi / (nu * nv))
    rel = float(np.abs(E - direct).max() / direct.max())
    traced = ctx.irradiance_traced(np.repeat(p, 50, 0), np.tile(nrm, (6, 1)).astype(np.float32), n_u=nu, n_v=nv, offset=0.0)[:, :3].reshape(6, 50, 3)
    print("SH9 truncation at 16 x 16: max |E_sh - E_direct| / max E = %.4f (max E = %.4f, min E_sh = %.4f); against irradiance_traced: %.4f"
          % (rel, direct.max(), E.min(), float(np.abs(E - traced).max() / direct.max())))
    assert direct.max() > 1e-2
    assert rel < 0.03  # the oracle alone: 0.0109 on these inputs (0.020 at 12 x 10, 0.0083 at 32 x 32)


def _volume_matches_points(ctx, res, lo, hi, nu, nv):
    ctx.compute_irradiance_volume(res, (lo, hi), nu, nv)
    d, sh = ctx.get_irradiance_volume()
    assert tuple(d.res) == tuple(res) and np.array_equal(np.float32(list(d.aabb_min)), lo) and np.array_equal(np.float32(list(d.aabb_max)), hi)
    assert (d.sh.n_u, d.sh.n_v, d.sh.occlude_by_meshes) == (nu, nv, 1)
    assert sh.shape == (res[2], res[1], res[0], 28)
    want = ctx.irradiance_sh_traced(ref.volume_points(res, lo, hi), nu, nv)
    assert np.array_equal(sh.reshape(-1, 28).view(np.uint32), want.view(np.uint32))
    return sh.reshape(-1, 28)


def test_volume_is_the_traced_probes(ctx, scene_unit):
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    lo, hi = np.float32([0.1, 0.2, 0.15]), np.float32([0.9, 0.8, 0.85])
    sh = _volume_matches_points(ctx, (3, 2, 4), lo, hi, 6, 5)
    assert np.abs(sh[:, :3]).max() > 1e-2 and np.all(sh[:, 27] == 1)
    _volume_matches_points(ctx, (1, 1, 1), lo, hi, 6, 5)
    _volume_matches_points(ctx, (2, 1, 3), lo, hi, 6, 5)
    # 729 probes x 4096 rays = 2.99 M rays: two tracer chunks of whole probes
    res = (9, 9, 9)
    ctx.compute_irradiance_volume(res, (lo, hi), 64, 64)
    big = ctx.get_irradiance_volume()[1].reshape(-1, 28)
    P = ref.volume_points(res, lo, hi)
    for s in (slice(0, 3), slice(510, 515), slice(726, 729)):
        assert np.array_equal(big[s].view(np.uint32), ctx.irradiance_sh_traced(P[s], 64, 64).view(np.uint32))
    ctx.clear_irradiance_volume()


def _random_volume(rng, res, dead_cell):
    """random records in index order, a third of the probes dead, and the eight (or fewer) corners of `dead_cell` dead too"""
    n = res[0] * res[1] * res[2]
    sh = rng.normal(size=(n, 28)).astype(np.float32)
    sh[:, 27] = rng.uniform(0.1, 1.0, n)
    sh[rng.permutation(n)[:n // 3], 27] = 0
    if dead_cell is not None:
        for c in range(8):
            i, j, k = (min(dead_cell[a] + ((c >> a) & 1), res[a] - 1) for a in range(3))
            sh[i + res[0] * (j + res[1] * k), 27] = 0
    return sh


def _points(rng, n, res, lo, hi, cell=None):
    """n points, two thirds in the box and a third outside (clamped onto it), none within 1e-3 of a cell of a cell face; with `cell`: all
    strictly inside that cell"""
    p = np.empty((n, 3))
    for a in range(3):
        cells = max(res[a] - 1, 1)
        i = rng.integers(0, cells, n) if cell is None else np.full(n, cell[a])
        s = (i + rng.uniform(1e-3, 1 - 1e-3, n)) / cells
        if cell is None:
            out = rng.uniform(size=n) < 1 / 3
            s = np.where(out, np.where(rng.uniform(size=n) < 0.5, -rng.uniform(0.05, 2.0, n), 1 + rng.uniform(0.05, 2.0, n)), s)
        p[:, a] = lo[a] + s * (hi[a] - lo[a])
    return p.astype(np.float32)


@pytest.mark.parametrize("res,dead_cell", [((4, 3, 2), (2, 1, 0)), ((2, 1, 3), None), ((1, 1, 1), None)])
def test_lookup_matches_reference(res, dead_cell, ctx, native):
    rng = np.random.default_rng(7)
    lo, hi = np.float32([0.1, -0.3, 0.25]), np.float32([0.9, 0.8, 1.75])
    sh = _random_volume(rng, res, dead_cell)
    if res == (1, 1, 1):
        sh[0, 27] = 0.5
    vol = sh.reshape(res[2], res[1], res[0], 28)
    ctx.set_irradiance_volume(vol, (lo, hi), n_u=3, n_v=2)
    d, back = ctx.get_irradiance_volume()
    assert tuple(d.res) == res and (d.sh.n_u, d.sh.n_v) == (3, 2) and np.array_equal(back.view(np.uint32), vol.view(np.uint32))
    for n in (1, 65, 200):
        p = _points(rng, n, res, lo, hi)
        nrm = (rng.normal(size=(n, 3)) * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)
        got = ctx.irradiance_volume_at(p, nrm)
        E, W = ref.lookup(sh, res, lo, hi, p, nrm)
        scale, _ = ref.lookup(sh, res, lo, hi, p, nrm, absolute=True)
        # fp32 positions at r <= 9 and about 40 flops
        assert np.all(np.abs(got[:, :3] - E) <= 256 * ULP * scale), (np.abs(got[:, :3] - E) / np.maximum(scale, 1e-30)).max() / ULP
        assert np.abs(got[:, 3] - W).max() < 1e-5
        if n == 200 and res != (1, 1, 1):
            assert (W == 0).any() or (W < 0.999).any()  # dead probes took part
    # at a lattice point: the probe's own evaluation
    P = ref.volume_points(res, lo, hi).astype(np.float32)
    live = sh[:, 27] != 0
    nrm = rng.normal(size=(P.shape[0], 3)).astype(np.float32)
    got = ctx.irradiance_volume_at(P[live], nrm[live])
    own = native.irradiance_sh_eval(sh[live], nrm[live])
    scale = np.einsum("nmc,nm->nc", np.abs(sh[live, :27].astype(np.float64)).reshape(-1, 9, 3),
                      ref.A * np.abs(ref.sh9(nrm[live].astype(np.float64) / np.linalg.norm(nrm[live].astype(np.float64), axis=1, keepdims=True))))
    assert np.all(np.abs(got[:, :3] - own) <= 256 * ULP * scale) and np.abs(got[:, 3] - 1).max() < 1e-5
    if dead_cell is not None:
        q = _points(rng, 65, res, lo, hi, cell=dead_cell)
        assert np.all(ctx.irradiance_volume_at(q, rng.normal(size=(65, 3)).astype(np.float32)) == 0)
    if res == (1, 1, 1):
        sh[0, 27] = 0
        ctx.set_irradiance_volume(sh.reshape(1, 1, 1, 28), (lo, hi))
        assert np.all(ctx.irradiance_volume_at(np.float32([[0.5, 0.5, 0.5], [7, 7, 7]]), np.float32([[0, 0, 1], [1, 0, 0]])) == 0)
    ctx.clear_irradiance_volume()
    with pytest.raises(RuntimeError, match="no irradiance volume"):
        ctx.irradiance_volume_at(P[:1], nrm[:1])
    with pytest.raises(RuntimeError, match="no irradiance volume"):
        ctx.get_irradiance_volume()


def test_occlusion(ctx, scene_unit):
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    mi = pkg("meshio")
    # inside a small closed ball around (1.6, 1.6, 1.6), beyond the grid: every ray blocked and nothing to gather before the wall
    ctx.add_mesh(mi.icosphere(2, radius=1.0), (1.1, 1.1, 1.1))
    inside = ctx.irradiance_sh_traced(np.float32([[1.6, 1.6, 1.6]]), 8, 8)
    assert inside.shape == (1, 28) and np.all(inside == 0)
    ctx.clear_meshes()
    # a ring above the points
    rng = np.random.default_rng(9)
    p = np.float32([0.5, 0.5, 0.5]) + rng.uniform(-0.4, 0.4, (40, 3)).astype(np.float32)
    ctx.add_mesh(mi.torus(32, 16, R=1.0, r=0.3), (0.0, 0.0, 0.9))
    occ = ctx.irradiance_sh_traced(p, 8, 8)
    free = ctx.irradiance_sh_traced(p, 8, 8, occlude_by_meshes=False)  # (the same render box: the mesh box)
    ctx.clear_meshes()
    assert ((occ[:, 27] > 0) & (occ[:, 27] < 1)).any() and np.all(free[:, 27] == 1) and free[:, :3].max() > 0
    assert np.all(occ[:, :3] <= free[:, :3] + 1e-6)


def test_refusals_and_pyngp(ctx, native, scene_mod, scene_unit):
    syn = pkg("synthetic")
    p, n = np.float32([[0.5, 0.5, 0.5]]), np.float32([[0, 0, 1]])
    box = (np.float32([0, 0, 0]), np.float32([1, 1, 1]))
    host = native.Context(-1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        host.irradiance_sh_traced(p, 4, 4)
    host.close()
    c2 = native.Context(0)
    with pytest.raises(RuntimeError, match="No network"):
        c2.irradiance_sh_traced(p, 4, 4)
    with pytest.raises(RuntimeError, match="No network"):
        c2.compute_irradiance_volume((2, 2, 2), box, 4, 4)
    cfg = scene_mod.base_network_config()
    cfg["rgb_network"]["n_hidden_layers"] = 1  # configs/nerf/base_1layer.json
    c2.set_model(dict(syn.make_scene(aabb_scale=1, seed=3, log2_hashmap_size=14, cfg=cfg)))
    with pytest.raises(RuntimeError, match="base.json rgb head"):
        c2.irradiance_sh_traced(p, 4, 4)
    with pytest.raises(RuntimeError, match="base.json rgb head"):
        c2.compute_irradiance_volume((2, 2, 2), box, 4, 4)
    c2.set_model(scene_unit)
    for bad in ([[np.nan, 0, 0]], [[0, np.inf, 0]]):
        with pytest.raises(RuntimeError, match="position 0"):
            c2.irradiance_sh_traced(np.float32(bad), 4, 4)
        with pytest.raises(RuntimeError, match="position 0"):
            c2.irradiance_sphere_rays(np.float32(bad), 4, 4)
    for kw in ({"n_u": 0, "n_v": 4}, {"n_u": 4, "n_v": 0}):
        with pytest.raises(RuntimeError, match="n_u and n_v"):
            c2.irradiance_sh_traced(p, **kw)
        with pytest.raises(RuntimeError, match="n_u and n_v"):
            c2.irradiance_sphere_rays(p, **kw)
        with pytest.raises(RuntimeError, match="n_u and n_v"):
            c2.compute_irradiance_volume((2, 2, 2), box, **kw)
    with pytest.raises(RuntimeError, match="too large"):
        c2.irradiance_sh_traced(p, 1 << 11, 1 << 11)  # a probe of more than 2^21 rays
    with pytest.raises(RuntimeError, match="too large"):
        c2.irradiance_sh_traced(np.repeat(p, 129, 0), 1 << 11, 1 << 10)  # more than 2^28 rays
    with pytest.raises(RuntimeError, match="too large"):
        c2.compute_irradiance_volume((1000, 1000, 1000), box, 4, 4)
    with pytest.raises(RuntimeError, match="too large"):
        c2.compute_irradiance_volume((64, 64, 64), box, 64, 64)
    with pytest.raises(RuntimeError, match="resolution"):
        c2.compute_irradiance_volume((2, 0, 2), box, 4, 4)
    with pytest.raises(RuntimeError, match="min < max"):
        c2.compute_irradiance_volume((2, 2, 2), (box[0], np.float32([1, 0, 1])), 4, 4)
    with pytest.raises(RuntimeError, match="not finite"):
        c2.compute_irradiance_volume((2, 2, 2), (box[0], np.float32([1, np.inf, 1])), 4, 4)
    with pytest.raises(RuntimeError, match="extent is not finite"):  # (finite corners whose difference overflows a float)
        c2.compute_irradiance_volume((2, 2, 2), (np.float32([-3e38, 0, 0]), np.float32([3e38, 1, 1])), 4, 4)
    with pytest.raises(RuntimeError, match="no irradiance volume"):
        c2.irradiance_volume_at(p, n)
    with pytest.raises(RuntimeError, match="no irradiance volume"):
        c2.get_irradiance_volume()
    vol = np.ones((2, 2, 2, 28), np.float32)
    for bad in (np.nan, np.inf):
        v = vol.copy()
        v[1, 0, 1, 5] = bad
        with pytest.raises(RuntimeError, match="value 5 of probe 5 is not finite"):
            c2.set_irradiance_volume(v, box)
    with pytest.raises(RuntimeError, match="resolution|min < max"):
        c2.set_irradiance_volume(vol, (box[1], box[0]))
    with pytest.raises(RuntimeError, match="extent is not finite"):
        c2.set_irradiance_volume(vol, (np.float32([0, -2e38, 0]), np.float32([1, 2e38, 1])))
    # a huge box and huge positions stay inside the lattice: the far corner's own record
    c2.set_irradiance_volume(vol, (np.float32([-1e38] * 3), np.float32([1e38] * 3)))
    far = c2.irradiance_volume_at(np.float32([[3e38, -3e38, 3e38], [0, 0, 0]]), np.float32([[0, 0, 1], [0, 0, 1]]))
    assert np.all(np.isfinite(far)) and np.all(far[:, 3] == 1) and np.array_equal(far[0], far[1])
    c2.set_irradiance_volume(vol, box)
    with pytest.raises(RuntimeError, match="position 0"):
        c2.irradiance_volume_at(np.float32([[np.nan, 0, 0]]), n)
    for bad in ([[0, 0, 0]], [[np.nan, 0, 1]]):
        with pytest.raises(RuntimeError, match="normal 0"):
            c2.irradiance_volume_at(p, np.float32(bad))
    c2.close()
    # pyngp: the Testbed methods return what the Context methods return
    pyngp = pkg("build").import_pyngp()
    import os
    import tempfile

    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    with tempfile.TemporaryDirectory() as td:
        snap = os.path.join(td, "s.ingp")
        ctx.save_snapshot_file(snap)
        tb = pyngp.Testbed()
        tb.load_file(snap)
        rng = np.random.default_rng(1)
        q = np.float32([0.5, 0.5, 0.5]) + rng.uniform(-0.3, 0.3, (7, 3)).astype(np.float32)
        got = tb.compute_irradiance_sh_at_points(q, 8, 6, True)
        assert got.shape == (7, 28) and np.array_equal(got, ctx.irradiance_sh_traced(q, 8, 6))
        ra = np.float32(tb.render_aabb)
        vol = tb.compute_irradiance_volume([3, 2, 2], None, 6, 5, True)
        ctx.compute_irradiance_volume((3, 2, 2), (ra[:3], ra[3:]), 6, 5)
        assert vol["sh"].shape == (2, 2, 3, 28) and np.array_equal(vol["sh"], ctx.get_irradiance_volume()[1])
        assert np.array_equal(np.float32(vol["aabb"][0]), ra[:3]) and np.array_equal(np.float32(vol["aabb"][1]), ra[3:])
        sub = tb.compute_irradiance_volume([2, 2, 2], (0.2, 0.2, 0.2, 0.8, 0.8, 0.8), 6, 5, False)
        ctx.compute_irradiance_volume((2, 2, 2), (np.float32([0.2] * 3), np.float32([0.8] * 3)), 6, 5, occlude_by_meshes=False)
        assert np.array_equal(sub["sh"], ctx.get_irradiance_volume()[1])
        nq = rng.normal(size=(7, 3)).astype(np.float32)
        E = tb.irradiance_volume_lookup(q, nq)
        assert E.shape == (7, 4) and np.array_equal(E, ctx.irradiance_volume_at(q, nq)) and E[:, :3].max() > 0
    ctx.clear_irradiance_volume()
