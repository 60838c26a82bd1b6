"""Traced irradiance (include/ngp_hip.h, "traced irradiance"): caller rays through the NeRF, the hemisphere ray generator and the
estimate E(p, n) = (pi / K) sum_k rgb_k, checked against the oracle, exact geometric properties and the probes."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def ctx(gpu_ctx, native):
    """a context of this module's own: the models and meshes loaded here leave the shared session context alone"""
    c = native.Context(0)
    yield c
    c.close()


def _cam_along(o, d):
    """a camera matrix (column-major 3 x 4) at o whose forward axis is d: the oracle's depth is then the distance along the ray"""
    m = np.zeros(12, np.float32)
    m[6:9], m[9:12] = d, o
    return m


def _box_start(o, d, lo, hi, t_min):
    """the contract's t_start (entry + 1e-6 for an origin outside the box, 0 inside) and alive"""
    lo, hi = np.float32(lo), np.float32(hi)
    inside = np.all((o >= lo) & (o <= hi), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (lo - o) / d, (hi - o) / d
    tmin, tmax = np.minimum(a, b).max(1), np.maximum(a, b).min(1)
    hit = (tmin <= tmax) & (tmin > 0)
    entry = np.where(inside, 0.0, tmin + np.float32(1e-6)).astype(np.float32)
    alive = inside | hit
    return np.maximum(t_min, entry).astype(np.float32), alive


def _rays(rng, n, lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    c, ext = (lo + hi) / 2, hi - lo
    o = np.empty((n, 3), np.float32)
    k = n // 2
    o[:k] = rng.uniform(lo, hi, (k, 3))                                     # inside the box
    u = rng.normal(size=(n - k, 3))
    o[k:] = c + 0.9 * ext.max() * u / np.linalg.norm(u, axis=1, keepdims=True)  # outside, looking roughly inwards (some miss)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[k:] = (c - o[k:]) / np.linalg.norm(c - o[k:], axis=1, keepdims=True) + 0.6 * d[k:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t_min = np.where(rng.uniform(size=n) < 0.25, rng.uniform(0, 0.4 * ext.max(), n), 0).astype(np.float32)
    return o, d.astype(np.float32), t_min


def _linear(oracle, rgba):
    """the probe rule on the oracle's trace: an sRGB-trained network's rgb is linearised (shaded rays only, alpha > 0.001)"""
    out = rgba.copy()
    f = np.vectorize(oracle.lib.orc_srgb_to_linear, otypes=[np.float32])
    sh = rgba[:, 3] > 0.001
    out[sh, :3] = f(rgba[sh, :3])
    out[~sh] = 0
    return out


def _oracle_payloads(o, d, t, alive):
    import oracle as orc

    pl = np.zeros(o.shape[0], orc.PAYLOAD_DTYPE)
    pl["origin"], pl["dir"], pl["t"], pl["alive"] = o, d, t, alive
    pl["idx"] = np.arange(o.shape[0])
    return pl


@pytest.mark.parametrize("which", ["scene_unit", "scene_big"])
def test_caller_rays_match_oracle(which, request, ctx, oracle):
    sc = request.getfixturevalue(which)
    ctx.set_model(sc)
    ctx.clear_meshes()
    m = oracle.make_model(sc)
    lo, hi = sc["render_aabb"]
    rng = np.random.default_rng(11)
    o, d, t_min = _rays(rng, 3000, lo, hi)
    rgba, depth = ctx.trace_nerf_rays(o, d, np.stack([t_min, np.full_like(t_min, INF)], 1))
    st = ctx.render_stats()
    t0, alive = _box_start(o, d, lo, hi, t_min)
    assert 0.2 < alive.mean() < 0.98
    ref, _, ost = oracle.trace_payloads(m, _cam_along(np.zeros(3), np.zeros(3)), _oracle_payloads(o, d, t0, alive), oracle.make_opts(capped_skip=True))
    ref = _linear(oracle, ref)
    assert st["n_rays"] == 3000 and ost["n_samples"] > 0
    assert abs(int(st["n_samples"]) - int(ost["n_samples"])) <= 2e-3 * ost["n_samples"] + 2
    # (aabb_scale 4: exponential stepping puts a few samples where fp16 network outputs differ most; measured max 0.020 on one ray)
    assert np.abs(rgba - ref).max() < (1e-2 if which == "scene_unit" else 3e-2) and np.abs(rgba - ref).mean() < 2e-4
    assert (np.abs(rgba - ref).max(1) < 1e-2).mean() > 0.999
    assert np.all(rgba[~alive] == 0)
    assert (rgba[:, 3] > 0.2).sum() > 100
    # depth: the distance of the sample of largest weight; two nearly equal weights may swap on a rare ray (measured: 1 in 300 on scene_big)
    deep = np.nonzero((rgba[:, 3] > 0.2) & (ref[:, 3] > 0.2))[0][:300]
    ok = []
    for i in deep:
        _, dref, _ = oracle.trace_payloads(m, _cam_along(o[i], d[i]), _oracle_payloads(o[i:i + 1], d[i:i + 1], t0[i:i + 1], alive[i:i + 1]),
                                           oracle.make_opts(capped_skip=True))
        ok.append(abs(depth[i] - dref[0]) < 1e-3 * max(1.0, abs(dref[0])) + 2e-3)
    assert len(ok) > 100 and np.mean(ok) > 0.98
    oracle.release(m)


def test_t_max(ctx, scene_unit):
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    rng = np.random.default_rng(3)
    n = 512
    o = np.float32([0.5, 0.5, -0.8]) + rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    d = np.tile(np.float32([0, 0, 1]), (n, 1)) + rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
    inf, _ = ctx.trace_nerf_rays(o, d)
    assert (inf[:, 3] > 0.2).sum() > 50
    far, _ = ctx.trace_nerf_rays(o, d, np.tile(np.float32([0, 50.0]), (n, 1)))  # beyond the box exit
    assert np.array_equal(far, inf)
    near, _ = ctx.trace_nerf_rays(o, d, np.tile(np.float32([0, 0.8]), (n, 1)))  # ends at the box face, before any occupied cell
    assert np.all(near == 0)
    prev = np.zeros(n, np.float32)
    for tm in np.linspace(0.8, 2.2, 8):
        a, _ = ctx.trace_nerf_rays(o, d, np.tile(np.float32([0, tm]), (n, 1)))
        assert np.all(a[:, 3] >= prev)
        prev = a[:, 3]


def _normals(rng, n):
    v = rng.normal(size=(n, 3)).astype(np.float32)
    v[:4] = [[0, 0, 1], [0, 0, -1], [0, 0, 3], [1e-3, 0, -1]]  # local_frame switches sign at z = 0
    return v


def test_generator(ctx, oracle, scene_unit):
    ctx.clear_meshes()
    rng = np.random.default_rng(5)
    n, nu, nv = 24, 8, 6
    p = rng.uniform(-1, 2, (n, 3)).astype(np.float32)
    nrm = _normals(rng, n)
    o, d, t = ctx.irradiance_rays(p, nrm, n_u=nu, n_v=nv, offset=1e-3)
    nh = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(d, axis=2) - 1).max() < 1e-6
    a = (np.arange(nu) + 0.5) / nu
    cos = np.einsum("nkc,nc->nk", d, nh).reshape(n, nv, nu)
    assert np.abs(cos - np.sqrt(1 - a)[None, None, :]).max() < 1e-6
    # azimuths equally spaced: within one u, consecutive v differ by 2 pi / n_v around n
    tang = d - np.einsum("nk,nc->nkc", np.einsum("nkc,nc->nk", d, nh), nh)
    tang = tang.reshape(n, nv, nu, 3)
    tang /= np.linalg.norm(tang, axis=3, keepdims=True)
    cosdiff = (tang * np.roll(tang, -1, axis=1)).sum(3)
    assert np.abs(cosdiff - np.cos(2 * np.pi / nv)).max() < 1e-5
    assert np.abs(o - (p + 1e-3 * nh)[:, None, :]).max() < 1e-6
    mean = d.mean(1)
    assert np.abs(mean - 2 / 3 * nh).max() < 0.03  # (stratification error at 8 x 6)
    assert np.all(t == INF)
    # t_max: the closest hit over all meshes, against the oracle's trace_mesh over one-mesh scenes
    mi = pkg("meshio")
    meshes = [(mi.icosphere(2), (0.0, 0.0, 0.0)), (mi.torus(24, 12, R=1.0, r=0.2), (0.3, 0.1, 0.0))]
    for tris, c in meshes:
        ctx.add_mesh(tris, c)
    q = rng.uniform(-0.6, 0.6, (16, 3)).astype(np.float32) + 0.5
    nq = _normals(rng, 16)
    o, d, t = ctx.irradiance_rays(q, nq, n_u=6, n_v=6, offset=0.0)
    oo, dd = o.reshape(-1, 3), d.reshape(-1, 3)
    best = np.full(oo.shape[0], np.inf)
    for mesh in meshes:
        h = oracle.mesh_scene([mesh])
        hp, _ = oracle.trace_mesh(h, oo, dd)
        dist = np.einsum("kc,kc->k", hp - oo, dd)
        moved = np.abs(hp - oo).max(1) > 0
        ok = moved & (dist < 99.0)
        best = np.where(ok & (dist < best), dist, best)
        oracle.mesh_scene_destroy(h)
    t = t.reshape(-1)
    assert np.isinf(t).any() and np.isfinite(t).any()
    assert np.array_equal(np.isinf(t), np.isinf(best))
    fin = np.isfinite(t)
    assert np.abs(t[fin] - best[fin]).max() < 1e-4
    _, _, t_off = ctx.irradiance_rays(q, nq, n_u=6, n_v=6, offset=0.0, occlude_by_meshes=False)
    assert np.all(t_off == INF)
    ctx.clear_meshes()


def _restated(oracle, m, box, o, d, t, K):
    """(pi / K) sum rgb of the oracle's trace of the generator's rays. The geometry puts every mesh hit beyond the occupancy grid, where
    no sample lies: cutting a ray there changes nothing, so the uncut trace is exact."""
    oo, dd, tt = o.reshape(-1, 3), d.reshape(-1, 3), t.reshape(-1)
    t0, alive = _box_start(oo, dd, box[0], box[1], np.zeros(oo.shape[0], np.float32))
    rgba, _, _ = oracle.trace_payloads(m, _cam_along(np.zeros(3), np.zeros(3)), _oracle_payloads(oo, dd, t0, alive), oracle.make_opts(capped_skip=True))
    E = _linear(oracle, rgba)[:, :3].astype(np.float64).reshape(-1, K, 3).sum(1) * (np.pi / K)
    w = np.isinf(tt).reshape(-1, K).mean(1)
    return E, w


@pytest.mark.parametrize("arch", ["base", "frequency"])
def test_estimate_matches_restatement(arch, ctx, oracle, scene_mod, scene_unit):
    sc = scene_unit if arch == "base" else dict(pkg("synthetic").make_scene(aabb_scale=1, seed=7, cfg=scene_mod.frequency_network_config(n_neurons=128, n_hidden_density=3)),
                                                density_grid_bitfield=scene_unit["density_grid_bitfield"])
    ctx.set_model(sc)
    ctx.clear_meshes()
    m = oracle.make_model(sc)
    rng = np.random.default_rng(2)
    n = 6 if arch == "base" else 4
    p = np.float32([0.5, 0.5, 0.5]) + rng.uniform(-0.45, 0.45, (n, 3)).astype(np.float32)
    nrm = _normals(rng, n)
    nu, nv = (12, 10) if arch == "base" else (8, 8)
    K = nu * nv
    E = ctx.irradiance_traced(p, nrm, n_u=nu, n_v=nv)
    o, d, t = ctx.irradiance_rays(p, nrm, n_u=nu, n_v=nv)
    Eref, w = _restated(oracle, m, sc["render_aabb"], o, d, t, K)
    assert np.all(E[:, 3] == 1) and np.abs(E[:, :3] - Eref).max() < 1e-3
    assert E[:, :3].max() > 1e-2
    if arch == "base":
        # with meshes: a ball beside the object's grid (x in [1.1, 2.1]; add_mesh centres a mesh at 0.5 + center) blocks part of
        # the hemisphere of points that face it
        mi = pkg("meshio")
        ctx.add_mesh(mi.icosphere(2), (1.1, 0.0, 0.0))
        q = np.float32([[0.8, 0.5, 0.5], [0.7, 0.4, 0.6], [0.9, 0.55, 0.45]])
        nq = np.float32([[1, 0, 0], [1, 0.2, 0], [1, -0.1, 0.3]])
        E2 = ctx.irradiance_traced(q, nq, n_u=nu, n_v=nv)
        o, d, t = ctx.irradiance_rays(q, nq, n_u=nu, n_v=nv)
        h = oracle.mesh_scene([(mi.icosphere(2), (1.1, 0.0, 0.0))])
        lo, hi = oracle.mesh_scene_aabb(h)
        oracle.mesh_scene_destroy(h)
        Eref2, w2 = _restated(oracle, m, (lo - 4, hi + 4), o, d, t, K)
        assert np.all(E2[:, 3] == w2.astype(np.float32)) and np.all((w2 > 0) & (w2 < 1))
        assert np.abs(E2[:, :3] - Eref2).max() < 1e-3
        ctx.clear_meshes()
    oracle.release(m)


def test_exact_geometric_properties(ctx, scene_unit):
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    mi = pkg("meshio")
    ico = mi.icosphere(2, radius=1.0)
    ctx.add_mesh(ico)  # a ball of diameter ~1 around the object's centre (0.5, 0.5, 0.5)
    _, tris = ctx.mesh_bvh(0)
    T = np.stack([tris["a"], tris["b"], tris["c"]], 1).astype(np.float32)
    cen = T.mean(1)
    fn = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    fn *= np.sign(np.einsum("kc,kc->k", fn, cen - cen.mean(0)))[:, None]  # outward
    fn = (fn / np.linalg.norm(fn, axis=1, keepdims=True)).astype(np.float32)
    sel = np.arange(0, cen.shape[0], 7)
    with_mesh = ctx.irradiance_traced(cen[sel], fn[sel], n_u=8, n_v=8, offset=1e-4)
    assert np.all(with_mesh[:, 3] == 1) and with_mesh[:, :3].max() > 0
    ctx.clear_meshes()
    # a convex mesh blocks none of its own outward rays, and beyond the grid there is nothing to gather: the mesh changes nothing
    assert np.array_equal(ctx.irradiance_traced(cen[sel], fn[sel], n_u=8, n_v=8, offset=1e-4), with_mesh)
    # a point inside a small closed mesh: every ray blocked, and nothing to gather before the wall (the ball, around (1.6, 1.6, 1.6),
    # lies beyond the grid)
    ctx.add_mesh(ico, (1.1, 1.1, 1.1))
    inside = ctx.irradiance_traced(np.float32([[1.6, 1.6, 1.6]]), np.float32([[0, 0, 1]]), n_u=8, n_v=8)
    assert np.all(inside == 0)
    ctx.clear_meshes()


def test_occluder_and_determinism(ctx, scene_unit):
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    mi = pkg("meshio")
    rng = np.random.default_rng(9)
    p = np.float32([0.5, 0.5, 0.5]) + rng.uniform(-0.4, 0.4, (40, 3)).astype(np.float32)
    nrm = rng.normal(size=(40, 3)).astype(np.float32)
    ctx.add_mesh(mi.torus(32, 16, R=1.0, r=0.3), (0.0, 0.0, 0.9))  # a ring above the points
    occ = ctx.irradiance_traced(p, nrm, n_u=8, n_v=8)
    free = ctx.irradiance_traced(p, nrm, n_u=8, n_v=8, occlude_by_meshes=False)  # (the same render box: the mesh box)
    assert ((occ[:, 3] > 0) & (occ[:, 3] < 1)).any() and np.all(free[:, 3] == 1) and free[:, :3].max() > 0
    assert np.all(occ[:, :3] <= free[:, :3] + 1e-6)
    assert np.array_equal(occ, ctx.irradiance_traced(p, nrm, n_u=8, n_v=8))
    split = np.concatenate([ctx.irradiance_traced(p[:13], nrm[:13], n_u=8, n_v=8), ctx.irradiance_traced(p[13:], nrm[13:], n_u=8, n_v=8)])
    assert np.array_equal(split, occ)
    ctx.clear_meshes()
    # a request of several 2^21-ray chunks equals the same points in small calls
    q = np.float32([0.5, 0.5, 0.5]) + rng.uniform(-0.45, 0.45, (9000, 3)).astype(np.float32)
    nq = rng.normal(size=(9000, 3)).astype(np.float32)
    big = ctx.irradiance_traced(q, nq, n_u=16, n_v=16)
    for s in (slice(0, 50), slice(8150, 8250), slice(8950, 9000)):
        assert np.array_equal(big[s], ctx.irradiance_traced(q[s], nq[s], n_u=16, n_v=16))
    # and caller rays: chunked once, traced one chunk per call
    o = np.repeat(q[:1], 5, 0)
    d = nq[:5]
    one, _ = ctx.trace_nerf_rays(o, d)
    o2 = np.concatenate([np.repeat(q[:1], (1 << 21) + 5, 0)])
    d2 = np.concatenate([np.tile(d[:1], ((1 << 21), 1)), d])
    many, _ = ctx.trace_nerf_rays(o2, d2)
    assert np.array_equal(many[-5:], one) and np.array_equal(many[:3], np.repeat(one[:1], 3, 0))


def test_consistent_with_the_probes(ctx, scene_unit):
    """the centre probe's E(n) against the traced estimate at the render-box centre (no meshes): the probes' quadrature error"""
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    rng = np.random.default_rng(4)
    nrm = rng.normal(size=(24, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    c = np.tile(np.float32([0.5, 0.5, 0.5]), (24, 1))
    errs = []
    for (k, nt, nph) in ((16, 64, 32), (64, 256, 128)):
        E = ctx.irradiance_traced(c, nrm, n_u=k, n_v=k, offset=0.0)[:, :3]
        ctx.compute_envmap(0, nt, nph)
        P = ctx.irradiance(nrm)
        errs.append(float(np.abs(E - P).max() / np.abs(P).max()))
    print("traced vs probe, max |dE| / max E: coarse %.4f, fine %.4f" % tuple(errs))
    assert errs[1] < errs[0] and errs[1] < 0.02  # measured: coarse 0.042, fine 0.011


def test_refusals_and_pyngp(ctx, native, scene_mod, scene_unit):
    syn = pkg("synthetic")
    c2 = native.Context(0)
    p, n = np.float32([[0.5, 0.5, 0.5]]), np.float32([[0, 0, 1]])
    with pytest.raises(RuntimeError, match="No network"):
        c2.irradiance_traced(p, n)
    with pytest.raises(RuntimeError, match="No network"):
        c2.trace_nerf_rays(p, n)
    cfg = scene_mod.base_network_config()
    cfg["rgb_network"]["n_hidden_layers"] = 1  # configs/nerf/base_1layer.json
    c2.set_model(dict(syn.make_scene(aabb_scale=1, seed=3, log2_hashmap_size=14, cfg=cfg)))
    with pytest.raises(RuntimeError, match="base.json rgb head"):
        c2.irradiance_traced(p, n)
    with pytest.raises(RuntimeError, match="base.json rgb head"):
        c2.trace_nerf_rays(p, n)
    c2.set_model(scene_unit)
    for bad in ([[0, 0, 0]], [[np.nan, 0, 1]]):
        with pytest.raises(RuntimeError, match="normal 0"):
            c2.irradiance_traced(p, np.float32(bad))
        with pytest.raises(RuntimeError, match="direction 0"):
            c2.trace_nerf_rays(p, np.float32(bad))
    with pytest.raises(RuntimeError, match="origin 0"):
        c2.trace_nerf_rays(np.float32([[np.inf, 0, 0]]), n)
    with pytest.raises(RuntimeError, match="position 0"):
        c2.irradiance_traced(np.float32([[np.nan, 0, 0]]), n)
    for kw in ({"n_u": 0}, {"n_v": 0}):
        with pytest.raises(RuntimeError, match="n_u and n_v"):
            c2.irradiance_traced(p, n, **kw)
    for off in (-1e-3, np.inf, np.nan):
        with pytest.raises(RuntimeError, match="offset"):
            c2.irradiance_traced(p, n, offset=off)
    with pytest.raises(RuntimeError, match="too large"):
        c2.irradiance_traced(np.repeat(p, 5, 0), np.repeat(n, 5, 0), n_u=1 << 14, n_v=1 << 13)
    c2.close()
    # pyngp: the Testbed method returns what Context.irradiance_traced returns
    pyngp = pkg("build").import_pyngp()
    import tempfile, os
    ctx.set_model(scene_unit)
    ctx.clear_meshes()
    with tempfile.TemporaryDirectory() as td:
        snap = os.path.join(td, "s.ingp")
        ctx.save_snapshot_file(snap)
        tb = pyngp.Testbed()
        tb.load_file(snap)
        rng = np.random.default_rng(1)
        q = np.float32([0.5, 0.5, 0.5]) + rng.uniform(-0.3, 0.3, (20, 3)).astype(np.float32)
        nq = rng.normal(size=(20, 3)).astype(np.float32)
        got = tb.compute_irradiance_at_points(q, nq, 8, 8, 1e-4, True)
        want = ctx.irradiance_traced(q, nq, n_u=8, n_v=8, offset=1e-4)
        assert got.shape == (20, 4) and np.array_equal(got, want)
