"""Marching-cubes mesh extraction (Testbed::compute_marching_cubes_mesh; contract in include/ngp_hip.h): a numpy restatement of the
contract, checked on analytic fields here, and the GPU pipeline checked against it, against the oracle's network and through the files,
pyngp and the command line."""
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg

FOX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fox")


# ------------------------------------------------------------------------------------------ the restatement
def _edge_id(p, q):
    """cube edge between corners p, q (corner c = x + 2y + 4z): 4 axis + u + 2 v, (u, v) the other two coordinates in axis order"""
    a = (p ^ q).bit_length() - 1
    lo = p & q
    o = [(lo >> b) & 1 for b in range(3) if b != a]
    return 4 * a + o[0] + 2 * o[1]


def _face_cycles():
    """the six faces' corners, counter-clockwise about the outward normal"""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for s in (0, 1):
            cs = []
            for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):  # counter-clockwise about +a when (b, c, a) is right-handed: a != 1
                k = [0, 0, 0]
                k[a], k[b], k[c] = s, u, v
                cs.append(k[0] + 2 * k[1] + 4 * k[2])
            out.append(cs[::-1] if (a != 1) != (s == 1) else cs)
    return out


def _build_table():
    """every maximal run of dense corners along a face contributes the segment from the crossing entering it to the crossing leaving
    it; segments join into loops, taken by smallest edge id and fanned from it"""
    table = []
    for case in range(256):
        nxt = {}
        for cs in _face_cycles():
            ins = [(case >> c) & 1 for c in cs]
            if all(ins) or not any(ins):
                continue
            for i in range(4):
                if ins[i] and not ins[i - 1]:
                    j = i
                    while ins[(j + 1) % 4]:
                        j += 1
                    nxt[_edge_id(cs[i - 1], cs[i])] = _edge_id(cs[j % 4], cs[(j + 1) % 4])
        tris, left = [], set(nxt)
        while left:
            s = min(left)
            loop, e = [s], nxt[s]
            left.discard(s)
            while e != s:
                loop.append(e)
                left.discard(e)
                e = nxt[e]
            tris += [(loop[0], loop[k], loop[k + 1]) for k in range(1, len(loop) - 1)]
        table.append(tris)
    return table


TABLE = _build_table()
TT = np.full((256, 5, 3), -1, np.int64)
TN = np.array([len(t) for t in TABLE], np.int64)
for _c, _t in enumerate(TABLE):
    for _k, _tri in enumerate(_t):
        TT[_c, _k] = _tri
POPC = np.array([bin(i).count("1") for i in range(8)], np.int64)


def lattice_positions(q, res, aabb, R=None):
    """lattice coordinates q (n x 3) -> ngp space: R^T (min + (max - min) q / (res - 1)); R 3 x 3 (to_local)"""
    lo, hi = np.asarray(aabb[0], np.float32), np.asarray(aabb[1], np.float32)
    loc = lo + (hi - lo) * (np.asarray(q, np.float32) / (np.asarray(res, np.float32) - np.float32(1)))
    return (loc if R is None else loc @ np.asarray(R, np.float32)).astype(np.float32)


def marching_cubes_ref(d, thresh, aabb, R=None):
    """the contract on a lattice d of shape (rz, ry, rx): V (ngp space) and F"""
    d = np.asarray(d, np.float32)
    rz, ry, rx = d.shape
    res = (rx, ry, rz)
    n = rx * ry * rz
    ins = d > np.float32(thresh)
    cross = np.zeros((rz, ry, rx, 3), bool)
    cross[:, :, :-1, 0] = ins[:, :, :-1] != ins[:, :, 1:]
    cross[:, :-1, :, 1] = ins[:, :-1, :] != ins[:, 1:, :]
    cross[:-1, :, :, 2] = ins[:-1, :, :] != ins[1:, :, :]
    cross = cross.reshape(n, 3)
    vmask = cross[:, 0] * 1 + cross[:, 1] * 2 + cross[:, 2] * 4
    vofs = np.concatenate([[0], np.cumsum(cross.sum(1))[:-1]]).astype(np.int64)
    p, a = np.nonzero(cross)  # point-major, then axis: the vertex order
    df = d.reshape(-1)
    d0, d1 = df[p], df[p + np.array([1, rx, rx * ry])[a]]
    t = (np.float32(thresh) - d0) / (d1 - d0)
    q = np.stack([p % rx, (p // rx) % ry, p // (rx * ry)], 1).astype(np.float32)
    q[np.arange(len(p)), a] += t
    V = lattice_positions(q, res, aabb, R)
    c = np.zeros((rz - 1, ry - 1, rx - 1), np.int64)
    for k in range(8):
        x, y, z = k & 1, (k >> 1) & 1, (k >> 2) & 1
        c |= ins[z:rz - 1 + z, y:ry - 1 + y, x:rx - 1 + x].astype(np.int64) << k
    cz, cy, cx = np.meshgrid(np.arange(rz - 1), np.arange(ry - 1), np.arange(rx - 1), indexing="ij")
    cell = (cx + rx * (cy + ry * cz)).reshape(-1)
    c = c.reshape(-1)
    nt = TN[c]
    cell_r, case_r = np.repeat(cell, nt), np.repeat(c, nt)
    slot = np.arange(len(cell_r)) - np.repeat(np.cumsum(nt) - nt, nt)
    E = TT[case_r, slot]
    ax, u, v = E // 4, E & 1, (E >> 1) & 1
    strides = np.array([1, rx, rx * ry])
    first = np.array([1, 0, 0])[ax]  # the other two axes, in order
    second = np.array([2, 2, 1])[ax]
    owner = cell_r[:, None] + u * strides[first] + v * strides[second]
    F = vofs[owner] + POPC[vmask[owner] & ((1 << ax) - 1)]
    return V, F.astype(np.uint32).reshape(-1, 3)


def mesh_topology(V, F):
    """(watertight, Euler characteristic): every directed edge once and its reverse present"""
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).astype(np.int64)
    key, rkey = e[:, 0] << 32 | e[:, 1], e[:, 1] << 32 | e[:, 0]
    closed = len(np.unique(key)) == len(key) and np.isin(rkey, key).all()
    n_edges = len(np.unique(np.sort(e, 1), axis=0))
    return closed, len(V) - n_edges + len(F)


def signed_volume(V, F):
    v0, v1, v2 = (V[F[:, k]].astype(np.float64) for k in range(3))
    return float(np.einsum("ij,ij->i", v0, np.cross(v1, v2)).sum() / 6.0)


def _axes(res):
    return [(np.arange(r) / (r - 1)).astype(np.float32) for r in res]


def sphere_field(res, r=0.3, c=(0.5, 0.5, 0.5)):
    x, y, z = _axes(res)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return (r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)).astype(np.float32)


def torus_field(res, R=0.28, r=0.12):
    x, y, z = _axes(res)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    q = np.sqrt((X - 0.5) ** 2 + (Y - 0.5) ** 2) - R
    return (r - np.sqrt(q ** 2 + (Z - 0.5) ** 2)).astype(np.float32)


UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


# ------------------------------------------------------------------------------------------ CPU: the restatement on analytic fields
def test_table_is_the_classic_case_set():
    assert TN.max() == 5 and TN[0] == 0 and TN[255] == 0 and TN[1] == 1 and TN.sum() == 820
    for c in range(256):  # complementary cases cut the same edges
        assert sorted(set(TT[c][TT[c] >= 0])) == sorted(set(TT[255 - c][TT[255 - c] >= 0]))


def test_sphere_is_watertight_closed_and_outward():
    res, r = (64, 64, 64), 0.3
    V, F = marching_cubes_ref(sphere_field(res, r), 0.0, UNIT)
    closed, chi = mesh_topology(V, F)
    assert closed and chi == 2
    vol = signed_volume(V, F)
    assert vol > 0, "triangles wind inward"  # outward winding gives a positive volume
    assert abs(vol - 4.0 / 3.0 * np.pi * r ** 3) < 0.01 * 4.0 / 3.0 * np.pi * r ** 3
    assert np.abs(np.linalg.norm(V - 0.5, axis=1) - r).max() < 1.0 / 63
    n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    centre = V[F].mean(1) - 0.5
    assert (np.einsum("ij,ij->i", n, centre) > 0).all()


def test_torus_has_euler_characteristic_zero():
    V, F = marching_cubes_ref(torus_field((64, 64, 64)), 0.0, UNIT)
    closed, chi = mesh_topology(V, F)
    assert closed and chi == 0 and signed_volume(V, F) > 0


def test_vertex_order_and_interpolation_on_a_small_lattice():
    d = np.zeros((2, 2, 3), np.float32)  # rz, ry, rx
    d[0, 0, 1] = 3.0  # one dense point in the middle of the bottom row
    V, F = marching_cubes_ref(d, 1.0, ((0, 0, 0), (2, 1, 1)))
    # owners in linear order: point 0 (+x edge), point 1 (+x, +y, +z edges)
    np.testing.assert_allclose(V, [[1.0 / 3.0, 0, 0], [5.0 / 3.0, 0, 0], [1, 2.0 / 3.0, 0], [1, 0, 2.0 / 3.0]], atol=1e-6)
    assert F.shape == (2, 3) and sorted(set(F.ravel())) == [0, 1, 2, 3]


def test_host_only_context_refuses_every_entry(native):
    ctx = native.Context(-1)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx.density_on_grid(8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx.marching_cubes(np.zeros((4, 4, 4), np.float32), 0.5, UNIT)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx.compute_marching_cubes_mesh(8)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx._mc_mesh(0, 0, False)
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx.save_marching_cubes_mesh("/nonexistent/m.obj")
    with pytest.raises(RuntimeError, match="no HIP device"):
        ctx.marching_cubes_timings()
    ctx.close()


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def mc_ctx(gpu_ctx, native):
    """a context of this module's own: the session's (gpu_ctx, requested for its torch-first initialisation) keeps the model and the
    render box that the modules after this one find"""
    ctx = native.Context(0)
    yield ctx
    ctx.close()


def _assert_same_mesh(got, V, F, extent):
    assert got["F"].shape == F.shape and np.array_equal(got["F"], F)
    assert got["V"].shape == V.shape
    if len(V):
        assert np.abs(got["V"] - V).max() <= 1e-6 * extent


@pytest.mark.gpu
def test_all_256_corner_configurations(mc_ctx, scene_unit):
    mc_ctx.set_model(scene_unit)
    rng = np.random.default_rng(5)
    box = ((0.1, 0.2, 0.3), (0.6, 0.9, 0.5))
    for case in range(256):
        bits = np.array([(case >> k) & 1 for k in range(8)], bool).reshape(2, 2, 2)  # corner x + 2y + 4z -> [z, y, x]
        d = np.where(bits, rng.uniform(0.6, 2.0, bits.shape), rng.uniform(-1.0, 0.4, bits.shape)).astype(np.float32)
        got = mc_ctx.marching_cubes(d, 0.5, box)
        V, F = marching_cubes_ref(d, 0.5, box)
        assert len(F) == TN[case], case
        _assert_same_mesh(got, V, F, 0.7)


@pytest.mark.gpu
def test_random_lattices_with_a_rotated_box(mc_ctx, scene_unit):
    mc_ctx.set_model(scene_unit)
    th = 0.4
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], np.float32)
    mc_ctx.set_render_aabb((0, 0, 0), (1, 1, 1), R)
    try:
        rng = np.random.default_rng(9)
        box = ((-0.3, 0.1, 0.2), (1.4, 0.8, 0.65))
        for res in ((97, 64, 50), (5, 3, 130)):
            d = rng.standard_normal(res[::-1]).astype(np.float32)
            got = mc_ctx.marching_cubes(d, 0.25, box)
            V, F = marching_cubes_ref(d, 0.25, box, R)
            assert len(F) > 1000
            _assert_same_mesh(got, V, F, 1.7)
            again = mc_ctx.marching_cubes(d, 0.25, box)
            assert np.array_equal(again["V"].view(np.uint32), got["V"].view(np.uint32)) and np.array_equal(again["F"], got["F"])
    finally:
        mc_ctx.set_model(scene_unit)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["sphere", "torus"])
def test_analytic_surfaces_on_the_gpu(shape, mc_ctx, scene_unit):
    mc_ctx.set_model(scene_unit)
    res = (70, 64, 66)
    d = sphere_field(res) if shape == "sphere" else torus_field(res)
    got = mc_ctx.marching_cubes(d, 0.0, UNIT)
    V, F = marching_cubes_ref(d, 0.0, UNIT)
    _assert_same_mesh(got, V, F, 1.0)
    closed, chi = mesh_topology(got["V"], got["F"])
    assert closed and chi == (2 if shape == "sphere" else 0) and signed_volume(got["V"], got["F"]) > 0


@pytest.mark.gpu
def test_refusals(mc_ctx, native, scene_unit):
    fresh = native.Context(0)
    with pytest.raises(RuntimeError, match="No network"):
        fresh.compute_marching_cubes_mesh(8)
    fresh.close()
    mc_ctx.set_model(scene_unit)
    for res in (1, 1025, (2, 2, 0)):
        with pytest.raises(RuntimeError, match="resolution"):
            mc_ctx.density_on_grid(res)
    for box in (((0, 0, 0), (1, 0, 1)), ((0, 0, 0), (np.inf, 1, 1)), ((np.nan, 0, 0), (1, 1, 1))):
        with pytest.raises(RuntimeError, match="aabb"):
            mc_ctx.compute_marching_cubes_mesh(8, box)
    for th in (np.nan, np.inf):
        with pytest.raises(RuntimeError, match="thresh"):
            mc_ctx.compute_marching_cubes_mesh(8, None, th)
    mc_ctx.marching_cubes(np.zeros((3, 3, 3), np.float32), 0.5, UNIT)
    with pytest.raises(RuntimeError, match="no normals or colours"):
        mc_ctx._mc_mesh(0, 0, True)


def _lattice_inputs(ctx, res, aabb=None):
    """warped positions of every lattice point, x fastest"""
    d = ctx.get_model()
    R = np.asarray(d.render_aabb_to_local, np.float32).reshape(3, 3).T
    box = aabb if aabb is not None else (tuple(d.render_aabb_min), tuple(d.render_aabb_max))
    k, j, i = np.meshgrid(*[np.arange(r) for r in res[::-1]], indexing="ij")
    q = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float32)
    p = lattice_positions(q, res, box, R)
    lo, hi = np.asarray(d.aabb_min, np.float32), np.asarray(d.aabb_max, np.float32)
    return ((p - lo) / (hi - lo)).astype(np.float32), R, box


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["unit", "linear", "frequency"])
def test_density_on_grid_against_the_oracle(which, mc_ctx, oracle, scene_mod, scene_unit):
    from conftest import _with_bitfield

    if which == "unit":
        sc = scene_unit
    elif which == "linear":
        sc = _with_bitfield(oracle, pkg("synthetic").make_scene(aabb_scale=1, seed=51, log2_hashmap_size=15, cfg=scene_mod.linear_network_config(0)))
    else:
        sc = dict(pkg("synthetic").make_scene(aabb_scale=1, seed=7, cfg=scene_mod.frequency_network_config()))
        sc["density_grid_bitfield"] = scene_unit["density_grid_bitfield"]
    mc_ctx.set_model(sc)
    res = (19, 16, 13)
    box = ((0.05, 0.1, 0.0), (0.95, 0.8, 1.0))
    got = mc_ctx.density_on_grid(res, box).reshape(-1)
    pos01, _, _ = _lattice_inputs(mc_ctx, res, box)
    m = oracle.make_model(sc)
    ref_logit = oracle.network(m, pos01, np.full_like(pos01, 0.5)).astype(np.float32)[:, 3]
    oracle.release(m)
    assert mc_ctx.get_model().density_activation == 3  # exponential
    ref = np.exp(ref_logit)
    # the parity tests' fp16 logit tolerance, carried through exp
    assert np.isfinite(got).all() and (np.abs(got - ref) <= ref * (np.exp(3e-2) - 1) + 1e-30).all()
    mc_ctx.set_model(scene_unit)


def _load(ctx, which, scene_unit):
    """the model, a resolution and a threshold that cuts a large surface through it (the synthetic model's density is a random-weight
    network's: its level is the 80th percentile of the lattice; the fox snapshot's is run.py's default)"""
    if which == "unit":
        ctx.set_model(scene_unit)
        return 96, float(np.quantile(ctx.density_on_grid(96), 0.8))
    ctx.load_snapshot_file(os.path.join(FOX, "fox_base_t16.ingp"))
    return 128, 2.5


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["unit", "fox"])
def test_compute_mesh_end_to_end(which, native, oracle, scene_unit):
    ctx = native.Context(0)
    res, thresh = _load(ctx, which, scene_unit)
    mesh = ctx.compute_marching_cubes_mesh(res, None, thresh)
    V, N, Cc, F = mesh["V"], mesh["N"], mesh["C"], mesh["F"]
    assert len(F) > 500
    lattice = ctx.density_on_grid(res)
    pos01, R, box = _lattice_inputs(ctx, (res,) * 3)
    rV, rF = marching_cubes_ref(lattice, thresh, box, R)
    _assert_same_mesh(mesh, rV, rF, float(np.max(np.asarray(box[1]) - np.asarray(box[0]))))
    # normals: -grad / |grad| of the oracle's density head at the vertices
    sc = ctx.get_scene() if which == "fox" else scene_unit
    if which == "fox":
        grid = np.asarray(sc["density_grid"], np.float16).astype(np.float32)
        sc["density_grid_bitfield"], _ = oracle.density_grid_to_bitfield(grid, sc["max_cascade"])
    d = ctx.get_model()
    lo, hi = np.asarray(d.aabb_min, np.float32), np.asarray(d.aabb_max, np.float32)
    m = oracle.make_model(sc)
    sub = np.arange(0, len(V), max(1, len(V) // 20000))  # (the oracle runs on the host)
    g = oracle.density_gradient(m, ((V[sub] - lo) / (hi - lo)).astype(np.float32)).astype(np.float64) / (hi - lo)
    want = -g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-30)
    assert (np.einsum("ij,ij->i", want, N[sub]) > 0.99).mean() >= 0.99
    # ... and the mesh's own faces, where the lattice resolves the field: on the coarse lattice the network's fine detail (hash-grid cells,
    # ReLU kinks) turns the gradient away from the faces, so the check runs in a box an eighth of a lattice step wide around a point
    # where the field crosses the threshold -- found on a fine lattice along an x edge of the mesh near its middle
    step = (np.asarray(box[1], np.float32) - np.asarray(box[0], np.float32)) / (res - 1)
    near = np.argsort(np.linalg.norm(V - V.mean(0), axis=1))
    x_edge = np.abs(np.round(V[:, 1:] / step[1:] - np.asarray(box[0])[1:] / step[1:]) - (V[:, 1:] - np.asarray(box[0])[1:]) / step[1:]).max(1) < 1e-3
    v = V[next(i for i in near if x_edge[i])]
    lo_x = np.asarray(box[0])[0] + step[0] * np.floor((v[0] - np.asarray(box[0])[0]) / step[0])
    eps = 1e-6 * float(np.max(hi - lo))
    line = ctx.density_on_grid((1024, 2, 2), ((lo_x, v[1] - eps, v[2] - eps), (lo_x + step[0], v[1] + eps, v[2] + eps)))[0, 0]
    k = int(np.nonzero((line[:-1] > thresh) != (line[1:] > thresh))[0][0])
    c = np.array([lo_x + step[0] * (k + 0.5) / 1023, v[1], v[2]], np.float32)
    half = step / 16
    zoom = ctx.compute_marching_cubes_mesh(48, (tuple(c - half), tuple(c + half)), thresh)
    zV, zN, zF = zoom["V"], zoom["N"], zoom["F"]
    assert len(zF) > 100
    fn = np.cross(zV[zF[:, 1]] - zV[zF[:, 0]], zV[zF[:, 2]] - zV[zF[:, 0]]).astype(np.float64)
    vn = np.zeros((len(zV), 3))
    for k in range(3):
        np.add.at(vn, zF[:, k], fn)
    vn /= np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-30)
    cos = np.einsum("ij,ij->i", vn, zN)
    assert (cos > 0.9).mean() >= 0.95, f"normals agree with the faces for {(cos > 0.9).mean():.3f} of the vertices"
    assert np.allclose(np.linalg.norm(N[np.any(N != 0, 1)], axis=1), 1.0, atol=1e-5)
    # colours: sigmoid of the oracle network's rgb logits at (V, normalize(V - 0.5))
    dirs = V[sub] - 0.5
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    logits = oracle.network(m, ((V[sub] - lo) / (hi - lo)).astype(np.float32), ((dirs + 1) * 0.5).astype(np.float32)).astype(np.float32)
    oracle.release(m)
    assert np.abs(Cc[sub] - 1.0 / (1.0 + np.exp(-logits[:, :3]))).max() <= 1e-2
    # raising the threshold keeps every vertex on an edge with an end dense at the lower one
    hi_mesh = ctx.compute_marching_cubes_mesh(res, None, thresh * 4)
    Vh, Fh = marching_cubes_ref(lattice, thresh * 4, box, R)
    _assert_same_mesh(hi_mesh, Vh, Fh, float(np.max(np.asarray(box[1]) - np.asarray(box[0]))))
    flat = lattice.reshape(-1)
    ins = flat > thresh * 4
    cross_pts = []
    for a, st in enumerate((1, res, res * res)):
        idx = np.arange(flat.size)
        coord = [idx % res, (idx // res) % res, idx // (res * res)][a]
        ok = coord < res - 1
        e = idx[ok][ins[idx[ok]] != ins[idx[ok] + st]]
        cross_pts.append(np.maximum(flat[e], flat[e + st]))
    assert all((c > thresh).all() for c in cross_pts) and sum(len(c) for c in cross_pts) == len(hi_mesh["V"])
    ms = ctx.marching_cubes_timings()
    assert all(x > 0 for x in ms)
    ctx.close()


def _read_ply(path):
    with open(path) as f:
        assert f.readline().strip() == "ply" and f.readline().strip() == "format ascii 1.0"
        props, nv, nf = [], 0, 0
        while True:
            line = f.readline().split()
            if line[0] == "end_header":
                break
            if line[0] == "element":
                nv, nf = (int(line[2]), nf) if line[1] == "vertex" else (nv, int(line[2]))
            elif line[0] == "property" and line[1] != "list":
                props.append(line[2])
        rows = [f.readline().split() for _ in range(nv)]
        faces = [f.readline().split() for _ in range(nf)]
    vals = np.asarray(rows, np.float64).reshape(nv, len(props))
    fa = np.asarray(faces, np.int64).reshape(nf, 4)
    assert (fa[:, 0] == 3).all()
    return props, vals, fa[:, 1:]


@pytest.mark.gpu
def test_mesh_files(native, tmp_path):
    meshio = pkg("meshio")
    ctx = native.Context(0)
    ctx.load_snapshot_file(os.path.join(FOX, "fox_base_t16.ingp"))
    ctx.load_training_data(os.path.join(FOX, "transforms_test.json"))
    info = ctx.dataset_info()
    mesh = ctx.compute_marching_cubes_mesh(64)
    V, F = mesh["V"], mesh["F"]
    ds = (V - info["offset"]) / info["scale"]
    obj, ply = str(tmp_path / "m.obj"), str(tmp_path / "m.PLY")
    ctx.save_marching_cubes_mesh(obj)
    ctx.save_marching_cubes_mesh(ply)
    tris = meshio.load_obj(obj)
    assert tris.shape == (len(F), 3, 3)
    np.testing.assert_allclose(tris, ds[F], rtol=1e-6, atol=1e-6 * np.abs(ds).max())
    lines = open(obj).read().splitlines()
    assert sum(l.startswith("vn ") for l in lines) == len(V) and lines[-1].startswith("f ") and "//" in lines[-1]
    props, vals, fa = _read_ply(ply)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(fa, F.astype(np.int64))
    np.testing.assert_allclose(vals[:, :3], ds, rtol=1e-6, atol=1e-6 * np.abs(ds).max())
    np.testing.assert_allclose(vals[:, 3:6], mesh["N"], atol=1e-6)
    assert np.abs(vals[:, 6:] - np.clip(mesh["C"], 0, 1) * 255).max() <= 0.5 + 1e-3
    with pytest.raises(RuntimeError, match=r"\.obj or \.ply"):
        ctx.save_marching_cubes_mesh(str(tmp_path / "m.stl"))
    ctx.close()
    # the project's own mesh loader takes the OBJ
    g = native.Context(0)
    g.load_mesh_file(obj)
    assert g.n_meshes() == 1 and g.mesh_info(0)["n_tris"] == len(F)
    g.close()


@pytest.mark.gpu
def test_pyngp_and_command_line_save_the_same_mesh(tmp_path):
    pyngp = pkg("build").import_pyngp()
    snap = os.path.join(FOX, "fox_base_t16.ingp")
    testbed = pyngp.Testbed()
    testbed.load_snapshot(snap)
    a = str(tmp_path / "py.obj")
    testbed.compute_and_save_marching_cubes_mesh(a, [64, 64, 64])  # scripts/run.py --save_mesh
    assert os.path.getsize(a) > 1000
    d = testbed.compute_marching_cubes_mesh([64, 64, 64])
    assert set(d) == {"V", "N", "C", "F"} and d["F"].shape[1] == 3 and len(d["V"]) == len(d["N"]) == len(d["C"]) > 0
    with pytest.raises(RuntimeError, match="UV"):
        testbed.compute_and_save_marching_cubes_mesh(str(tmp_path / "uv.obj"), [64, 64, 64], generate_uvs_for_obj_file=True)
    exe = pkg("build").build_main()
    b = str(tmp_path / "cli.obj")
    r = subprocess.run([exe, "--snapshot", snap, "--save_mesh", b, "--marching_cubes_res", "64", "--marching_cubes_density_thresh", "2.5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(a).read() == open(b).read()
