"""SH9 irradiance volumes without a GPU: the descriptors' layout, the refusals of a host-only context, the host evaluation against the
float64 reference, and the reference's own quadrature bias."""
import numpy as np
import pytest

import irradiance_sh_reference as ref
import mesh_reference as mref
from irradiance_volume_cases import GEN_POINTS, GEN_SHAPES, UNSAFE_CAP, gen_meshes


def test_volume_desc_layouts(native):
    C = native.C
    s = native.IrradianceShDesc
    assert [f for f, _ in s._fields_] == ["n_u", "n_v", "min_transmittance", "occlude_by_meshes"]
    assert C.sizeof(s) == 16 and [getattr(s, f).offset for f, _ in s._fields_] == [0, 4, 8, 12]
    v = native.IrradianceVolumeDesc
    assert [f for f, _ in v._fields_] == ["res", "aabb_min", "aabb_max", "sh"]
    assert C.sizeof(v) == 52 and [getattr(v, f).offset for f, _ in v._fields_] == [0, 12, 24, 36]
    # the header declares the same members in the same order
    import re

    with open(native.HEADER_PATH) as f:
        h = f.read()
    body = re.search(r"typedef struct ngp_irradiance_sh_desc \{(.*?)\} ngp_irradiance_sh_desc;", h, re.S).group(1)
    assert re.findall(r"\b(n_u|n_v|min_transmittance|occlude_by_meshes)\b(?=[,;])", body) == ["n_u", "n_v", "min_transmittance", "occlude_by_meshes"]
    body = re.search(r"typedef struct ngp_irradiance_volume_desc \{(.*?)\} ngp_irradiance_volume_desc;", h, re.S).group(1)
    assert re.findall(r"\b(res|aabb_min|aabb_max|sh)\b(?=\[3\]|;)", body) == ["res", "aabb_min", "aabb_max", "sh"]


def test_volume_entries_refuse_host_only(native):
    L = native.load_library()
    names = ("ngp_irradiance_sphere_rays", "ngp_irradiance_sh_traced", "ngp_irradiance_sh_eval", "ngp_compute_irradiance_volume", "ngp_get_irradiance_volume",
             "ngp_set_irradiance_volume", "ngp_clear_irradiance_volume", "ngp_irradiance_volume_at")
    for name in names:
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    p, n = np.float32([[0.5, 0.5, 0.5]]), np.float32([[0.0, 0.0, 1.0]])
    box = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    calls = [lambda: ctx.irradiance_sphere_rays(p, 4, 4), lambda: ctx.irradiance_sh_traced(p, 4, 4), lambda: ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4),
             lambda: ctx.get_irradiance_volume(), lambda: ctx.set_irradiance_volume(np.ones((1, 1, 1, 28), np.float32), box), lambda: ctx.clear_irradiance_volume(),
             lambda: ctx.irradiance_volume_at(p, n)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    ctx.close()


def test_sh_eval_matches_reference(native):
    rng = np.random.default_rng(0)
    sh = rng.normal(size=(64, 28)).astype(np.float32)
    nrm = rng.normal(size=(64, 3)).astype(np.float32)
    nrm[:16] /= np.linalg.norm(nrm[:16], axis=1, keepdims=True)
    nrm[16:32] *= rng.uniform(1e-3, 1e3, (16, 1)).astype(np.float32)  # unnormalised, short and long
    nrm[32:35] = [[0, 0, 1], [0, -2, 0], [3, 0, 0]]
    got = native.irradiance_sh_eval(sh, nrm)
    c = sh[:, :27].astype(np.float64).reshape(64, 9, 3)
    want = ref.evaluate(c, nrm)
    Y = ref.sh9(nrm.astype(np.float64) / np.linalg.norm(nrm.astype(np.float64), axis=1, keepdims=True))
    scale = np.einsum("nmc,nm->nc", np.abs(c), ref.A * np.abs(Y))
    assert got.shape == (64, 3) and got.dtype == np.float32
    assert np.all(np.abs(got - want) <= 16 * 2.0 ** -24 * scale), (np.abs(got - want) / scale).max() * 2.0 ** 24
    for bad in ([0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0]):
        with pytest.raises(RuntimeError, match="zero or not finite"):
            native.irradiance_sh_eval(sh[:1], np.float32([bad]))


def _bias(n_u, n_v):
    """largest relative error of E over 50 normals when a random radiance of degree <= 2 is projected with n_u x n_v directions"""
    rng = np.random.default_rng(0)
    coef = rng.normal(size=(9, 1))
    nrm = rng.normal(size=(50, 3))
    d = ref.sphere_dirs(n_u, n_v)
    L = ref.sh9(d) @ coef                     # the radiance at the directions, one channel
    E = ref.evaluate(ref.project(L, d), nrm)  # (50, 1)
    exact = ref.evaluate(coef, nrm)
    return float(np.abs(E - exact).max() / np.abs(exact).max())


def test_reference_quadrature_bias():
    """the midpoint rule in z: a band-limited radiance is not reproduced exactly, and the bias falls as 1 / n_u^2"""
    d = ref.sphere_dirs(7, 5)
    assert d.shape == (35, 3) and np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15
    assert np.allclose(d[3 + 7 * 2], [np.sqrt(1 - 0.0) * np.cos(np.pi), np.sin(np.pi), 0.0], atol=1e-15)  # u = 3: z = 0; v = 2: phi = pi
    # orthonormality of the basis under a fine quadrature
    dd = ref.sphere_dirs(256, 64)
    Y = ref.sh9(dd)
    assert np.abs(Y.T @ Y * (4 * np.pi / dd.shape[0]) - np.eye(9)).max() < 1e-4
    e16, e64 = _bias(16, 16), _bias(64, 64)
    print("largest relative error of E: 16 x 16 %.3e, 64 x 64 %.3e, ratio %.2f" % (e16, e64, e16 / e64))
    assert e64 < 2e-3 and 12 < e16 / e64 < 20  # measured: 8.1e-4 and a ratio of 15.96
    # a constant radiance: c_0 exact, a small c_6, every other coefficient zero
    c = ref.project(np.ones((256, 1)), ref.sphere_dirs(16, 16))[:, 0]
    assert abs(c[0] - 4 * np.pi * 0.28209479177387814) < 1e-12 and abs(c[6] + 0.0155) < 1e-4
    assert np.abs(np.delete(c, [0, 6])).max() < 1e-12
    # the lattice and the dead-probe rule
    P = ref.volume_points((3, 1, 2), [0.0, 0.0, 0.0], [1.0, 2.0, 3.0])
    assert np.array_equal(P, [[0, 1, 0], [0.5, 1, 0], [1, 1, 0], [0, 1, 3], [0.5, 1, 3], [1, 1, 3]])
    sh = np.zeros((6, 28))
    sh[:, 0:3] = np.arange(6)[:, None] + 1.0
    sh[:, 27] = [1, 0, 1, 1, 1, 1]
    E, W = ref.lookup(sh, (3, 1, 2), [0, 0, 0], [1, 2, 3], np.array([[0.25, 5.0, 0.0], [0.5, 1.0, 0.0], [-1.0, 0.0, 1.5]]), np.array([[0, 0, 1.0]] * 3))
    y0a0 = 0.28209479177387814 * np.pi
    assert np.allclose(W, [0.5, 0.0, 1.0]) and np.allclose(E[0], 1.0 * y0a0) and np.all(E[1] == 0) and np.allclose(E[2], 2.5 * y0a0)


@pytest.mark.parametrize("nu,nv", GEN_SHAPES)
def test_generator_points_are_unambiguous(nu, nv):
    """the probes of the GPU generator test: the brute-force reference flags at most 2 % of their sphere rays as rays a float32 trace may
    decide differently, and they see both hits and misses (numpy only)"""
    K = nu * nv
    d = ref.sphere_dirs(nu, nv).astype(np.float32)
    o = np.repeat(GEN_POINTS[:, None, :], K, 1).reshape(-1, 3)
    t, unsafe = mref.global_nearest([mref.normalise(tris, c) for tris, c in gen_meshes()], o, np.tile(d, (GEN_POINTS.shape[0], 1)))
    hit = np.isfinite(t).reshape(-1, K)
    print("%d x %d: flagged %.4f, hit share per probe %s" % (nu, nv, unsafe.mean(), hit.mean(1)))
    assert unsafe.mean() <= UNSAFE_CAP
    assert hit[0].all() and not hit[4].any()
    if K > 1:
        assert all(0 < hit[i].mean() < 1 for i in (1, 2, 3))
