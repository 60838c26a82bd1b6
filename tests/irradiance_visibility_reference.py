"""A restatement of the probe visibility contract (include/ngp_hip.h, "probe visibility") in numpy: the octahedral texel directions and their
inverse, the wrapped bilinear read of a map, the maps from given rays and distances, the default D, and the visibility-weighted lookup
with its absolute scale. Written from the definitions (the Chebyshev weight: Majercik et al., "Dynamic Diffuse Global Illumination with
Ray-Traced Irradiance Fields", JCGT 2019); nothing here comes from the package or from oracle/. The SH9 pieces are
irradiance_sh_reference's.

Every function takes dtype = float64 (the reference) or float32. The float32 form runs the SAME sums in float32, in the order the contract
states (k ascending; a blend corner by corner), and exists only to measure what float32 costs: the tests' allowances are multiples of its
deviation from the float64 form on the test's own inputs."""
import numpy as np

import irradiance_sh_reference as sh_ref

SIDE = 8
TEXELS = 64
VAR_FLOOR = 1e-4  # of D^2
# rho = x^(2^e) is formed in float32: below this float64 sum of a texel's weights its largest terms are near or under float32's normal
# range (2^-126) and the texel's float32 moments mean little; exactly 0 is exact again: the texel stores (D, D^2)
S_UNDERFLOW = 2.0 ** -100


def _sgn(x):
    return np.where(x < 0, -1.0, 1.0).astype(x.dtype)


def decode(a, b, dtype=np.float64):
    """the unit direction of the point (a, b) of the square [-1, 1]^2: (..., 3)"""
    T = dtype
    a, b = np.asarray(a, T), np.asarray(b, T)
    z = T(1) - np.abs(a) - np.abs(b)
    x = np.where(z < 0, (T(1) - np.abs(b)) * _sgn(a), a)
    y = np.where(z < 0, (T(1) - np.abs(a)) * _sgn(b), b)
    d = np.stack([x, y, z], -1).astype(T)
    return (d / np.sqrt((d * d).sum(-1, dtype=T))[..., None]).astype(T)


def texel_dirs(dtype=np.float64):
    """w_q of the 64 texels, q = i + 8 j: (64, 3)"""
    T = dtype
    q = np.arange(TEXELS)
    a = (T(2) * (T(0.5) + (q % SIDE).astype(T)) / T(SIDE) - T(1)).astype(T)
    b = (T(2) * (T(0.5) + (q // SIDE).astype(T)) / T(SIDE) - T(1)).astype(T)
    return decode(a, b, T)


def encode(d, dtype=np.float64):
    """(a, b) in [-1, 1]^2 of directions d (..., 3): the inverse of the texel direction"""
    d = np.asarray(d, dtype)
    inv = dtype(1) / (np.abs(d[..., 0]) + np.abs(d[..., 1]) + np.abs(d[..., 2]))
    a, b = d[..., 0] * inv, d[..., 1] * inv
    fold = d[..., 2] < 0
    fa = (dtype(1) - np.abs(b)) * _sgn(a)
    fb = (dtype(1) - np.abs(a)) * _sgn(b)
    return np.where(fold, fa, a).astype(dtype), np.where(fold, fb, b).astype(dtype)


def wrap(i, j):
    """texel indices in -1..8 -> 0..7 across the octahedron's edges: i first, then j with the roles swapped"""
    i, j = np.asarray(i).copy(), np.asarray(j).copy()
    lo, hi = i < 0, i > 7
    j = np.where(lo | hi, 7 - j, j)
    i = np.where(lo, -1 - i, np.where(hi, 15 - i, i))
    lo, hi = j < 0, j > 7
    i = np.where(lo | hi, 7 - i, i)
    j = np.where(lo, -1 - j, np.where(hi, 15 - j, j))
    return i, j


def read_map(maps, d, dtype=np.float64):
    """bilinear read of maps (n, 64, C) at unit directions d (n, 3): (n, C)"""
    T = dtype
    maps = np.asarray(maps, T)
    a, b = encode(d, T)
    s, t = T(4) * (a + T(1)) - T(0.5), T(4) * (b + T(1)) - T(0.5)
    fs, ft = np.floor(s), np.floor(t)
    i0, j0 = np.clip(fs.astype(np.int64), -1, 7), np.clip(ft.astype(np.int64), -1, 7)
    ws, wt = (s - fs).astype(T), (t - ft).astype(T)
    rows = np.arange(maps.shape[0])

    def texel(i, j):
        i, j = wrap(i, j)
        return maps[rows, i + SIDE * j]

    t00, t10, t01, t11 = texel(i0, j0), texel(i0 + 1, j0), texel(i0, j0 + 1), texel(i0 + 1, j0 + 1)
    w00, w10, w01, w11 = (T(1) - ws) * (T(1) - wt), ws * (T(1) - wt), (T(1) - ws) * wt, ws * wt
    return ((w00[:, None] * t00 + w10[:, None] * t10) + (w01[:, None] * t01 + w11[:, None] * t11)).astype(T)


def sphere_dirs(n_u, n_v, dtype=np.float64):
    """the SH9 section's K directions; in float32 formed as a float32 program would (the reference form: irradiance_sh_reference.sphere_dirs)"""
    if dtype == np.float64:
        return sh_ref.sphere_dirs(n_u, n_v)
    T = dtype
    k = np.arange(n_u * n_v)
    a = ((k % n_u).astype(T) + T(0.5)) / T(n_u)
    b = ((k // n_u).astype(T) + T(0.5)) / T(n_v)
    s = T(2) * np.sqrt(a * (T(1) - a))
    phi = (T(2) * b).astype(np.float64) * np.pi  # (sine and cosine of half turns: rounded once, from the float32 argument)
    d = np.stack([s * np.cos(phi).astype(T), s * np.sin(phi).astype(T), T(1) - T(2) * a], 1).astype(T)
    return (d / np.sqrt((d * d).sum(1, dtype=T))[:, None]).astype(T)


def maps_from_rays(dirs, t_max, e, D, dtype=np.float64):
    """the maps (P, 64, 2) of P probes from the K ray directions dirs (K, 3) and the rays' hit distances t_max (P, K) (+inf: no hit), and the
    float sums S (P, 64) of the weights. The sums run over k ascending."""
    T = dtype
    w = texel_dirs(T)
    dirs = np.asarray(dirs, T)
    D = T(D)
    d = np.minimum(np.asarray(t_max, T), D)
    P = d.shape[0]
    S, s1, s2 = np.zeros((P, TEXELS), T), np.zeros((P, TEXELS), T), np.zeros((P, TEXELS), T)
    for k in range(dirs.shape[0]):
        x = np.maximum(T(0), (w[:, 0] * dirs[k, 0] + w[:, 1] * dirs[k, 1]) + w[:, 2] * dirs[k, 2]).astype(T)
        rho = x
        with np.errstate(under="ignore"):
            for _ in range(e):
                rho = (rho * rho).astype(T)
            rd = (rho[None, :] * d[:, k, None]).astype(T)
            S = (S + rho[None, :]).astype(T)
            s1 = (s1 + rd).astype(T)
            s2 = (s2 + rd * d[:, k, None]).astype(T)
    ok = S > 0
    den = np.where(ok, S, T(1))
    with np.errstate(under="ignore"):
        maps = np.stack([np.where(ok, s1 / den, D), np.where(ok, s2 / den, D * D)], -1).astype(T)
    return maps, S


def default_max_distance(res, lo, hi):
    """D of a descriptor that asks for the default: 1.5 x the diagonal of a lattice cell (an axis of one probe: extent 0), 1.5 x the box
    diagonal when every axis has one probe; float32"""
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    if all(r == 1 for r in res):
        return np.float32(1.5 * np.sqrt(((hi - lo) ** 2).sum()))
    return np.float32(1.5 * np.sqrt(sum(((hi[a] - lo[a]) / (res[a] - 1)) ** 2 for a in range(3) if res[a] > 1)))


def probe_positions(res, lo, hi):
    """the lattice formula in double from the descriptor's floats, rounded to float32: (probes, 3) in index order"""
    return sh_ref.volume_points(res, np.asarray(lo, np.float32), np.asarray(hi, np.float32)).astype(np.float32)


def lookup_visible(sh, res, lo, hi, maps, D, normal_bias, p, n, absolute=False, dtype=np.float64, points_dtype=np.float32):
    """the visible lookup at points p (n, 3), normals n (n, 3) from records sh (probes, 28) and maps (probes, 64, 2), both float32 data.
    Returns (E (n, 3), W' (n,), info): info holds vis (n, 8; 1 where a corner takes no part), wgt (n, 8: the live corners' trilinear weights)
    and r (n, 8). dtype float32: the weights, vis and the blend in float32 (the evaluation of E from the blended coefficients stays in float64:
    its error is the plain lookup's). absolute: the blend of |c| evaluated with |Y|, an error scale. points_dtype: the points and normals are
    float32 data, as an entry takes them; float64 keeps a caller's float64 points (a frame's hit points)."""
    T = dtype
    sh = np.asarray(sh, np.float32).reshape(-1, 28).astype(T)
    maps = np.asarray(maps, np.float32).reshape(-1, TEXELS, 2)
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    lo_, hi_ = lo32.astype(T), hi32.astype(T)
    p, n = np.asarray(p, points_dtype).astype(T), np.asarray(n, points_dtype).astype(T)
    nh = (n / np.sqrt((n * n).sum(1, dtype=T))[:, None]).astype(T)
    pos = probe_positions(res, lo32, hi32).astype(T)
    D = T(np.float32(D))
    i0, f = np.zeros(p.shape, np.int64), np.zeros(p.shape, T)
    for a in range(3):
        if res[a] > 1:
            s = (np.clip((np.clip(p[:, a], lo_[a], hi_[a]) - lo_[a]) / (hi_[a] - lo_[a]), T(0), T(1)) * T(res[a] - 1)).astype(T)
            fl = np.minimum(np.floor(s), T(res[a] - 2))
            i0[:, a] = fl.astype(np.int64)
            f[:, a] = s - fl
    pb = (p + nh * T(np.float32(normal_bias))).astype(T)
    N = p.shape[0]
    csum, W = np.zeros((N, 27), T), np.zeros(N, T)
    vis_all, wgt_all, r_all = np.ones((N, 8)), np.zeros((N, 8)), np.zeros((N, 8))
    for corner in range(8):
        dxyz = np.array([corner & 1, (corner >> 1) & 1, corner >> 2])
        wgt = (np.where(dxyz[0] == 1, f[:, 0], T(1) - f[:, 0]) * np.where(dxyz[1] == 1, f[:, 1], T(1) - f[:, 1])).astype(T)
        wgt = (wgt * np.where(dxyz[2] == 1, f[:, 2], T(1) - f[:, 2])).astype(T)
        idx = np.minimum(i0 + dxyz, np.asarray(res) - 1)  # (an index past the lattice only ever carries weight 0)
        g = idx[:, 0] + res[0] * (idx[:, 1] + res[1] * idx[:, 2])
        rec = sh[g]
        live = (wgt != 0) & (rec[:, 27] != 0)
        v = (pb - pos[g]).astype(T)
        r = np.sqrt((v * v).sum(1, dtype=T)).astype(T)
        unit = v / np.where(r > 0, r, T(1))[:, None]
        unit[r == 0] = (0, 0, 1)
        m = read_map(maps[g], unit.astype(T), T)
        var = np.maximum(m[:, 1] - m[:, 0] * m[:, 0], T(VAR_FLOOR) * D * D).astype(T)
        dd = (r - m[:, 0]).astype(T)
        ch = (var / (var + dd * dd)).astype(T)
        vis = np.where((r == 0) | (r <= m[:, 0]), T(1), ch * ch * ch).astype(T)
        wv = np.where(live, wgt * vis, T(0)).astype(T)
        csum = (csum + wv[:, None] * (np.abs(rec[:, :27]) if absolute else rec[:, :27])).astype(T)
        W = (W + wv).astype(T)
        vis_all[:, corner] = np.where(live, vis, 1.0)
        wgt_all[:, corner] = np.where(live, wgt, 0.0)
        r_all[:, corner] = r
    c = np.where(W[:, None] > 0, csum * (T(1) / np.where(W > 0, W, T(1)))[:, None], T(0)).astype(np.float64).reshape(-1, 9, 3)
    Y = sh_ref.sh9(nh.astype(np.float64) / np.linalg.norm(nh.astype(np.float64), axis=1, keepdims=True))
    E = np.einsum("nmc,nm->nc", c, sh_ref.A * (np.abs(Y) if absolute else Y))
    return E, W.astype(np.float64), {"vis": vis_all, "wgt": wgt_all, "r": r_all, "pos": pos.astype(np.float64)}
