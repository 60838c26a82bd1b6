"""A float64 restatement of the SH9 irradiance volumes (include/ngp_hip.h, "SH9 irradiance volumes"): the sphere of directions, the nine
real spherical harmonics of degree <= 2, the projection of a radiance onto them, the clamped-cosine evaluation, the probe lattice and the
lookup with its dead-probe rule. numpy only; nothing here comes from the package or from oracle/.

Written from the definitions: the real SH in the sign convention of the network's direction encoding (the Condon-Shortley phase dropped
for m = 0 only), and Ramamoorthi & Hanrahan, "An efficient representation for irradiance environment maps" (2001), for the factors
A = (pi, 2 pi / 3, pi / 4)."""
import numpy as np

A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)


def sphere_dirs(n_u, n_v):
    """the K = n_u n_v directions, k = u + n_u v: equal-area strata in (z, phi), stratum centres; (K, 3)"""
    k = np.arange(n_u * n_v)
    u, v = k % n_u, k // n_u
    a, b = (u + 0.5) / n_u, (v + 0.5) / n_v
    z, phi = 1.0 - 2.0 * a, 2.0 * np.pi * b
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def sh9(d):
    """Y_m(d) for unit directions d (..., 3): (..., 9)"""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c1 = 0.5 * np.sqrt(3.0 / np.pi)
    c2 = 0.5 * np.sqrt(15.0 / np.pi)
    return np.stack([np.full_like(x, 0.5 * np.sqrt(1.0 / np.pi)),
                     -c1 * y, c1 * z, -c1 * x,
                     c2 * x * y, -c2 * y * z, 0.25 * np.sqrt(5.0 / np.pi) * (3.0 * z * z - 1.0), -c2 * x * z, 0.5 * c2 * (x * x - y * y)], -1)


def project(L, dirs):
    """c[m, ch] = (4 pi / K) sum_k L[k, ch] Y_m(dirs[k]) for L (..., K, C): (..., 9, C)"""
    L = np.asarray(L, np.float64)
    return np.einsum("...kc,km->...mc", L, sh9(dirs)) * (4.0 * np.pi / L.shape[-2])


def evaluate(c, n):
    """E[ch] = sum_m A_m c[m, ch] Y_m(n / |n|) for c (..., 9, C) and n (..., 3): (..., C)"""
    n = np.asarray(n, np.float64)
    Y = sh9(n / np.linalg.norm(n, axis=-1, keepdims=True))
    return np.einsum("...mc,...m->...c", np.asarray(c, np.float64), A * Y)


def volume_points(res, lo, hi):
    """the probe positions in index order g = i + rx (j + ry k): lo + (i / (rx - 1), ...) (hi - lo), an axis of one probe at the box centre"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ax = [lo[a] + (np.arange(res[a]) / (res[a] - 1) if res[a] > 1 else np.array([0.5])) * (hi[a] - lo[a]) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3)


def lookup(sh, res, lo, hi, p, n, absolute=False):
    """(E (n, 3), W (n,)) at points p with normals n from records sh (probes, 28) in index order: trilinear over the up to 8 corner probes,
    a probe whose float 27 is 0 is dead and skipped, the live ones renormalised by their weight W; zeros where W = 0. absolute: the same
    weighted mean of |c| evaluated with |Y| (an error scale, not an irradiance)."""
    sh = np.asarray(sh, np.float64).reshape(-1, 28)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p, n = np.asarray(p, np.float64), np.asarray(n, np.float64)
    i0, f = np.zeros(p.shape, np.int64), np.zeros(p.shape)
    for a in range(3):
        if res[a] > 1:
            s = np.clip((p[:, a] - lo[a]) / (hi[a] - lo[a]), 0.0, 1.0) * (res[a] - 1)
            i0[:, a] = np.minimum(np.floor(s), res[a] - 2)
            f[:, a] = s - i0[:, a]
    csum, W = np.zeros((p.shape[0], 27)), np.zeros(p.shape[0])
    for corner in range(8):
        d = np.array([corner & 1, (corner >> 1) & 1, corner >> 2])
        w = np.prod(np.where(d == 1, f, 1.0 - f), axis=1)
        idx = np.minimum(i0 + d, np.asarray(res) - 1)  # (an index past the lattice only ever carries weight 0)
        rec = sh[idx[:, 0] + res[0] * (idx[:, 1] + res[1] * idx[:, 2])]
        w = np.where(rec[:, 27] != 0, w, 0.0)
        csum += w[:, None] * (np.abs(rec[:, :27]) if absolute else rec[:, :27])
        W += w
    c = np.where(W[:, None] > 0, csum / np.where(W > 0, W, 1.0)[:, None], 0.0).reshape(-1, 9, 3)
    Y = sh9(n / np.linalg.norm(n, axis=1, keepdims=True))
    E = np.einsum("nmc,nm->nc", c, A * (np.abs(Y) if absolute else Y))
    return E, W
