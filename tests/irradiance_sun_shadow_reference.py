"""A restatement of the NeRF shadow of the sun pass (include/ngp_hip.h, "sun", the *_shadowed entries) in numpy, on top of
irradiance_sun_reference.sun_rays and irradiance_bounce_reference.hits: which probe rays own a shadow ray (the rays the sun pass lights),
the shadow ray's origin q = h + shadow_bias N_ff, and what the tracer's alpha does to B. Nothing here comes from the package or from oracle/;
alpha_s itself is the tracer's business (ngp_trace_nerf_rays and the oracle's trace are its references).

`lit_q` takes dtype = float64 (the reference) or float32. The float32 form runs the SAME steps rounded as a float32 program rounds them, as
irradiance_sun_reference.sun_rays does: the direction, the hit distance by the ray / triangle expression of a float32 tracer on the
reference's own triangle, the normal, h = o + t w with the product rounded first, q = h + bias N_ff likewise. Which rays are lit is the
float64 form's decision in both. It exists only to price float32."""
import numpy as np

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import irradiance_sun_reference as sr
import irradiance_visibility_reference as vr


def lit_q(hit, probes, nu, nv, sun, bias, dtype=np.float64):
    """(q (P, K, 3), lit (P, K), unsafe (P, K)): the shadow rays' origins at the hits `hit` (of irradiance_bounce_reference.hits), zeros
    where the sun pass lights nothing; lit and unsafe are irradiance_sun_reference.sun_rays' own"""
    T_ = dtype
    probes = np.asarray(probes, np.float32)
    P, K = hit["t"].shape
    _, info = sr.sun_rays(hit, probes, nu, nv, sun, 1.0, bias, 1.0, None)
    lit = info["lit"].reshape(-1)
    q = np.zeros((P * K, 3), T_)
    if lit.any():
        s = sr.unit_sun(sun)
        o = np.repeat(probes, K, 0)[lit].astype(T_)
        b = T_(np.float32(bias))
        if dtype == np.float64:
            d = np.tile(sh_ref.sphere_dirs(nu, nv), (P, 1))[lit]
            t, N = hit["t"].reshape(-1)[lit], hit["N"].reshape(-1, 3)[lit]
            nff = np.where(((N * d).sum(1) < 0)[:, None], N, -N)
            assert np.all((nff * s.astype(np.float64)).sum(1) > 0)
            q[lit] = o + t[:, None] * d + b * nff
        else:
            d = np.tile(vr.sphere_dirs(nu, nv, T_), (P, 1))[lit].astype(T_)
            t, n = br._tri_t32(hit["T"][hit["tri"].reshape(-1)[lit]], o, d)
            N = (n / np.sqrt(((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]).astype(T_) + n[:, 2] * n[:, 2]).astype(T_))[:, None]).astype(T_)
            turned = ((N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]).astype(T_) + N[:, 2] * d[:, 2]).astype(T_) < 0
            nff = np.where(turned[:, None], N, -N).astype(T_)
            h = (o + (d * t[:, None]).astype(T_)).astype(T_)
            q[lit] = (h + (nff * b).astype(T_)).astype(T_)
    return q.reshape(P, K, 3), info["lit"], info["unsafe"]


def apply(B, alpha_s):
    """B' = fl32(max(1 - alpha_s, 0) B): B (..., 3) and alpha_s (...) as float32, one float32 product a channel"""
    B, a = np.asarray(B, np.float32), np.asarray(alpha_s, np.float32)
    through = np.maximum((np.float32(1) - a).astype(np.float32), np.float32(0))
    return (through[..., None] * B).astype(np.float32)


def case(scene, res, lo, hi, nu, nv, sun, bias=sr.STAGE_BIAS):
    """a lattice's own probes among `scene`'s meshes as the loader leaves them: a dict of probes, hit, q (float64), q32, lit, unsafe, safe
    and dev = the largest |q32 - q| on safe lit rays"""
    probes = vr.probe_positions(res, lo, hi)
    hit = br.hits(br.normalised(scene), probes, nu, nv)
    q, lit, unsafe = lit_q(hit, probes, nu, nv, sun, bias)
    q32, _, _ = lit_q(hit, probes, nu, nv, sun, bias, np.float32)
    safe = ~unsafe
    m = lit & safe
    dev = float(np.abs(q32.astype(np.float64) - q)[m].max()) if m.any() else 0.0
    return {"probes": probes, "hit": hit, "q": q, "q32": q32, "lit": lit, "unsafe": unsafe, "safe": safe, "dev": dev}
