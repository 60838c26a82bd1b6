"""A restatement of the sun contract (include/ngp_hip.h, "sun") in numpy: the closest hit of a probe's sphere rays with its triangle kept
(irradiance_bounce_reference.hits), the normal turned against the ray, its cosine to the sun, the shadow ray from the lifted hit point
against every triangle of every mesh (mesh_reference.nearest_hit, the brute force), the radiance the hit throws back and the projection
(irradiance_sh_reference.project). Nothing here comes from the package or from oracle/, and nothing is a BVH.

`sun_rays` takes dtype = float64 (the reference) or float32. The float32 form runs the SAME steps rounded as a float32 program rounds
them, as irradiance_bounce_reference.bounce_rays does: the directions, the hit distance by the ray / triangle expression of a float32
tracer on the reference's own triangle, the normal, the cosine, the product. Which rays are shadowed is the float64 form's decision in
both. It exists only to price float32: the tests' allowance is a multiple of its deviation from the float64 form on the test's own inputs.

A ray is unsafe, and left out of comparisons, when its primary hit is unsafe (irradiance_bounce_reference.hits), when
mesh_reference.nearest_hit flags its shadow ray (edge, tie, range), or when some triangle is crossed inside its edges at |t| < TIE_EPS
of the shadow origin: there a float32 program may legitimately decide the other way."""
import numpy as np

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import irradiance_visibility_reference as vr
import mesh_reference as ref

STAGE_SUN = np.float32([0.3, 0.9, -0.2])
STAGE_RADIANCE = ref.SUN_COLOUR.astype(np.float32)
STAGE_BIAS = ref.SHADOW_OFFSET
# E of nine coefficients overshoots the true irradiance of a non-negative radiance by at most 1.0625, the 16 x 16 quadrature by at most
# 1.29 % (test_irradiance_bounce_cpu.py::test_series_between_two_facing_quads)
OVERSHOOT = 1.0625 * 1.02
_cache = {}


def unit_sun(direction):
    """s^ as the library forms it: the quotient in double precision from the float32 direction, rounded to float32"""
    d = np.asarray(direction, np.float32).astype(np.float64)
    return (d / np.sqrt((d * d).sum())).astype(np.float32)


def sun_rays(hit, probes, nu, nv, sun, radiance, bias, albedo, alpha, dtype=np.float64):
    """B^sun (P, K, 3) at the hits `hit` (of irradiance_bounce_reference.hits): (1 - alpha) albedo radiance c vis / pi, 0 without a hit and
    where c <= 0. alpha: (P, K) or None. Returns (B, info): info holds, per ray (P, K), hit, facing (a hit with c > 0), shadowed and lit (of
    the facing rays), unsafe, and t_shadow (the nearest shadow hit of the facing rays, inf elsewhere)."""
    T_ = dtype
    probes = np.asarray(probes, np.float32)
    P, K = hit["t"].shape
    mask = (hit["tri"] >= 0).reshape(-1)
    s = unit_sun(sun)
    source = (np.broadcast_to(np.asarray(albedo, np.float32), (3,)).astype(T_) * np.broadcast_to(np.asarray(radiance, np.float32), (3,)).astype(T_)).astype(T_)
    al = np.zeros(P * K, T_) if alpha is None else np.asarray(alpha, np.float32).reshape(-1).astype(T_)
    B = np.zeros((P * K, 3), T_)
    facing, shadowed, unsafe = np.zeros(P * K, bool), np.zeros(P * K, bool), hit["unsafe"].reshape(-1).copy()
    t_shadow = np.full(P * K, np.inf)
    if mask.any():
        # the float64 geometry decides what is lit, for both forms
        o64 = np.repeat(probes, K, 0)[mask].astype(np.float64)
        d64 = np.tile(sh_ref.sphere_dirs(nu, nv), (P, 1))[mask]
        N64 = hit["N"].reshape(-1, 3)[mask]
        nff64 = np.where(((N64 * d64).sum(1) < 0)[:, None], N64, -N64)
        c64 = (nff64 * s.astype(np.float64)).sum(1)
        f = c64 > 0
        q64 = o64[f] + hit["t"].reshape(-1)[mask][f, None] * d64[f] + float(np.float32(bias)) * nff64[f]
        sd = np.broadcast_to(s.astype(np.float64), q64.shape)
        ts, _, _, s_unsafe = ref.nearest_hit(hit["T"], q64, sd)
        tb, _, _, _ = ref.nearest_hit(hit["T"], q64, -sd)  # (a crossing just behind the origin)
        idx = np.flatnonzero(mask)[f]
        facing[idx] = True
        shadowed[idx] = np.isfinite(ts)
        t_shadow[idx] = ts
        unsafe[idx] |= s_unsafe | (ts < ref.TIE_EPS) | (tb < ref.TIE_EPS)
        if dtype == np.float64:
            c = c64
        else:
            o = np.repeat(probes, K, 0)[mask].astype(T_)
            d = np.tile(vr.sphere_dirs(nu, nv, T_), (P, 1))[mask].astype(T_)
            _, n = br._tri_t32(hit["T"][hit["tri"].reshape(-1)[mask]], o, d)
            N = (n / np.sqrt(((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]).astype(T_) + n[:, 2] * n[:, 2]).astype(T_))[:, None]).astype(T_)
            turned = ((N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]).astype(T_) + N[:, 2] * d[:, 2]).astype(T_) < 0
            nff = np.where(turned[:, None], N, -N).astype(T_)
            c = ((nff[:, 0] * s[0] + nff[:, 1] * s[1]).astype(T_) + nff[:, 2] * s[2]).astype(T_)
        lit = f & ~np.isfinite(np.where(f, t_shadow[mask], np.inf))
        M = ((source[None, :] * np.maximum(c, 0)[:, None].astype(T_)).astype(T_) / T_(np.pi)).astype(T_)
        B[mask] = np.where(lit[:, None], ((T_(1) - al[mask])[:, None] * M).astype(T_), T_(0))
    shape = (P, K)
    info = {"hit": mask.reshape(shape), "facing": facing.reshape(shape), "shadowed": shadowed.reshape(shape), "lit": (facing & ~shadowed).reshape(shape),
            "unsafe": unsafe.reshape(shape), "t_shadow": t_shadow.reshape(shape)}
    return B.reshape(P, K, 3), info


def sunlit(v0, B, nu, nv):
    """S (P, 28) in float64: V_0 + the projection of B on the 27 coefficients, float 27 V_0's"""
    out = np.asarray(v0, np.float64).reshape(-1, 28).copy()
    out[:, :27] += sh_ref.project(np.asarray(B, np.float64), sh_ref.sphere_dirs(nu, nv)).reshape(out.shape[0], 27)
    return out


def stage_case(nu, nv, sun=STAGE_SUN):
    """the per-ray stage test's case at irradiance_volume_cases.GEN_POINTS among irradiance_bounce_reference.stage_meshes: a dict of hit, alpha,
    B (float64), B32 (the float32 form), info, safe (P, K), dev = the largest |B32 - B| on safe rays, and allow = 256 ULP of the largest
    albedo x radiance / pi + mesh_cases.GPU_FACTOR dev"""
    key = (nu, nv, tuple(np.float32(sun).tolist()))
    if key not in _cache:
        import mesh_cases as mc
        from irradiance_volume_cases import GEN_POINTS

        hit = br.hits(br.stage_meshes(), GEN_POINTS, nu, nv)
        alpha = br.stage_alpha(GEN_POINTS.shape[0], nu * nv)
        B, info = sun_rays(hit, GEN_POINTS, nu, nv, sun, STAGE_RADIANCE, STAGE_BIAS, br.STAGE_ALBEDO, alpha)
        B32, _ = sun_rays(hit, GEN_POINTS, nu, nv, sun, STAGE_RADIANCE, STAGE_BIAS, br.STAGE_ALBEDO, alpha, np.float32)
        safe = ~info["unsafe"]
        dev = float(np.abs(B32.astype(np.float64) - B)[safe].max()) if safe.any() else 0.0
        scale = float((br.STAGE_ALBEDO.astype(np.float64) * STAGE_RADIANCE.astype(np.float64)).max())
        _cache[key] = {"hit": hit, "alpha": alpha, "B": B, "B32": B32, "info": info, "safe": safe, "dev": dev, "allow": 256 * 2.0 ** -24 * scale / np.pi + mc.GPU_FACTOR * dev}
    return _cache[key]
