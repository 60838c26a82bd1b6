"""The cases the mesh-albedo tests share (include/ngp_hip.h, "mesh albedos"), composed from the existing float64 references with no new
arithmetic: the mesh of a hit is the mesh whose triangles hold hit["tri"] in the concatenated list, and the per-mesh B is
sum_m [mesh = m] x (the uniform reference run with albedo A_m), in float64 and in the references' float32 form.

The allowances are the existing ones: 256 ULP of the scale + mesh_cases.GPU_FACTOR x the composed float32 form's deviation from float64 on
the case's own safe rays. The scale is stage_case's of either reference: the bounce's the source volume's largest |E| / pi (5.0e-5 at K =
64), the sun's the largest albedo x radiance / pi, the largest channel over both albedos taken for the albedo. Nothing here comes from the
package or from oracle/."""
import numpy as np

import irradiance_bounce_reference as br
import irradiance_sun_reference as sr

A0, A1 = np.float32([0.9, 0.1, 0.1]), np.float32([0.2, 0.7, 0.4])
ALBEDOS = (A0, A1)
BOUNCE_SHAPES = [(3, 5), (8, 8), (9, 9), (16, 16)]  # K = 15, 64, 81, 256: both meshes among the safe hits; (1, 1) hits mesh 0 alone (the tail)
SUN_SHAPES = [(8, 8), (9, 9), (16, 16)]  # K = 64, 81, 256: both meshes among the lit safe rays
# safe hits on (mesh 0, mesh 1) of the bounce stage per K, and lit safe rays of the sun stage under STAGE_SUN
BOUNCE_HITS = {15: (20, 1), 64: (89, 8), 81: (111, 10), 256: (354, 32)}
SUN_LIT = {64: (25, 2), 81: (29, 2), 256: (100, 7)}
E2E_HITS = (122, 92, 1)  # floor hits, torus hits, unsafe rays of the 12 x 64 of irradiance_bounce_reference.E2E_CASE
_cache = {}


def mesh_of(hit, meshes):
    """(P, K) the mesh of every ray's closest hit, -1 without one"""
    ends = np.cumsum([np.asarray(m).shape[0] for m in meshes])
    return np.where(hit["tri"] >= 0, np.searchsorted(ends, hit["tri"], side="right"), -1)


def compose(mesh, per_mesh):
    """sum_m [mesh = m] B_m over the uniform runs per_mesh[m] (P, K, 3)"""
    out = np.zeros_like(per_mesh[0])
    for m, B in enumerate(per_mesh):
        out = out + np.where((mesh == m)[..., None], B, 0).astype(B.dtype)
    return out


def bounce_rays(hit, mesh, probes, nu, nv, albedos, alpha, src, dtype=np.float64):
    return compose(mesh, [br.bounce_rays(hit, probes, nu, nv, a, alpha, src, dtype)[0] for a in albedos])


def sun_rays(hit, mesh, probes, nu, nv, sun, radiance, bias, albedos, alpha, dtype=np.float64):
    return compose(mesh, [sr.sun_rays(hit, probes, nu, nv, sun, radiance, bias, a, alpha, dtype)[0] for a in albedos])


def _finish(case, B, B32, scale):
    import mesh_cases as mc

    safe = case["safe"]
    dev = float(np.abs(B32.astype(np.float64) - B)[safe].max()) if safe.any() else 0.0
    return dict(case, B=B, B32=B32, dev=dev, allow=256 * 2.0 ** -24 * scale / np.pi + mc.GPU_FACTOR * dev)


def bounce_case(nu, nv, visible, albedos=ALBEDOS):
    """irradiance_bounce_reference.stage_case with the two meshes' own albedos: hit, mesh, alpha, B, B32, safe, dev, allow"""
    key = ("bounce", nu, nv, visible, tuple(np.concatenate(albedos).tolist()))
    if key not in _cache:
        from irradiance_volume_cases import GEN_POINTS

        base = br.stage_case(nu, nv, visible)
        sh, res, lo, hi = br.stage_volume()
        D, maps = br.stage_maps()
        src = br.source(sh, res, lo, hi, maps, D, br.STAGE_BIAS) if visible else br.source(sh, res, lo, hi)
        hit, alpha = base["hit"], base["alpha"]
        mesh = mesh_of(hit, br.stage_meshes())
        B = bounce_rays(hit, mesh, GEN_POINTS, nu, nv, albedos, alpha, src)
        B32 = bounce_rays(hit, mesh, GEN_POINTS, nu, nv, albedos, alpha, src, np.float32)
        scale = br.volume_scale(sh)  # (as stage_case computes it: an albedo is at most 1)
        _cache[key] = _finish({"hit": hit, "mesh": mesh, "alpha": alpha, "safe": base["safe"], "uniform": base}, B, B32, scale)
    return _cache[key]


def sun_case(nu, nv, albedos=ALBEDOS):
    """irradiance_sun_reference.stage_case with the two meshes' own albedos: hit, mesh, alpha, B, B32, info, safe, dev, allow"""
    key = ("sun", nu, nv, tuple(np.concatenate(albedos).tolist()))
    if key not in _cache:
        from irradiance_volume_cases import GEN_POINTS

        base = sr.stage_case(nu, nv)
        hit, alpha = base["hit"], base["alpha"]
        mesh = mesh_of(hit, br.stage_meshes())
        args = (hit, mesh, GEN_POINTS, nu, nv, sr.STAGE_SUN, sr.STAGE_RADIANCE, sr.STAGE_BIAS, albedos, alpha)
        scale = max(float((np.float64(a) * sr.STAGE_RADIANCE.astype(np.float64)).max()) for a in albedos)
        _cache[key] = _finish({"hit": hit, "mesh": mesh, "alpha": alpha, "info": base["info"], "safe": base["safe"], "uniform": base}, sun_rays(*args),
                              sun_rays(*args, np.float32), scale)
    return _cache[key]


def e2e_hits():
    """the hits of irradiance_bounce_reference.E2E_CASE's lattice among e2e_scene's floor (mesh 0) and torus (mesh 1), and their meshes"""
    if "e2e" not in _cache:
        import irradiance_visibility_reference as vr

        res, lo, hi, nu, nv = br.E2E_CASE
        meshes = br.normalised(br.e2e_scene())
        hit = br.hits(meshes, vr.probe_positions(res, lo, hi), nu, nv)
        _cache["e2e"] = (hit, mesh_of(hit, meshes))
    return _cache["e2e"]
