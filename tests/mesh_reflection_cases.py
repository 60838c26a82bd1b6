"""What test_mesh_reflection_cpu.py and test_mesh_reflection_gpu.py share (include/ngp_hip.h, "mesh reflection"): the two cases and
mesh_sun_nerf_shadow_cases.render_with_sun_factor restated with a radiance added per pixel behind the BRDF, which also returns every pixel's
mirror ray.

A pixel owns a mirror ray when it is covered AND its primary ray found a triangle (mesh_reference.trace's hit, a real triangle hit: a covered
pixel whose ray chose no mesh owns none). With n^ = unit(ff), ff the winding normal turned against the primary ray d, and c = -(n^ . d):
    q = pos + SHADOW_OFFSET n^,   r = d + 2 c n^,   t_hit = mesh_reference.global_nearest(meshes, q, unit(r))   (inf: no mesh in the way)
    added = strength F rgb_r where alpha_r > 0,   F = mix(Cspec0, 1, schlick(c)),   Cspec0 = mix(0.08 specular, base^2, metallic)
(rgb_r, alpha_r) is what the caller hands in: the premultiplied radiance the NeRF sends along the ray. q32, r32 and c32 are the same in
float32, every product and sum rounded where a float32 program rounds it, on the reference's own triangle; they exist only to price float32.

Case A is mesh_sun_nerf_shadow_cases' scene, camera and sun: the floor under the unit NeRF. Case B adds an upright plate that stands between
part of the floor's mirror rays and the object, so that those rays are cut (a finite t_hit) in front of density they would otherwise cross."""
import numpy as np

import irradiance_bounce_reference as br
import mesh_cases as mc
import mesh_reference as ref
import mesh_sun_nerf_shadow_cases as sc

WIDTH, HEIGHT, FOCAL, SUN, CAMERA = sc.WIDTH, sc.HEIGHT, sc.FOCAL, sc.SUN, sc.CAMERA
MIN_RAYS, FULL_SHARE, EMPTY_SHARE = 200, 0.20, 0.30  # case A: pixels that own a ray; of them alpha_r > 0.9; alpha_r = 0
MIN_CUT, MIN_CUT_FULL = 100, 50                      # case B: rays with a finite t_hit; of them with an uncut alpha_r > 0.9
# The plate: mesh_cases.cube scaled and centred so that, after the loader's normalisation (longest side 1), it is 0.04 thick in x, spans the
# floor in z and stands from just above the floor (y = -0.089) to just under the captured object's base plate (y = 0.189 against 0.2), at
# x = 0.55 .. 0.59. Mirror rays of floor pixels on the camera's side of it climb towards the object's underside and meet the plate first.
# (A plate that hangs higher, or beyond the object, cuts rays only behind the density they cross, and their alpha does not change.)
PLATE_SCALE, PLATE_CENTER = (0.04, 0.28, 1.0), (0.07, -0.45, 0.0)
_cache = {}


def scene(case="A"):
    """[(triangles, centre)]: A the floor, B the floor and the plate"""
    if case == "A":
        return br.floor_scene()
    plate = (mc.cube().astype(np.float64) * np.array(PLATE_SCALE)).astype(np.float32)
    return br.floor_scene() + [(plate, PLATE_CENTER)]


def meshes(case="A"):
    return br.normalised(scene(case))


def _dot32(x, y):
    f = np.float32
    return ((x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]).astype(f) + x[:, 2] * y[:, 2]).astype(f)


def _mirror32(meshes, M, d, entry, start, owns):
    """(q32, r32, c32) of the pixels `owns` as a float32 program forms them, on the reference's own triangles: the hit by the float32
    tracer's ray / triangle expression, n^ by one square root and three quotients, c = -((x x + y y) + z z), q = pos + fl(n^ 1e-3),
    r = d + fl(n^ fl(2 c))"""
    f = np.float32
    n_px = d.shape[0]
    q32, r32, c32 = np.zeros((n_px, 3), f), np.zeros((n_px, 3), f), np.zeros(n_px, f)
    if not owns.any():
        return q32, r32, c32
    _, mesh, idx, _, _, _ = ref.reference_rule_hit(meshes, start, d)
    d32 = d[owns].astype(f)
    step = (np.maximum(np.where(np.isfinite(entry[owns]), entry[owns], 0.0), 0.0).astype(f) + f(1e-6)).astype(f)
    o32 = (M[:, 3].astype(f) + (d32 * step[:, None]).astype(f)).astype(f)
    tri = np.stack([meshes[m][i] for m, i in zip(mesh[owns], idx[owns])]).astype(f)
    t, n = br._tri_t32(tri, o32, d32)
    pos = (o32 + (d32 * t[:, None]).astype(f)).astype(f)
    nn = (n / np.sqrt(_dot32(n, n))[:, None]).astype(f)
    nff = np.where((_dot32(nn, d32) < 0)[:, None], nn, -nn).astype(f)
    nh = (nff / np.sqrt(_dot32(nff, nff))[:, None]).astype(f)  # (the pass normalises the turned normal once more)
    c = (-_dot32(nh, d32)).astype(f)
    q32[owns] = (pos + (nh * f(ref.SHADOW_OFFSET)).astype(f)).astype(f)
    r32[owns] = (d32 + (nh * (f(2) * c).astype(f)[:, None]).astype(f)).astype(f)
    c32[owns] = c
    return q32, r32, c32


def _t_hit32(meshes, rq, r, rq32, r32, cut):
    """t_hit of the rays `cut` as a float32 program forms it: the float32 tracer's ray / triangle expression on the triangle the reference
    hits, from q32 along the float32 normalize(r32)"""
    out = np.zeros(rq.shape[0], np.float32)
    if cut.any():
        T = np.concatenate(meshes)
        _, idx, _, _ = ref.nearest_hit(T, rq[cut], ref._unit(r[cut]))
        out[cut], _ = br._tri_t32(T[idx].astype(np.float32), rq32[cut], unit32(r32[cut]))
    return out


def fresnel(c, basecolor=(0.8, 0.8, 0.8), metallic=0.0, specular=1.0, dtype=np.float64):
    """F (n, 3) = mix(Cspec0, 1, schlick(c)), Cspec0 = mix(specular 0.08 (1, 1, 1), base^2, metallic): the BRDF's own, its tint at 0. With
    dtype float32 every operation is rounded to float32, in the pass's order."""
    t = dtype
    base = np.asarray(basecolor, np.float32).astype(t)
    base2 = (base * base).astype(t)
    s0 = (np.ones(3, t) * t(np.float32(specular)) * t(np.float32(0.08))).astype(t)
    cspec0 = (s0 + ((base2 - s0).astype(t) * t(np.float32(metallic))).astype(t)).astype(t)
    m = np.clip((t(1) - np.asarray(c, t)).astype(t), t(0), t(1))
    m2 = (m * m).astype(t)
    fh = ((m2 * m2).astype(t) * m).astype(t)
    return (cspec0[None] + ((t(1) - cspec0).astype(t)[None] * fh[:, None]).astype(t)).astype(t)


def added_radiance(c, reflected, strength, dtype=np.float64, **brdf):
    """(n, 3): strength (F (.) rgb_r) where alpha_r > 0, zeros elsewhere; reflected (n, 4) premultiplied"""
    t = dtype
    refl = np.asarray(reflected, np.float32).astype(t)
    F = fresnel(c, dtype=dtype, **{k: v for k, v in brdf.items() if k in ("basecolor", "metallic", "specular")})
    add = ((F * refl[:, :3]).astype(t) * t(np.float32(strength))).astype(t)
    return np.where((refl[:, 3] > 0)[:, None], add, t(0))


def render_with_reflection(meshes, matrix_3x4, width, height, focal, ambient_fn, factor=None, reflected=None, strength=1.0, sun_dir=SUN, basecolor=(0.8, 0.8, 0.8),
                           pixel_offset=(0.5, 0.5), **brdf):
    """mesh_sun_nerf_shadow_cases.render_with_sun_factor, its statements in its order, with `added_radiance` added to a covered pixel's colour
    behind the BRDF. reflected: None (nothing is added) or (h, w, 4), the premultiplied (rgb_r, alpha_r) of every pixel's mirror ray; what it
    holds where a pixel owns no ray is not looked at. Adds to that function's dict, per pixel: owns (h, w), rq and r (h, w, 3; float64, zeros
    without a ray), rq32 and r32 (float32), c and c32, t_hit (inf: no mesh in the way; 0 without a ray), t_unsafe (global_nearest's flag),
    F (h, w, 3), added (h, w, 3), added32 (the float32 form of the added term), and rq_dev / r_dev, the largest |rq32 - rq| / |r32 - r| on
    safe pixels that own a ray; t_hit32 (0 where t_hit is not finite) and t_dev, the largest |t_hit32 - t_hit| / max(1, t_hit) on safe cut rays."""
    meshes = [np.asarray(T, np.float32) for T in meshes]
    M = np.asarray(matrix_3x4, np.float32).astype(np.float64)
    lo, hi = [b.astype(np.float64) for b in ref.scene_box(meshes)]
    ys, xs = np.mgrid[0:height, 0:width]
    u = (xs.reshape(-1) + pixel_offset[0]) / width
    v = (ys.reshape(-1) + pixel_offset[1]) / height
    local = np.stack([(u - 0.5) * width / focal[0], (v - 0.5) * height / focal[1], np.ones_like(u)], 1)
    d = ref._unit(local @ M[:, :3].T)
    origin = np.broadcast_to(M[:, 3], d.shape)
    entry, _, _ = ref.box_entry(lo, hi, origin, d)
    start = origin + (np.maximum(np.where(np.isfinite(entry), entry, 0.0), 0.0) + 1e-6)[:, None] * d
    pos, nrm, hit, unsafe = ref.trace(meshes, start, d)
    covered = ref._inside(lo, hi, pos) & np.isfinite(entry)
    facing = np.where(((nrm * d).sum(1) < 0)[:, None], nrm, -nrm)
    sun = ref._unit(np.asarray(sun_dir, np.float64))
    spos = pos + ref.SHADOW_OFFSET * ref._unit(facing)
    q = spos
    s_entry, _, _ = ref.box_entry(lo, hi, spos, np.broadcast_to(sun, spos.shape))
    s_entry = np.where(np.isfinite(s_entry), s_entry, 3.402823466e+38)
    spos = spos + np.maximum(s_entry + 1e-6, 0.0)[:, None] * sun
    alive = ref._inside(lo, hi, spos)
    sdir = np.where(alive[:, None], sun, d)
    send, _, _, s_unsafe = ref.trace(meshes, spos, sdir)
    shadowed = ref._inside(lo, hi, send)
    N = ref._unit(np.where(hit[:, None], nrm, d))
    f = np.ones(width * height) if factor is None else np.broadcast_to(np.asarray(factor, np.float64).reshape(-1), (width * height,))
    light = ref.SUN_COLOUR * np.where(shadowed, 0.0, f)[:, None]
    base = np.asarray(basecolor, np.float32).astype(np.float64)
    amb = np.asarray(ambient_fn(pos, N), np.float64)
    f32 = {k: float(np.float32(x)) for k, x in brdf.items()}
    rgb, ndl, ndv = ref.shade(base * base, amb, light, sun, -d, N, **f32)
    # ---- the mirror ray and what it adds
    owns = covered & hit
    nh = ref._unit(facing)
    c = np.where(owns, -(nh * d).sum(1), 0.0)
    rq = np.where(owns[:, None], q, 0.0)
    r = np.where(owns[:, None], d + 2.0 * c[:, None] * nh, 0.0)
    t_hit, t_unsafe = np.zeros(width * height), np.zeros(width * height, bool)
    if owns.any():
        t_hit[owns], t_unsafe[owns] = ref.global_nearest(meshes, rq[owns], ref._unit(r[owns]))
    refl = np.zeros((width * height, 4), np.float32) if reflected is None else np.asarray(reflected, np.float32).reshape(-1, 4)
    refl = np.where(owns[:, None], refl, np.float32(0))
    shading = dict(basecolor=basecolor, **{k: x for k, x in brdf.items() if k in ("metallic", "specular")})
    F = fresnel(c, **shading)
    added = added_radiance(c, refl, strength, **shading)
    rq32, r32, c32 = _mirror32(meshes, M, d, entry, start, owns)
    added32 = added_radiance(c32, refl, strength, dtype=np.float32, **shading)
    t_hit32 = _t_hit32(meshes, rq, r, rq32, r32, owns & np.isfinite(t_hit))
    rgb = rgb + added
    rgba = np.zeros((width * height, 4))
    rgba[covered, :3], rgba[covered, 3] = rgb[covered], 1.0
    depth = np.where(covered, ((pos - M[:, 3]) * M[:, 2]).sum(1), ref.MAX_DEPTH)
    unsafe = unsafe | (covered & (s_unsafe | (np.abs(ndl) < ref.EDGE_EPS) | (np.abs(ndv) < ref.EDGE_EPS)))
    shape = (height, width)
    has = covered & ~shadowed
    q = np.where(has[:, None], q, 0.0)
    q32 = sc._q32(meshes, M, d, entry, start, has)
    m = has & ~unsafe
    dev = float(np.abs(q32.astype(np.float64) - q)[m].max()) if m.any() else 0.0
    mo = owns & ~unsafe
    rq_dev = float(np.abs(rq32.astype(np.float64) - rq)[mo].max()) if mo.any() else 0.0
    r_dev = float(np.abs(r32.astype(np.float64) - r)[mo].max()) if mo.any() else 0.0
    mt = mo & ~t_unsafe & np.isfinite(t_hit)
    t_dev = float((np.abs(t_hit32.astype(np.float64) - t_hit)[mt] / np.maximum(1.0, t_hit[mt])).max()) if mt.any() else 0.0
    return {"rgba": rgba.reshape(height, width, 4), "depth": depth.reshape(shape), "unsafe": unsafe.reshape(shape), "covered": covered.reshape(shape),
            "shadowed": (covered & shadowed).reshape(shape), "lit": (covered & ~shadowed & (ndl >= 0) & (ndv >= 0)).reshape(shape),
            "occluded": (covered & shadowed & (ndl >= 0) & (ndv >= 0)).reshape(shape),
            "pos": pos.reshape(height, width, 3), "N": N.reshape(height, width, 3), "view": (-d).reshape(height, width, 3),
            "has_ray": has.reshape(shape), "q": q.reshape(height, width, 3), "q32": q32.reshape(height, width, 3), "q_dev": dev,
            "owns": owns.reshape(shape), "rq": rq.reshape(height, width, 3), "rq32": rq32.reshape(height, width, 3), "r": r.reshape(height, width, 3),
            "r32": r32.reshape(height, width, 3), "c": c.reshape(shape), "c32": c32.reshape(shape), "t_hit": t_hit.reshape(shape),
            "t_unsafe": t_unsafe.reshape(shape), "F": F.reshape(height, width, 3), "added": added.reshape(height, width, 3),
            "added32": added32.reshape(height, width, 3), "rq_dev": rq_dev, "r_dev": r_dev, "t_hit32": t_hit32.reshape(shape), "t_dev": t_dev}


SHARED_KEYS = ("rgba", "depth", "unsafe", "covered", "shadowed", "lit", "occluded", "pos", "N", "view", "has_ray", "q", "q32", "q_dev")  # render_with_sun_factor's


def frame(case="A", reflected=None, strength=1.0, ambient_fn=sc.no_ambient, **opts):
    """the float64 frame of a case; the one that adds nothing is computed once per process and case"""
    if reflected is None and ambient_fn is sc.no_ambient and not opts:
        if case not in _cache:
            _cache[case] = render_with_reflection(meshes(case), CAMERA, WIDTH, HEIGHT, FOCAL, sc.no_ambient)
        return _cache[case]
    return render_with_reflection(meshes(case), CAMERA, WIDTH, HEIGHT, FOCAL, ambient_fn, None, reflected, strength, **opts)


def unit32(v):
    """normalize3 of a float32 program: one square root of (x x + y y) + z z and three quotients"""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    return (v / np.sqrt(_dot32(v, v))[:, None]).astype(np.float32)


def frame_bound(rgb_ref):
    """mesh_sun_nerf_shadow_cases' colour rule: GPU_FACTOR x the oracle's deviation on the frame `defaults` x max(1, |rgb_ref|)"""
    return sc.frame_bound(rgb_ref)
