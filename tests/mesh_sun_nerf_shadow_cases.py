"""What test_mesh_sun_nerf_shadow_cpu.py and test_mesh_sun_nerf_shadow_gpu.py share (include/ngp_hip.h, "sun: the NeRF in front of the frames'
sun"): the scene and camera, and mesh_volume_cases.render_with_ambient restated with a per-pixel factor on the sun, which also returns where
each pixel's shadow ray through the NeRF starts.

The scene is irradiance_bounce_reference.floor_scene() (a slab under the NeRF's unit cube) under the sun (1, 1, 1). The camera stands over
the corner of the floor the sun points away from and looks down at it, so that the captured object's shadow falls on visible floor and
little of the object itself is in front of it.

A pixel has a shadow ray when its primary ray hits a mesh inside the scene box and the meshes do not shadow the hit. Its origin is
q = pos + SHADOW_OFFSET unit(ff), ff the winding normal turned against the primary ray: the mesh shadow ray's own origin before it is moved
to the scene box. q32 is the same in float32, every product and sum rounded where a float32 program rounds it, the hit distance by the ray /
triangle expression of a float32 tracer on the reference's own triangle (irradiance_bounce_reference._tri_t32); which pixels have a ray is the
float64 form's decision. It exists only to price float32."""
import numpy as np

import irradiance_bounce_reference as br
import mesh_cases as mc
import mesh_reference as ref
import mesh_volume_cases as mv

WIDTH, HEIGHT = 64, 48
FOCAL = (60.0, 60.0)
SUN = (1.0, 1.0, 1.0)
CAMERA = mc.look_at((-0.35, 1.3, -0.35), (0.3, -0.1, 0.3), up=(0.0, 1.0, 0.0))
BLOCKED_SHARE, OPEN_SHARE, MIN_RAYS = 0.10, 0.30, 200  # conditions on the case: alpha_s > 0.9, alpha_s = 0, pixels with a shadow ray
_cache = {}


def scene():
    return br.floor_scene()


def meshes():
    return br.normalised(scene())


def render_with_sun_factor(meshes, matrix_3x4, width, height, focal, ambient_fn, factor=None, sun_dir=SUN, basecolor=(0.8, 0.8, 0.8), pixel_offset=(0.5, 0.5), **brdf):
    """mesh_volume_cases.render_with_ambient, its statements in its order, with light = SUN_COLOUR where(shadowed, 0, factor): factor None
    (ones), a number or one value a pixel (h, w). Adds to its dict, per pixel: has_ray (h, w), q (h, w, 3; float64, zeros without a ray),
    q32 (float32) and q_dev, the largest |q32 - q| on safe pixels with a ray."""
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
    rgba = np.zeros((width * height, 4))
    rgba[covered, :3], rgba[covered, 3] = rgb[covered], 1.0
    depth = np.where(covered, ((pos - M[:, 3]) * M[:, 2]).sum(1), ref.MAX_DEPTH)
    unsafe = unsafe | (covered & (s_unsafe | (np.abs(ndl) < ref.EDGE_EPS) | (np.abs(ndv) < ref.EDGE_EPS)))
    shape = (height, width)
    has = covered & ~shadowed
    q = np.where(has[:, None], q, 0.0)
    q32 = _q32(meshes, M, d, entry, start, has)
    m = has & ~unsafe
    dev = float(np.abs(q32.astype(np.float64) - q)[m].max()) if m.any() else 0.0
    return {"rgba": rgba.reshape(height, width, 4), "depth": depth.reshape(shape), "unsafe": unsafe.reshape(shape), "covered": covered.reshape(shape),
            "shadowed": (covered & shadowed).reshape(shape), "lit": (covered & ~shadowed & (ndl >= 0) & (ndv >= 0)).reshape(shape),
            "occluded": (covered & shadowed & (ndl >= 0) & (ndv >= 0)).reshape(shape),
            "pos": pos.reshape(height, width, 3), "N": N.reshape(height, width, 3), "view": (-d).reshape(height, width, 3),
            "has_ray": has.reshape(shape), "q": q.reshape(height, width, 3), "q32": q32.reshape(height, width, 3), "q_dev": dev}


def _q32(meshes, M, d, entry, start, has):
    """q of the pixels `has` as a float32 program forms it, on the reference's own triangles"""
    f = np.float32
    out = np.zeros((d.shape[0], 3), f)
    if not has.any():
        return out
    _, mesh, idx, _, _, _ = ref.reference_rule_hit(meshes, start, d)
    d32 = d[has].astype(f)
    step = (np.maximum(np.where(np.isfinite(entry[has]), entry[has], 0.0), 0.0).astype(f) + f(1e-6)).astype(f)
    o32 = (M[:, 3].astype(f) + (d32 * step[:, None]).astype(f)).astype(f)
    tri = np.stack([meshes[m][i] for m, i in zip(mesh[has], idx[has])]).astype(f)
    t, n = br._tri_t32(tri, o32, d32)
    pos = (o32 + (d32 * t[:, None]).astype(f)).astype(f)
    nn = (n / np.sqrt(((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]).astype(f) + n[:, 2] * n[:, 2]).astype(f))[:, None]).astype(f)
    turned = ((nn[:, 0] * d32[:, 0] + nn[:, 1] * d32[:, 1]).astype(f) + nn[:, 2] * d32[:, 2]).astype(f) < 0
    nff = np.where(turned[:, None], nn, -nn).astype(f)
    out[has] = (pos + (nff * f(ref.SHADOW_OFFSET)).astype(f)).astype(f)
    return out


def s_hat(sun_dir=SUN):
    """the shadow rays' direction as the mesh pass forms it: normalize(normalize(sun_dir)) in float32, each length the square root of
    (x x + y y) + z z and three quotients"""
    f = np.float32
    v = np.asarray(sun_dir, f)
    for _ in range(2):
        v = (v / np.sqrt(((v[0] * v[0] + v[1] * v[1]).astype(f) + v[2] * v[2]).astype(f))).astype(f)
    return v


def no_ambient(pos, N):
    """Shade with the default ambientcolor (0, 0, 0)"""
    return np.zeros_like(pos)


def frame(factor=None, ambient_fn=no_ambient, **opts):
    """the float64 frame of the case; the one without a factor is computed once per process"""
    if factor is None and ambient_fn is no_ambient and not opts:
        if "plain" not in _cache:
            _cache["plain"] = render_with_sun_factor(meshes(), CAMERA, WIDTH, HEIGHT, FOCAL, no_ambient)
        return _cache["plain"]
    return render_with_sun_factor(meshes(), CAMERA, WIDTH, HEIGHT, FOCAL, ambient_fn, factor, **opts)


def factor_of(alpha_s):
    """T_s = max(1 - alpha_s, 0) in float32"""
    a = np.asarray(alpha_s, np.float32)
    return np.maximum((np.float32(1) - a).astype(np.float32), np.float32(0))


def frame_bound(rgb_ref):
    """mesh_volume_cases' colour rule without its lookup term: GPU_FACTOR x the oracle's deviation on the frame `defaults` x max(1, |rgb_ref|)"""
    return mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][1] * np.maximum(1.0, np.abs(rgb_ref))
