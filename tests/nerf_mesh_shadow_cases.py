"""What test_nerf_mesh_shadow_cpu.py and test_nerf_mesh_shadow_gpu.py share (include/ngp_hip.h, "sun: the meshes in front of the sun on the
NeRF"): the scene and camera, and the float64 restatement of what the pass does to a NeRF pixel from (depth, camera, meshes).

The scene is irradiance_bounce_reference.floor_scene() (a slab under the NeRF's unit cube) plus a plate: mesh_cases.cube() scaled by
(1, 0.02, 1) and loaded with centre (0.5, 0.7, 0.0), which the loader leaves at [0.507, 1.190, 0.007] - [1.493, 1.210, 0.993], above half of
the cube on the side the sun (1, 1, 1) comes from. The camera stands in front of the cube below the plate's height and looks at the cube's
middle: the plate lies above its view, the floor behind the NeRF, so the frame has NeRF-over-floor pixels, NeRF-over-nothing pixels and bare
floor pixels. ("Nothing": a ray that enters no mesh's box leaves the mesh pass's opaque black pixel at no depth.) In this view every blocked
pixel has nothing behind it; CAMERA_ABOVE looks down far enough to put the floor behind some of them.

A pixel owns a surface point when the NeRF's alpha on it exceeds 0.2: p = o + d (depth - fwd . (o - pos)) / (fwd . d) on the pixel's own
ray, depth the NeRF pass's z-depth of that pixel. q = p + bias s^; blocked = a triangle of any mesh within 100 of q along s^
(mesh_reference.global_nearest); f = 1 - strength (float32) where blocked, else 1. surface_points32 is p as a float32 program forms it, every
product and sum rounded where it rounds it; it exists only to price float32."""
import numpy as np

import irradiance_bounce_reference as br
import mesh_cases as mc
import mesh_reference as ref
from mesh_sun_nerf_shadow_cases import s_hat

WIDTH, HEIGHT = 64, 48
FOCAL = (60.0, 60.0)
SUN = (1.0, 1.0, 1.0)
CAMERA = mc.look_at((0.5, 1.1, -0.9), (0.5, 0.45, 0.5), up=(0.0, 1.0, 0.0))
CAMERA_ABOVE = mc.look_at((0.5, 1.15, -0.7), (0.5, 0.2, 0.5), up=(0.0, 1.0, 0.0))  # a second view: the floor behind part of the shadowed NeRF
STRENGTH, BIAS = 0.5, 1e-2  # the bindings' defaults
OWNER_ALPHA = 0.2           # the NeRF pass writes a pixel's depth above this alpha
PLATE_CENTER = (0.5, 0.7, 0.0)
MIN_OWNERS, BLOCKED_SHARE, OPEN_SHARE = 200, 0.10, 0.30  # conditions on the case


def scene():
    """[(triangles, centre)]: the floor, and the plate between the sun and half of the NeRF"""
    plate = (mc.cube().astype(np.float64) * np.array([1.0, 0.02, 1.0])).astype(np.float32)
    return br.floor_scene() + [(plate, PLATE_CENTER)]


def meshes():
    return br.normalised(scene())


def pixel_rays(matrix_3x4=CAMERA, width=WIDTH, height=HEIGHT, focal=FOCAL, pixel_offset=(0.5, 0.5)):
    """(o, d, fwd, pos) in float64: the pinhole ray of every pixel, row by row, as mesh_volume_cases.render_with_ambient forms it"""
    M = np.asarray(matrix_3x4, np.float32).astype(np.float64)
    ys, xs = np.mgrid[0:height, 0:width]
    u = (xs.reshape(-1) + pixel_offset[0]) / width
    v = (ys.reshape(-1) + pixel_offset[1]) / height
    local = np.stack([(u - 0.5) * width / focal[0], (v - 0.5) * height / focal[1], np.ones_like(u)], 1)
    d = ref._unit(local @ M[:, :3].T)
    return np.broadcast_to(M[:, 3], d.shape), d, M[:, 2], M[:, 3]


def surface_points(depth, **cam):
    """(h w, 3) float64: the point at z-depth `depth` (h, w) on every pixel's ray"""
    o, d, fwd, pos = pixel_rays(**cam)
    t = (np.asarray(depth, np.float64).reshape(-1) - (o - pos) @ fwd) / (d @ fwd)
    return o + d * t[:, None]


def surface_points32(depth, matrix_3x4=CAMERA, width=WIDTH, height=HEIGHT, focal=FOCAL, pixel_offset=(0.5, 0.5)):
    """surface_points as a float32 program forms it: the pixel's direction (quotients, the matrix product column by column, the length as
    the square root of (x x + y y) + z z and three quotients), the distance along it, the point"""
    f = np.float32
    M = np.asarray(matrix_3x4, f)
    ys, xs = np.mgrid[0:height, 0:width]
    u = ((xs.reshape(-1).astype(f) + f(pixel_offset[0])) / f(width)).astype(f)
    v = ((ys.reshape(-1).astype(f) + f(pixel_offset[1])) / f(height)).astype(f)
    lx = (((u - f(0.5)) * f(width)).astype(f) / f(focal[0])).astype(f)
    ly = (((v - f(0.5)) * f(height)).astype(f) / f(focal[1])).astype(f)
    lz = np.ones_like(lx)
    d = ((M[:, 0][None] * lx[:, None]).astype(f) + (M[:, 1][None] * ly[:, None]).astype(f)).astype(f)
    d = (d + (M[:, 2][None] * lz[:, None]).astype(f)).astype(f)

    def dot(a, b):
        return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(f) + a[..., 2] * b[..., 2]).astype(f)

    d = (d / np.sqrt(dot(d, d)).astype(f)[:, None]).astype(f)
    fwd, pos = M[:, 2], M[:, 3]
    o = np.broadcast_to(pos, d.shape)
    t = ((np.asarray(depth, f).reshape(-1) - dot(o - pos, fwd[None])).astype(f) / dot(fwd[None], d)).astype(f)
    return (o + (d * t[:, None]).astype(f)).astype(f)


def shadow(nerf_alpha, depth, meshes_, strength=STRENGTH, bias=BIAS, sun_dir=SUN, **cam):
    """the pass restated in float64 from the NeRF's alpha (h, w) and depth (h, w). Returns a dict, per pixel: owner (alpha > 0.2), p (zeros
    for a pixel that owns no point), p32 and p_dev (the largest |p32 - p| on owners), blocked, unsafe (the float64 tracer's flag of the
    shadow ray), f (float32: 1 - strength where blocked, else 1) and record (p as float32 next to 2 blocked / 1 open / 0)."""
    a = np.asarray(nerf_alpha, np.float32)
    shape = a.shape
    owner = (a > np.float32(OWNER_ALPHA)).reshape(-1)
    p = np.where(owner[:, None], surface_points(depth, **cam), 0.0)
    p32 = np.where(owner[:, None], surface_points32(depth, **cam), np.float32(0))
    s = s_hat(sun_dir).astype(np.float64)
    blocked, unsafe = blocked_from(p[owner], meshes_, bias, sun_dir)
    full_blocked, full_unsafe = np.zeros(owner.size, bool), np.zeros(owner.size, bool)
    full_blocked[owner], full_unsafe[owner] = blocked, unsafe
    f = np.where(full_blocked, np.float32(1) - np.float32(strength), np.float32(1)).astype(np.float32)
    record = np.concatenate([p.astype(np.float32), np.where(owner, np.where(full_blocked, 2.0, 1.0), 0.0).astype(np.float32)[:, None]], 1)
    dev = float(np.abs(p32.astype(np.float64) - p)[owner].max()) if owner.any() else 0.0
    return {"owner": owner.reshape(shape), "p": p.reshape(shape + (3,)), "p32": p32.reshape(shape + (3,)), "p_dev": dev, "blocked": full_blocked.reshape(shape),
            "unsafe": full_unsafe.reshape(shape), "f": f.reshape(shape), "record": record.reshape(shape + (4,)), "s_hat": s}


def blocked_from(p, meshes_, bias=BIAS, sun_dir=SUN):
    """(blocked, unsafe) of the shadow rays from the points p (n, 3): q = p + bias s^ in float64, the nearest hit over all the meshes"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    if not p.shape[0]:
        return np.zeros(0, bool), np.zeros(0, bool)
    s = s_hat(sun_dir).astype(np.float64)
    t, unsafe = ref.global_nearest(meshes_, p + bias * s, np.broadcast_to(s, p.shape))
    return np.isfinite(t), unsafe


def composite(n, m, f):
    """the pass's output in float32, shade_ray's expression in shade_ray's order: (fl(n.rgb f) + fl(m.rgb k), n.a + fl(m.a k)), k = fl(1 - n.a);
    a pixel with n.a == 0 stays m. n, m: (..., 4) float32, f: (...) float32."""
    n, m, f = np.asarray(n, np.float32), np.asarray(m, np.float32), np.asarray(f, np.float32)
    k = (np.float32(1) - n[..., 3:4]).astype(np.float32)
    scaled = np.concatenate([(n[..., :3] * f[..., None]).astype(np.float32), n[..., 3:4]], -1)
    out = (scaled + (m * k).astype(np.float32)).astype(np.float32)
    return np.where(n[..., 3:4] == 0, m, out)
