"""What test_sun_disk_cpu.py and test_sun_disk_gpu.py share (include/ngp_hip.h, "sun: the sun's disk"): the table of shadow directions
restated in float64, the two cases, and the float64 restatement of what the option does to a mesh pixel and to a NeRF pixel.

Mesh side: irradiance_bounce_reference.floor_scene() plus a low plate, mesh_cases.cube() scaled by (1, 0.02, 1) and loaded with centre
(0.3, -0.4, 0.3), just above the floor, seen by mesh_sun_nerf_shadow_cases.CAMERA under the sun (1, 1, 1). M3's shadow ray from the floor
sees the floor alone, so without the option the plate throws no shadow onto the floor at all; with it the floor shows the plate's shadow
with a penumbra. NeRF side: nerf_mesh_shadow_cases' scene and its two cameras. Both with a disk of 5 degrees and 16 rays.

A pixel's count is the number of its K rays that mesh_reference.global_nearest finds blocked (a triangle of any mesh within 100); a ray the
float64 tracer flags is a tie a float32 tracer may decide either way, so a pixel with such a ray is left out of the count's comparison, and
the cases keep those pixels under UNSAFE_CAP."""
import math

import numpy as np

import irradiance_bounce_reference as br
import mesh_cases as mc
import mesh_reference as ref
import mesh_sun_nerf_shadow_cases as sc
import nerf_mesh_shadow_cases as nc

WIDTH, HEIGHT, FOCAL = sc.WIDTH, sc.HEIGHT, sc.FOCAL
SUN = (1.0, 1.0, 1.0)
RADIUS, K = 0.0872665, 16          # 5 degrees
REAL_SUN = 0.00465                 # the bindings' True
CAMERA = sc.CAMERA
PLATE_CENTER = (0.3, -0.4, 0.3)
CLASS_SHARE, UNSAFE_CAP = 0.10, 0.03  # conditions on the cases: each of open, partial and full; owner pixels with a flagged ray
ALLOWED_RAYS = (1, 2, 4, 8, 16)
_cache = {}


# ---------------------------------------------------------------------------------------------------------------- the table
def directions(sun_dir, angular_radius, n_rays, s=0):
    """(n_rays, 3) float32: the contract's table, every step in float64 in the contract's order and one rounding to float32 at the end.
    sun_dir and angular_radius are taken as the float32 values the library receives."""
    sd = np.asarray(sun_dir, np.float32).astype(np.float64)
    sh = sd / math.sqrt(sd[0] * sd[0] + sd[1] * sd[1] + sd[2] * sd[2])
    a = 0
    for j in (1, 2):
        if abs(sh[j]) < abs(sh[a]):
            a = j
    e = np.zeros(3)
    e[a] = 1.0
    c = np.array([e[1] * sh[2] - e[2] * sh[1], e[2] * sh[0] - e[0] * sh[2], e[0] * sh[1] - e[1] * sh[0]])
    u = c / math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    v = np.array([sh[1] * u[2] - sh[2] * u[1], sh[2] * u[0] - sh[0] * u[2], sh[0] * u[1] - sh[1] * u[0]])
    tr = math.tan(float(np.float32(angular_radius)))
    golden = math.pi * (3.0 - math.sqrt(5.0))
    turn = float(s) * 0.6180339887498949
    rot = 2.0 * math.pi * (turn - math.floor(turn))
    out = np.zeros((n_rays, 3), np.float32)
    for k in range(n_rays):
        r = math.sqrt((k + 0.5) / n_rays) if n_rays > 1 else 0.0
        phi = k * golden + rot
        m = tr * r
        w = sh + m * (math.cos(phi) * u + math.sin(phi) * v)
        out[k] = (w / math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])).astype(np.float32)
    return out


def counts(meshes_, q, dirs):
    """(count, flagged) of the points q (n, 3): how many of the directions dirs (K, 3) the float64 tracer finds blocked from each, and
    whether it flags any of a point's rays"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    count, flagged = np.zeros(q.shape[0], np.int64), np.zeros(q.shape[0], bool)
    if q.shape[0]:
        for d in np.asarray(dirs, np.float32).astype(np.float64):
            t, unsafe = ref.global_nearest(meshes_, q, np.broadcast_to(d, q.shape))
            count += np.isfinite(t)
            flagged |= unsafe
    return count, flagged


def visibility(count, n_rays):
    """V = (K - count) / K in float32 (exact for these K)"""
    return ((np.float32(n_rays) - np.asarray(count, np.float32)) / np.float32(n_rays)).astype(np.float32)


def factor(count, n_rays, strength):
    """f = fl(1 - fl(strength fl(count / K))) in float32"""
    blocked = (np.asarray(count, np.float32) / np.float32(n_rays)).astype(np.float32)
    return (np.float32(1) - (np.float32(strength) * blocked).astype(np.float32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- mesh side
def mesh_scene():
    """[(triangles, centre)]: the floor and the low plate"""
    plate = (mc.cube().astype(np.float64) * np.array([1.0, 0.02, 1.0])).astype(np.float32)
    return br.floor_scene() + [(plate, PLATE_CENTER)]


def mesh_meshes():
    return br.normalised(mesh_scene())


def mesh_geometry(pixel_offset=(0.5, 0.5), width=WIDTH, height=HEIGHT, meshes_=None, camera=None):
    """M1-M4 of mesh_sun_nerf_shadow_cases.render_with_sun_factor, its statements in its order, per pixel: pos, N, view, covered, hit, M4's
    shadowed, unsafe (the primary ray's flag and the shading's edge cases; M4's own ray is not looked at where a pixel owns a disk), and
    what the option adds: owner = covered and hit, q = pos + SHADOW_OFFSET unit(ff) (float64; zeros for the others). entry and start are
    the primary rays' box entry and start (what mesh_sun_nerf_shadow_cases._q32 begins from). meshes_, camera: another scene and view than
    the mesh side's (not cached)."""
    key = ("geometry", tuple(pixel_offset), width, height)
    if meshes_ is None and camera is None and key in _cache:
        return _cache[key]
    meshes = [np.asarray(T, np.float32) for T in (mesh_meshes() if meshes_ is None else meshes_)]
    M = np.asarray(CAMERA if camera is None else camera, np.float32).astype(np.float64)
    lo, hi = [b.astype(np.float64) for b in ref.scene_box(meshes)]
    ys, xs = np.mgrid[0:height, 0:width]
    u = (xs.reshape(-1) + pixel_offset[0]) / width
    v = (ys.reshape(-1) + pixel_offset[1]) / height
    local = np.stack([(u - 0.5) * width / FOCAL[0], (v - 0.5) * height / FOCAL[1], np.ones_like(u)], 1)
    d = ref._unit(local @ M[:, :3].T)
    origin = np.broadcast_to(M[:, 3], d.shape)
    entry, _, _ = ref.box_entry(lo, hi, origin, d)
    start = origin + (np.maximum(np.where(np.isfinite(entry), entry, 0.0), 0.0) + 1e-6)[:, None] * d
    pos, nrm, hit, unsafe = ref.trace(meshes, start, d)
    covered = ref._inside(lo, hi, pos) & np.isfinite(entry)
    facing = np.where(((nrm * d).sum(1) < 0)[:, None], nrm, -nrm)
    sun = ref._unit(np.asarray(SUN, np.float64))
    spos = pos + ref.SHADOW_OFFSET * ref._unit(facing)
    q = spos
    s_entry, _, _ = ref.box_entry(lo, hi, spos, np.broadcast_to(sun, spos.shape))
    s_entry = np.where(np.isfinite(s_entry), s_entry, 3.402823466e+38)
    spos = spos + np.maximum(s_entry + 1e-6, 0.0)[:, None] * sun
    alive = ref._inside(lo, hi, spos)
    send, _, _, s_unsafe = ref.trace(meshes, spos, np.where(alive[:, None], sun, d))
    shadowed = ref._inside(lo, hi, send)
    owner = covered & hit
    N = ref._unit(np.where(hit[:, None], nrm, d))
    g = dict(meshes=meshes, M=M, d=d, entry=entry, start=start, pos=pos, N=N, covered=covered, hit=hit, owner=owner, shadowed=shadowed, primary_unsafe=unsafe, shadow_unsafe=s_unsafe,
             q=np.where(owner[:, None], q, 0.0), sun=sun, shape=(height, width))
    if meshes_ is None and camera is None:
        _cache[key] = g
    return g


def mesh_colour(g, V, T_s=1.0, ambient_fn=sc.no_ambient, basecolor=(0.8, 0.8, 0.8), **brdf):
    """render_with_sun_factor's shading with light = SUN_COLOUR V T_s where the pixel owns a disk and SUN_COLOUR where(shadowed, 0, T_s)
    elsewhere. V, T_s: numbers or (h, w). Returns rgba (h, w, 4) float64 and unsafe (h, w): the pixels the comparison leaves out."""
    h, w = g["shape"]
    V = np.broadcast_to(np.asarray(V, np.float64).reshape(-1), (h * w,))
    T = np.broadcast_to(np.asarray(T_s, np.float64).reshape(-1), (h * w,))
    light = ref.SUN_COLOUR * np.where(g["owner"], V * T, np.where(g["shadowed"], 0.0, T))[:, None]
    base = np.asarray(basecolor, np.float32).astype(np.float64)
    amb = np.asarray(ambient_fn(g["pos"], g["N"]), np.float64)
    f32 = {k: float(np.float32(x)) for k, x in brdf.items()}
    rgb, ndl, ndv = ref.shade(base * base, amb, light, g["sun"], -g["d"], g["N"], **f32)
    rgba = np.zeros((h * w, 4))
    rgba[g["covered"], :3], rgba[g["covered"], 3] = rgb[g["covered"]], 1.0
    unsafe = g["primary_unsafe"] | (g["covered"] & (~g["owner"] & g["shadow_unsafe"] | (np.abs(ndl) < ref.EDGE_EPS) | (np.abs(ndv) < ref.EDGE_EPS)))
    return rgba.reshape(h, w, 4), unsafe.reshape(h, w)


def mesh_case(s=0, pixel_offset=(0.5, 0.5)):
    """the mesh side through mesh_reference with the restated table of spp index s: the geometry, and per pixel count (h, w), flagged
    (h, w) and V (float32)"""
    key = ("mesh_case", s, tuple(pixel_offset))
    if key not in _cache:
        g = mesh_geometry(pixel_offset)
        own = g["owner"]
        count, flagged = np.zeros(own.size, np.int64), np.zeros(own.size, bool)
        count[own], flagged[own] = counts(g["meshes"], g["q"][own], directions(SUN, RADIUS, K, s))
        _cache[key] = dict(g, count=count.reshape(g["shape"]), flagged=flagged.reshape(g["shape"]), V=visibility(count, K).reshape(g["shape"]))
    return _cache[key]


def classes(count, owner, n_rays=K):
    """(open, partial, full) among the owners"""
    c = np.asarray(count)[np.asarray(owner, bool)]
    return int((c == 0).sum()), int(((c > 0) & (c < n_rays)).sum()), int((c == n_rays).sum())


# ---------------------------------------------------------------------------------------------------------------- NeRF side
def nerf_shadow(nerf_alpha, depth, dirs, strength=nc.STRENGTH, bias=nc.BIAS, n_rays=K, **cam):
    """nerf_mesh_shadow_cases.shadow with the disk: owner and p are its own; count and flagged from q = p + bias s^ along dirs; f"""
    sh = nc.shadow(nerf_alpha, depth, nc.meshes(), strength, bias, **cam)
    owner = sh["owner"].reshape(-1)
    count, flagged = np.zeros(owner.size, np.int64), np.zeros(owner.size, bool)
    count[owner], flagged[owner] = counts_from_p(sh["p"].reshape(-1, 3)[owner], dirs, bias)
    shape = sh["owner"].shape
    f = np.where(owner, factor(count, n_rays, strength), np.float32(1)).astype(np.float32)
    return dict(owner=sh["owner"], p=sh["p"], p_dev=sh["p_dev"], count=count.reshape(shape), flagged=flagged.reshape(shape), f=f.reshape(shape))


def counts_from_p(p, dirs, bias=nc.BIAS):
    """counts() from q = p + bias s^, s^ the mesh pass's float32 central direction, formed in float64"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return counts(nc.meshes(), p + bias * sc.s_hat(nc.SUN).astype(np.float64), dirs)
