"""What test_mesh_volume_cpu.py and test_mesh_volume_gpu.py share: a float64 restatement of the mesh pass whose ambient light comes from a
caller's function (built from mesh_reference's own blocks), the volumes the ShadeIrradianceVolume frames are rendered with, which pixels
of such a frame a float32 renderer may legitimately colour differently, and the per-pixel colour bound the GPU frames are held to.

Volumes. Records are (probes, 28) in index order g = i + rx (j + ry k): 27 coefficients c[3 m + channel] and the weight w (0: dead).
  sky      2 x 2 x 2, every probe the one record whose E(N) / pi is the sky term of the frame `ambient_x` (or, with the up direction y,
           of `sun_down`): that term is of degree 1 in N, so nine coefficients hold it exactly and a ShadeIrradianceVolume frame with it
           must be the Shade frame.
  varying  4 x 3 x 3 seeded random records, two dead probes at the lattice points nearest the meshes.
Both span mesh_reference.scene_box of the render scene, padded by PAD a side.

The bound. A GPU frame's hit point may be off by delta = GPU_FACTOR ORACLE_DEV_FRAME["defaults"][0] max(1, depth), what the depth check
already allows. dE = the largest |E(p +- delta e_a) - E(p)| over the three axes (float64) is what that does to the volume's estimate; the
lookup itself is held to 256 ULP of its absolute scale (test_irradiance_volume.py::test_lookup_matches_reference); the ambient light enters
the colour through k = mix(0.2, FV, metallic) base^2 <= 1 (mesh_reference.shade). Hence
    |rgb - rgb_ref| <= GPU_FACTOR ORACLE_DEV_FRAME["defaults"][1] max(1, |rgb_ref|) + k (256 ULP scale + dE) / pi.
"""
import numpy as np

import irradiance_sh_reference as sh_ref
import mesh_cases as mc
import mesh_reference as ref

ULP = 2.0 ** -24
PAD = 0.25
FACE_MARGIN = 1e-3     # in cells: a hit point this close to a face between two cells may blend other probes in float32
MIN_WEIGHT = 0.05      # below it the blend renormalised by W is ill-conditioned
CLAMP_MARGIN = 1e-4    # |E| below this share of its absolute scale: the clamp at zero decides
VARYING_RES = (4, 3, 3)
VARYING_SEED = 11
VARYING_DEAD = ((1, 1, 1), (2, 1, 1))  # the lattice points nearest the meshes: (x, y, z) indices
SKY_AMBIENT = (0.3, 0.2, 0.1)          # FRAMES["ambient_x"] and FRAMES["sun_down"]


def render_with_ambient(meshes, matrix_3x4, width, height, focal, ambient_fn, sun_dir=(1.0, 1.0, 1.0), basecolor=(0.8, 0.8, 0.8), pixel_offset=(0.5, 0.5), **brdf):
    """mesh_reference.render restated from box_entry, trace, shade and scene_box, the ambient light of every pixel being
    ambient_fn(pos (n, 3), N (n, 3)) -> (n, 3). Returns render's dict and, per pixel, pos (h, w, 3), N (h, w, 3), view (h, w, 3: the unit
    vector towards the camera) and depth."""
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
    s_entry, _, _ = ref.box_entry(lo, hi, spos, np.broadcast_to(sun, spos.shape))
    s_entry = np.where(np.isfinite(s_entry), s_entry, 3.402823466e+38)
    spos = spos + np.maximum(s_entry + 1e-6, 0.0)[:, None] * sun
    alive = ref._inside(lo, hi, spos)
    sdir = np.where(alive[:, None], sun, d)
    send, _, _, s_unsafe = ref.trace(meshes, spos, sdir)
    shadowed = ref._inside(lo, hi, send)
    N = ref._unit(np.where(hit[:, None], nrm, d))
    light = ref.SUN_COLOUR * np.where(shadowed, 0.0, 1.0)[:, None]
    base = np.asarray(basecolor, np.float32).astype(np.float64)
    amb = np.asarray(ambient_fn(pos, N), np.float64)
    f32 = {k: float(np.float32(x)) for k, x in brdf.items()}
    rgb, ndl, ndv = ref.shade(base * base, amb, light, sun, -d, N, **f32)
    rgba = np.zeros((width * height, 4))
    rgba[covered, :3], rgba[covered, 3] = rgb[covered], 1.0
    depth = np.where(covered, ((pos - M[:, 3]) * M[:, 2]).sum(1), ref.MAX_DEPTH)
    unsafe = unsafe | (covered & (s_unsafe | (np.abs(ndl) < ref.EDGE_EPS) | (np.abs(ndv) < ref.EDGE_EPS)))
    shape = (height, width)
    return {"rgba": rgba.reshape(height, width, 4), "depth": depth.reshape(shape), "unsafe": unsafe.reshape(shape), "covered": covered.reshape(shape),
            "shadowed": (covered & shadowed).reshape(shape), "lit": (covered & ~shadowed & (ndl >= 0) & (ndv >= 0)).reshape(shape),
            "occluded": (covered & shadowed & (ndl >= 0) & (ndv >= 0)).reshape(shape),
            "pos": pos.reshape(height, width, 3), "N": N.reshape(height, width, 3), "view": (-d).reshape(height, width, 3)}


def sky_ambient_fn(ambientcolor, up_dir):
    """the Shade modes' ambient light, in mesh_reference.render's order of operations"""
    up = ref._unit(np.asarray(up_dir, np.float64))
    a = np.asarray(ambientcolor, np.float32).astype(np.float64)
    return lambda pos, N: a * (ref.SKY_COLOUR * (-(N * up).sum(1) * 0.5 + 0.5)[:, None])


def volume_ambient_fn(sh, res, lo, hi):
    """ShadeIrradianceVolume's: max(E(pos, N), 0) / pi"""
    return lambda pos, N: np.maximum(sh_ref.lookup(sh, res, lo, hi, pos, N)[0], 0.0) / np.pi


def volume_box():
    """the scene box of the render scene, padded by PAD a side; float32, as a volume descriptor holds it"""
    lo, hi = ref.scene_box(mc.normalised(mc.render_scene()))
    return (lo - np.float32(PAD)).astype(np.float32), (hi + np.float32(PAD)).astype(np.float32)


def sky_record(ambientcolor=SKY_AMBIENT, up_dir=(1.0, 0.0, 0.0)):
    """the 27 coefficients c (float64) with evaluate(c, N) / pi = ambientcolor SKY_COLOUR (0.5 - 0.5 N . up) for every unit N, and w = 1:
    solved by least squares over more directions than unknowns (the system is consistent, the residual is rounding)"""
    rng = np.random.default_rng(0)
    n = ref._unit(rng.normal(size=(64, 3)))
    want = np.pi * sky_ambient_fn(ambientcolor, up_dir)(None, n)
    c, *_ = np.linalg.lstsq(sh_ref.A * sh_ref.sh9(n), want, rcond=None)  # (9, 3)
    return np.concatenate([c.reshape(27), [1.0]])


def sky_volume(up_dir=(1.0, 0.0, 0.0)):
    """(records (8, 28) float64, res, lo, hi): the sky term of ambientcolor SKY_AMBIENT and `up_dir` (ambient_x: x; sun_down: the default y)"""
    lo, hi = volume_box()
    return np.tile(sky_record(up_dir=up_dir), (8, 1)), (2, 2, 2), lo, hi


def sky_scale():
    """the absolute scale sum_m A_m |c_m| |Y_m| of the sky record's E, bounded over N by its value with every |Y_m| at its maximum: what the
    lookup's 256 ULP refer to"""
    c = np.abs(sky_record()[:27].reshape(9, 3))
    ymax = np.abs(sh_ref.sh9(ref._unit(np.random.default_rng(1).normal(size=(4096, 3))))).max(0) * 1.01
    return float(((sh_ref.A * ymax)[:, None] * c).sum(0).max())


def varying_volume(seed=VARYING_SEED, dead=VARYING_DEAD):
    """(records (36, 28) float32, res, lo, hi): coefficients N(0, 1) with c_0 moved up by 3.5 so that most E > 0 (and, from this
    camera, a channel of a fifth of the pixels is not), the probes `dead` dead"""
    res = VARYING_RES
    rng = np.random.default_rng(seed)
    n = res[0] * res[1] * res[2]
    sh = rng.normal(size=(n, 28))
    sh[:, :3] += 3.5
    sh[:, 27] = rng.uniform(0.3, 1.0, n)
    for i, j, k in dead:
        sh[i + res[0] * (j + res[1] * k), 27] = 0.0
    lo, hi = volume_box()
    return sh.astype(np.float32), res, lo, hi


def as_grid(sh, res):
    """records in index order -> the (rz, ry, rx, 28) float32 array Context.set_irradiance_volume takes"""
    return np.ascontiguousarray(np.asarray(sh, np.float32).reshape(res[2], res[1], res[0], 28))


def volume_frame(meshes, name, sh, res, lo, hi, **opts):
    """the float64 ShadeIrradianceVolume frame of camera `name` with the geometry options `opts`, and what the GPU frame is held to:
    adds E, W, scale (h, w[, 3]), unsafe_volume (the pixels unsafe by the rules of the module docstring, the frame's own included) and
    bound (h, w, 3)."""
    fr = render_with_ambient(meshes, mc.camera_matrix(name), mc.WIDTH, mc.HEIGHT, mc.focal(name), volume_ambient_fn(sh, res, lo, hi), **opts)
    h, w = fr["depth"].shape
    pos, N = fr["pos"].reshape(-1, 3), fr["N"].reshape(-1, 3)
    E, W = sh_ref.lookup(sh, res, lo, hi, pos, N)
    scale, _ = sh_ref.lookup(sh, res, lo, hi, pos, N, absolute=True)
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    near_face = np.zeros(pos.shape[0], bool)
    for a in range(3):
        if res[a] > 1:
            s = (pos[:, a] - lo64[a]) / (hi64[a] - lo64[a]) * (res[a] - 1)
            near_face |= (np.abs(s - np.round(s)) < FACE_MARGIN) & (s > -FACE_MARGIN) & (s < res[a] - 1 + FACE_MARGIN)
    clamp = (np.abs(E) < CLAMP_MARGIN * scale).any(1)
    unsafe = fr["unsafe"].reshape(-1) | (fr["covered"].reshape(-1) & (near_face | (W < MIN_WEIGHT) | clamp))
    # the bound
    depth = fr["depth"].reshape(-1)
    delta = mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][0] * np.maximum(1.0, np.where(fr["covered"].reshape(-1), depth, 0.0))
    dE = np.zeros_like(E)
    for a in range(3):
        for sgn in (-1.0, 1.0):
            q = pos.copy()
            q[:, a] += sgn * delta
            dE = np.maximum(dE, np.abs(sh_ref.lookup(sh, res, lo, hi, q, N)[0] - E))
    base = np.asarray(opts.get("basecolor", (0.8, 0.8, 0.8)), np.float32).astype(np.float64)
    metallic = float(np.float32(opts.get("metallic", 0.0)))
    FV = ref.schlick((N * fr["view"].reshape(-1, 3)).sum(1))
    k = ref._mix(0.2, FV, metallic)[:, None] * (base * base)
    first = mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][1] * np.maximum(1.0, np.abs(fr["rgba"][..., :3].reshape(-1, 3)))
    fr.update(E=E.reshape(h, w, 3), W=W.reshape(h, w), scale=scale.reshape(h, w, 3), unsafe_volume=unsafe.reshape(h, w),
              bound=(first + k * (256 * ULP * scale + dE) / np.pi).reshape(h, w, 3), bound_first=first.reshape(h, w, 3),
              bound_dE=(k * dE / np.pi).reshape(h, w, 3))
    return fr


_cache = {}


def varying_frame(metallic=0.0):
    """volume_frame of the varying volume at the camera `defaults`, computed once per process and metallic"""
    key = ("varying", metallic)
    if key not in _cache:
        sh, res, lo, hi = varying_volume()
        _cache[key] = volume_frame(mc.normalised(mc.render_scene()), "defaults", sh, res, lo, hi, **({"metallic": metallic} if metallic else {}))
    return _cache[key]


def check_volume_frame(fr, rgba, depth, name="volume"):
    """a GPU frame against volume_frame's: coverage and depth by mesh_cases.compare_frame's rules on the pixels safe for the volume, the
    colour within the per-pixel bound. Returns (largest depth deviation, largest ratio of colour deviation to bound, safe covered pixels)."""
    view = dict(fr, unsafe=fr["unsafe_volume"])
    dd, _ = mc.compare_frame(name, view, rgba, depth)
    both = ~fr["unsafe_volume"] & fr["covered"]
    ratio = np.abs(rgba[..., :3][both] - fr["rgba"][..., :3][both]) / fr["bound"][both]
    return dd, float(ratio.max()) if both.any() else 0.0, int(both.sum())
