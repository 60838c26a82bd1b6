"""What test_irradiance_visibility_cpu.py and test_irradiance_visibility_gpu.py share: the slab scene, the volumes with their distance maps,
the rules for points a float32 lookup may legitimately answer differently, and the ShadeIrradianceVolume frame with visibility and its bound.

The slab. The contract's example is a wall x in [0.08, 0.12], |y|, |z| <= 2 between the probes of a 2 x 2 x 2 volume over [-0.5, 0.5]^3, the
left probes (x = -0.5) holding the constant radiance 1 and the right ones 0.01. The mesh loader scales every mesh so that its longest side
is 1, so the GPU's slab is a cube scaled to (0.04, 4, 4) as the loader leaves it, and volume, points and D are carried into its frame by the
similarity x -> origin + sigma x (`SlabFrame`), under which every vis is unchanged (r, m1, sqrt(m2) and D all scale by sigma). Tests state
their points in the example's coordinates. `slab_t_max` is the analytic wall in either frame.

Unsafe points of a lookup (left out; their share is capped by mesh_cases.UNSAFE_CAP), by mesh_volume_cases' rules and one more:
  - within FACE_MARGIN (in cells) of a face between two cells: float32 may blend other probes;
  - W' < MIN_WEIGHT: the blend renormalised by W' is ill-conditioned;
  - within PROBE_MARGIN = 1e-3 of a live corner probe: the direction the map is read at is undefined there.

The frame's bound is mesh_volume_cases' with the lookup replaced:
    |rgb - rgb_ref| <= GPU_FACTOR ORACLE_DEV_FRAME["defaults"][1] max(1, |rgb_ref|) + k (256 ULP scale + dE) / pi,
dE = the largest |E(p +- delta e_a) - E(p)| of the VISIBLE lookup over the three axes in float64, delta the hit point's allowance
GPU_FACTOR ORACLE_DEV_FRAME["defaults"][0] max(1, depth), k = mix(0.2, FV, metallic) base^2 and scale the visible lookup's absolute scale.
vis is continuous in the point, so what the hit point's error does to it is inside dE; the maps are the renderer's own (read back), so
their error does not enter."""
import numpy as np

import irradiance_sh_reference as sh_ref
import irradiance_visibility_reference as vr
import mesh_cases as mc
import mesh_reference as ref
import mesh_volume_cases as mv

PROBE_MARGIN = 1e-3
SLAB_X = (0.08, 0.12)
SLAB_HALF = 2.0
SLAB_RES = (2, 2, 2)
SLAB_RAYS = (16, 16)
SLAB_SHARPNESS = 5
LEFT_RADIANCE, RIGHT_RADIANCE = 1.0, 0.01
BEHIND = (0.4, -0.3, 0.27)   # behind the wall, seen from the bright probes
LIT = (-0.3, 0.2, 0.1)       # on the bright side


# ------------------------------------------------------------------------------------------------------------- the slab
def slab_scene():
    """[(triangles, centre)]: mesh_cases.cube scaled to (0.04, 4, 4), 12 triangles"""
    tris = mc.cube().astype(np.float64) * np.array([SLAB_X[1] - SLAB_X[0], 2 * SLAB_HALF, 2 * SLAB_HALF])
    return [(tris.astype(np.float32), (0.0, 0.0, 0.0))]


class SlabFrame:
    """the similarity from the example's coordinates into the loaded slab's: x -> origin + sigma x"""

    def __init__(self):
        lo, hi = ref.mesh_box(mc.normalised(slab_scene())[0])
        lo, hi = lo.astype(np.float64), hi.astype(np.float64)
        self.sigma = float((hi[0] - lo[0]) / (SLAB_X[1] - SLAB_X[0]))
        self.origin = np.array([lo[0] - self.sigma * SLAB_X[0], 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])])
        self.half = float(0.5 * (hi[1] - lo[1]))
        self.x = (float(lo[0]), float(hi[0]))

    def points(self, p):
        return (self.origin + self.sigma * np.asarray(p, np.float64)).astype(np.float32)

    def box(self):
        return self.points((-0.5, -0.5, -0.5)), self.points((0.5, 0.5, 0.5))


def slab_t_max(o, d, x=SLAB_X, half=SLAB_HALF, centre=(0.0, 0.0)):
    """distance along unit directions d (K, 3) from origins o (P, 3) to the wall x in [x0, x1], |y - cy|, |z - cz| <= half: (P, K), inf
    without a hit. The origins lie outside the wall and within its y, z extent, so only the two large faces can be hit first."""
    o, d = np.asarray(o, np.float64)[:, None, :], np.asarray(d, np.float64)[None, :, :]
    face = np.where(o[..., 0] < x[0], x[0], x[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (face - o[..., 0]) / d[..., 0]
        y, z = o[..., 1] + t * d[..., 1], o[..., 2] + t * d[..., 2]
    hit = (t > 0) & np.isfinite(t) & (np.abs(y - centre[0]) <= half) & (np.abs(z - centre[1]) <= half)
    return np.where(hit, t, np.inf)


def constant_record(L):
    """the SH9 record of a constant radiance L in every channel: c_0 = 4 pi Y_0 L, so E(n) = pi L for every n; w = 1"""
    rec = np.zeros(28)
    rec[:3] = 4.0 * np.pi * 0.5 * np.sqrt(1.0 / np.pi) * L
    rec[27] = 1.0
    return rec


def slab_records():
    """(8, 28) float32 in index order: the probes at x = lo bright, those at x = hi dim"""
    return np.stack([constant_record(LEFT_RADIANCE if g % 2 == 0 else RIGHT_RADIANCE) for g in range(8)]).astype(np.float32)


def slab_volume(example=True):
    """(records, res, lo, hi, D, maps (8, 64, 2) float32) of the slab example, its maps from the analytic wall in float64. example: in the
    example's own coordinates; else in the loaded slab's frame."""
    if example:
        lo, hi = np.full(3, -0.5, np.float32), np.full(3, 0.5, np.float32)
        wall = dict(x=SLAB_X, half=SLAB_HALF, centre=(0.0, 0.0))
    else:
        fr = SlabFrame()
        lo, hi = fr.box()
        wall = dict(x=fr.x, half=fr.half, centre=(fr.origin[1], fr.origin[2]))
    D = vr.default_max_distance(SLAB_RES, lo, hi)
    dirs = vr.sphere_dirs(*SLAB_RAYS)
    t = slab_t_max(vr.probe_positions(SLAB_RES, lo, hi), dirs, **wall)
    maps, _ = vr.maps_from_rays(dirs, t, SLAB_SHARPNESS, D)
    return slab_records(), SLAB_RES, lo, hi, D, maps.astype(np.float32)


def as_map_grid(maps, res):
    """maps in index order -> the (rz, ry, rx, 64, 2) float32 array Context.set_irradiance_volume_visibility takes"""
    return np.ascontiguousarray(np.asarray(maps, np.float32).reshape(res[2], res[1], res[0], 64, 2))


# --------------------------------------------------------------------------------------------------- seeded maps and points
def seeded_maps(res, D, seed=21):
    """(probes, 64, 2) float32: m1 uniform in [0.05 D, D], m2 = m1^2 + var, var uniform in [0, (0.2 D)^2]"""
    rng = np.random.default_rng(seed)
    n = res[0] * res[1] * res[2]
    m1 = rng.uniform(0.05 * D, D, (n, 64))
    return np.stack([m1, m1 * m1 + rng.uniform(0.0, (0.2 * D) ** 2, (n, 64))], -1).astype(np.float32)


def seeded_points(lo, hi, n=2000, seed=22, outside=0.15):
    """n points, the share `outside` of them up to a quarter of the box's size beyond it, and random normals: float32"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    p = rng.uniform(lo, hi, (n, 3))
    k = int(outside * n)
    p[:k] = rng.uniform(lo - 0.25 * ext, hi + 0.25 * ext, (k, 3))
    return p.astype(np.float32), ref._unit(rng.normal(size=(n, 3))).astype(np.float32)


def unsafe_points(res, lo, hi, p, W, info):
    """the module docstring's rules for lookup points"""
    lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p = np.asarray(p, np.float64)
    near_face = np.zeros(p.shape[0], bool)
    for a in range(3):
        if res[a] > 1:
            s = (p[:, a] - lo64[a]) / (hi64[a] - lo64[a]) * (res[a] - 1)
            near_face |= (np.abs(s - np.round(s)) < mv.FACE_MARGIN) & (s > -mv.FACE_MARGIN) & (s < res[a] - 1 + mv.FACE_MARGIN)
    near_probe = ((info["r"] < PROBE_MARGIN) & (info["wgt"] > 0)).any(1)
    return near_face | (W < mv.MIN_WEIGHT) | near_probe


def lookup_allowance(sh, res, lo, hi, maps, D, bias, p, n):
    """(E, W', scale, unsafe, allowance for E (n, 3), allowance for W'): 256 ULP of the absolute scale (the plain lookup's allowance) plus
    GPU_FACTOR x the largest deviation of the float32 restatement of the visibility-weighted blend from float64 over the safe points,
    relative to the scale"""
    E, W, info = vr.lookup_visible(sh, res, lo, hi, maps, D, bias, p, n)
    scale, _, _ = vr.lookup_visible(sh, res, lo, hi, maps, D, bias, p, n, absolute=True)
    E32, W32, _ = vr.lookup_visible(sh, res, lo, hi, maps, D, bias, p, n, dtype=np.float32)
    unsafe = unsafe_points(res, lo, hi, p, W, info)
    safe = ~unsafe
    smax = np.maximum(scale, 1e-30)
    dev = float((np.abs(E32 - E) / smax)[safe].max()) if safe.any() else 0.0
    dev_w = float(np.abs(W32 - W)[safe].max()) if safe.any() else 0.0
    return E, W, scale, unsafe, 256 * mv.ULP * scale + mc.GPU_FACTOR * dev * scale, 256 * mv.ULP + mc.GPU_FACTOR * dev_w, info


# ------------------------------------------------------------------------------------------------------------ the frame
VARYING_RAYS = (16, 16)
VARYING_SHARPNESS = 5
# the varying lattice's cells are several times the meshes' size, so with the default D (1.5 cell diagonals) hardly a texel sees a mesh and
# every vis is 1. D = 6 lies below the cell's diagonal (8.2): the far corners of every cell are weighted down by the Chebyshev term (its
# m1 the capped distance, lowered where the meshes are seen), the near ones are not
VARYING_MAX_DISTANCE = 6.0


def varying_visibility():
    """(D, maps (36, 64, 2) float32) of mesh_volume_cases.varying_volume's lattice among the render scene's meshes, in float64 from the
    brute-force nearest hit over all triangles: what the CPU test reasons from (the GPU tests read the renderer's own maps back)"""
    if "varying_maps" not in _cache:
        _, res, lo, hi = mv.varying_volume()
        D = np.float32(VARYING_MAX_DISTANCE)
        dirs = vr.sphere_dirs(*VARYING_RAYS)
        pos = vr.probe_positions(res, lo, hi).astype(np.float64)
        o = np.repeat(pos, dirs.shape[0], 0)
        d = np.tile(dirs, (pos.shape[0], 1))
        t, _ = ref.global_nearest(mc.normalised(mc.render_scene()), o, d)
        maps, _ = vr.maps_from_rays(dirs, t.reshape(pos.shape[0], -1), VARYING_SHARPNESS, D)
        _cache["varying_maps"] = (D, maps.astype(np.float32))
    return _cache["varying_maps"]


def visible_volume_frame(meshes, name, sh, res, lo, hi, maps, D, bias=0.0, **opts):
    """mesh_volume_cases.volume_frame with the visible lookup: the float64 frame and what a GPU frame is held to. Adds E, W, scale,
    min_vis (h, w: the smallest vis among a pixel's live corners), unsafe_volume and bound."""
    look = lambda p, n, **kw: vr.lookup_visible(sh, res, lo, hi, maps, D, bias, p, n, points_dtype=np.float64, **kw)  # (the frame's own float64 hit points)
    fr = mv.render_with_ambient(meshes, mc.camera_matrix(name), mc.WIDTH, mc.HEIGHT, mc.focal(name), lambda pos, N: np.maximum(look(pos, N)[0], 0.0) / np.pi, **opts)
    h, w = fr["depth"].shape
    pos, N = fr["pos"].reshape(-1, 3), fr["N"].reshape(-1, 3)
    E, W, info = look(pos, N)
    scale, _, _ = look(pos, N, absolute=True)
    clamp = (np.abs(E) < mv.CLAMP_MARGIN * scale).any(1)
    covered = fr["covered"].reshape(-1)
    unsafe = fr["unsafe"].reshape(-1) | (covered & (unsafe_points(res, lo, hi, pos, W, info) | clamp))
    depth = fr["depth"].reshape(-1)
    delta = mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][0] * np.maximum(1.0, np.where(covered, depth, 0.0))
    dE = np.zeros_like(E)
    for a in range(3):
        for sgn in (-1.0, 1.0):
            q = pos.copy()
            q[:, a] += sgn * delta
            dE = np.maximum(dE, np.abs(look(q, N)[0] - E))
    base = np.asarray(opts.get("basecolor", (0.8, 0.8, 0.8)), np.float32).astype(np.float64)
    metallic = float(np.float32(opts.get("metallic", 0.0)))
    FV = ref.schlick((N * fr["view"].reshape(-1, 3)).sum(1))
    k = ref._mix(0.2, FV, metallic)[:, None] * (base * base)
    first = mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][1] * np.maximum(1.0, np.abs(fr["rgba"][..., :3].reshape(-1, 3)))
    live = info["wgt"] > 0
    fr.update(E=E.reshape(h, w, 3), W=W.reshape(h, w), scale=scale.reshape(h, w, 3), unsafe_volume=unsafe.reshape(h, w),
              min_vis=np.where(live, info["vis"], 1.0).min(1).reshape(h, w), clamped=(covered & (E < 0).any(1)).reshape(h, w),
              bound=(first + k * (256 * mv.ULP * scale + dE) / np.pi).reshape(h, w, 3))
    return fr


_cache = {}


def varying_visible_frame(metallic=0.0, maps=None, D=None):
    """visible_volume_frame of the varying volume at the camera `defaults`; maps None: varying_visibility's (computed once per process and
    metallic), else the caller's (the renderer's own)"""
    key = ("frame", metallic)
    if maps is None and key in _cache:
        return _cache[key]
    sh, res, lo, hi = mv.varying_volume()
    if maps is None:
        D0, m = varying_visibility()
    else:
        D0, m = D, maps
    fr = visible_volume_frame(mc.normalised(mc.render_scene()), "defaults", sh, res, lo, hi, m, D0, **({"metallic": metallic} if metallic else {}))
    if maps is None:
        _cache[key] = fr
    return fr
