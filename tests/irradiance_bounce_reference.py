"""A restatement of the bounce contract (include/ngp_hip.h, "bounces") in numpy: the closest hit of a probe's sphere rays with its triangle
kept, the hit point and the normal turned against the ray, the source lookup, the radiance the hit throws back, the projection and the
series V_b = V_0 + R(V_{b-1}). Built from mesh_reference (the brute-force nearest hit over all triangles, which is global_nearest with
the triangle kept, and winding_normals), irradiance_sh_reference (project, lookup) and irradiance_visibility_reference (lookup_visible);
nothing here comes from the package or from oracle/.

Every step takes dtype = float64 (the reference) or float32. The float32 form runs the SAME steps in float32: the directions as a float32
program forms them, the hit distance by the ray / triangle expression of a float32 tracer on the reference's own triangle, the hit point
o + t w with the product rounded first, the blend corner by corner (irradiance_visibility_reference's float32 blend; the plain lookup is
that blend with every probe in sight). It exists only to price float32: the tests' allowances are multiples of its deviation from the
float64 form on the test's own inputs.

A ray is unsafe, and left out of comparisons, when mesh_reference flags its hit as ambiguous (EDGE_EPS, TIE_EPS, RANGE_EPS) or when
|N . w| < FACING_EPS: there a float32 program may legitimately hit another triangle, or turn the normal the other way."""
import numpy as np

import irradiance_sh_reference as sh_ref
import irradiance_visibility_reference as vr
import mesh_reference as ref

FACING_EPS = 1e-4
# the largest |Y_m| over the sphere, m = 0..8: what bounds |E| of a record from its coefficients
Y_MAX = np.array([0.5 * np.sqrt(1 / np.pi)] + [0.5 * np.sqrt(3 / np.pi)] * 3 + [0.25 * np.sqrt(15 / np.pi)] * 2 + [0.5 * np.sqrt(5 / np.pi)] + [0.25 * np.sqrt(15 / np.pi)] * 2)
OPEN_M1 = 1e18  # a distance map no point is ever behind: the visible blend with these maps is the plain one


def source(sh, res, lo, hi, maps=None, D=None, bias=0.0):
    """what a pass reads: the records (probes, 28) in index order, the lattice, and (for the visible lookup) the maps (probes, 64, 2), D and
    normal_bias"""
    return {"sh": np.asarray(sh, np.float32).reshape(-1, 28), "res": tuple(res), "lo": np.asarray(lo, np.float32), "hi": np.asarray(hi, np.float32),
            "maps": None if maps is None else np.asarray(maps, np.float32).reshape(-1, 64, 2), "D": D, "bias": bias}


def volume_scale(sh):
    """an upper bound of |E(n)| over every record and normal: max over probes and channels of sum_m A_m |c_m| max |Y_m|"""
    c = np.abs(np.asarray(sh, np.float64).reshape(-1, 28)[:, :27]).reshape(-1, 9, 3)
    return float(((sh_ref.A * Y_MAX)[None, :, None] * c).sum(1).max())


def hits(meshes, probes, nu, nv):
    """the closest hit of every probe's K sphere rays over all the triangles of all the (normalised, float32) meshes, in float64: a dict of
    t (P, K; inf: none), tri (P, K; the index into the concatenated triangles, -1), N (P, K, 3; the winding normal), unsafe (P, K), T"""
    T = np.concatenate([np.asarray(m, np.float32) for m in meshes]) if len(meshes) else np.zeros((0, 3, 3), np.float32)
    probes = np.asarray(probes, np.float32)
    P, dirs = probes.shape[0], sh_ref.sphere_dirs(nu, nv)
    K = dirs.shape[0]
    if T.shape[0] == 0:
        return {"t": np.full((P, K), np.inf), "tri": np.full((P, K), -1), "N": np.zeros((P, K, 3)), "unsafe": np.zeros((P, K), bool), "T": T}
    o, d = np.repeat(probes.astype(np.float64), K, 0), np.tile(dirs, (P, 1))
    t, idx, nrm, unsafe = ref.nearest_hit(T, o, d)
    unsafe = unsafe | ((idx >= 0) & (np.abs((nrm * d).sum(1)) < FACING_EPS))
    return {"t": t.reshape(P, K), "tri": idx.reshape(P, K), "N": nrm.reshape(P, K, 3), "unsafe": unsafe.reshape(P, K), "T": T}


def _tri_t32(tri, o, d):
    """the hit distance as a float32 tracer forms it (Triangle::ray_intersect's expression) for rays o, d against their own triangles tri (n, 3, 3)"""
    f = np.float32
    a, v1, v2 = tri[:, 0], (tri[:, 1] - tri[:, 0]).astype(f), (tri[:, 2] - tri[:, 0]).astype(f)
    rov0 = (o - a).astype(f)

    def cross(x, y):
        return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], 1).astype(f)

    def dot(x, y):
        return ((x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]).astype(f) + x[:, 2] * y[:, 2]).astype(f)

    n = cross(v1, v2)
    return (f(1) / dot(d, n) * -dot(n, rov0)).astype(f), n


def _lookup(src, p, n, dtype):
    if src["maps"] is None:
        if dtype == np.float64:
            return sh_ref.lookup(src["sh"], src["res"], src["lo"], src["hi"], p, n)
        probes = src["sh"].shape[0]
        open_maps = np.broadcast_to(np.float32([OPEN_M1, OPEN_M1 * OPEN_M1]), (probes, 64, 2))
        E, W, _ = vr.lookup_visible(src["sh"], src["res"], src["lo"], src["hi"], open_maps, OPEN_M1, 0.0, p, n, dtype=np.float32, points_dtype=np.float32)
        return E, W
    E, W, _ = vr.lookup_visible(src["sh"], src["res"], src["lo"], src["hi"], src["maps"], src["D"], src["bias"], p, n, dtype=dtype, points_dtype=dtype)
    return E, W


def bounce_rays(hit, probes, nu, nv, albedo, alpha, src, dtype=np.float64):
    """B (P, K, 3) of one pass from the source `src` at the hits `hit` (of `hits`): (1 - alpha) albedo max(E(h, N_ff), 0) / pi, 0 without a
    hit and where W = 0. alpha: (P, K) or None. Returns (B, info): info holds h, nff, E, W of the rays with a hit (flat) and their mask."""
    T_ = dtype
    probes = np.asarray(probes, np.float32)
    P, K = hit["t"].shape
    mask = (hit["tri"] >= 0).reshape(-1)
    B = np.zeros((P * K, 3), T_)
    albedo = np.broadcast_to(np.asarray(albedo, np.float32), (3,)).astype(T_)
    al = np.zeros(P * K, T_) if alpha is None else np.asarray(alpha, np.float32).reshape(-1).astype(T_)
    info = {"mask": mask.reshape(P, K)}
    if mask.any():
        o = np.repeat(probes, K, 0)[mask].astype(T_)
        d = np.tile(vr.sphere_dirs(nu, nv, T_), (P, 1))[mask].astype(T_)
        if dtype == np.float64:
            t, N = hit["t"].reshape(-1)[mask], hit["N"].reshape(-1, 3)[mask]
        else:
            t, n = _tri_t32(hit["T"][hit["tri"].reshape(-1)[mask]], o, d)
            N = (n / np.sqrt(((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]).astype(T_) + n[:, 2] * n[:, 2]).astype(T_))[:, None]).astype(T_)
        facing = ((N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]).astype(T_) + N[:, 2] * d[:, 2]).astype(T_) < 0
        nff = np.where(facing[:, None], N, -N).astype(T_)
        h = (o + (d * t[:, None]).astype(T_)).astype(T_)
        E, W = _lookup(src, h, nff, dtype)
        M = ((albedo[None, :] * np.maximum(E, 0.0).astype(T_)).astype(T_) / T_(np.pi)).astype(T_)
        M = np.where((W > 0)[:, None], M, T_(0))
        B[mask] = ((T_(1) - al[mask])[:, None] * M).astype(T_)
        info.update(h=h, nff=nff, E=E, W=W)
    return B.reshape(P, K, 3), info


def records(B, t, nu, nv):
    """R (P, 28) of a pass: the projection of B (P, K, 3) onto coefficients 0..26, and the unblocked fraction of t (P, K)"""
    c = sh_ref.project(np.asarray(B, np.float64), sh_ref.sphere_dirs(nu, nv)).reshape(B.shape[0], 27)
    return np.concatenate([c, np.isinf(np.asarray(t)).mean(1)[:, None]], 1)


def bounced(meshes, v0, res, lo, hi, nu, nv, albedo, n_bounces, alpha=None, maps=None, D=None, bias=0.0):
    """[V_0, V_1, ..., V_N] (probes, 28 each, float64) of the lattice's own probes: V_b = V_0 + R(V_{b-1}) on the 27 coefficients, float 27
    V_0's. Every pass reads the records as the float32 data a context would hold."""
    probes = vr.probe_positions(res, lo, hi)
    hit = hits(meshes, probes, nu, nv)
    v0 = np.asarray(v0, np.float64).reshape(-1, 28)
    out = [v0]
    for _ in range(n_bounces):
        B, _ = bounce_rays(hit, probes, nu, nv, albedo, alpha, source(out[-1].astype(np.float32), res, lo, hi, maps, D, bias))
        nxt = v0.copy()
        nxt[:, :27] += records(B, hit["t"], nu, nv)[:, :27]
        out.append(nxt)
    return out


# ------------------------------------------------------------------------------------- the cases the CPU and the GPU tests share
# K below one wave, a tail, one stride of the projection exactly, one past it, several
RAY_SHAPES = [(1, 1), (3, 5), (8, 8), (9, 9), (16, 16)]
STAGE_RES = (4, 1, 3)  # an axis of one probe
STAGE_LO, STAGE_HI = np.float32([-0.2, -0.3, -0.1]), np.float32([1.6, 1.4, 1.1])  # around irradiance_volume_cases' two meshes
STAGE_DEAD = (5, 10)
STAGE_ALBEDO = np.float32([0.9, 0.5, 0.2])
STAGE_BIAS = 0.02
_cache = {}


def stage_meshes():
    """irradiance_volume_cases.gen_meshes as the loader leaves them"""
    if "meshes" not in _cache:
        from irradiance_volume_cases import gen_meshes

        _cache["meshes"] = [ref.normalise(tris, c) for tris, c in gen_meshes()]
    return _cache["meshes"]


def stage_volume(seed=31):
    """(records (12, 28) float32, res, lo, hi): coefficients N(0, 1) with c_0 moved up by 3.5 so that most E > 0, the probes STAGE_DEAD dead"""
    rng = np.random.default_rng(seed)
    n = STAGE_RES[0] * STAGE_RES[1] * STAGE_RES[2]
    sh = rng.normal(size=(n, 28))
    sh[:, :3] += 3.5
    sh[:, 27] = rng.uniform(0.3, 1.0, n)
    sh[list(STAGE_DEAD), 27] = 0.0
    return sh.astype(np.float32), STAGE_RES, STAGE_LO, STAGE_HI


def stage_maps(seed=32):
    """(D, maps (12, 64, 2) float32): m1 uniform in [0.05 D, D], m2 = m1^2 + var, var uniform in [0, (0.2 D)^2], D the lattice's default"""
    D = vr.default_max_distance(STAGE_RES, STAGE_LO, STAGE_HI)
    rng = np.random.default_rng(seed)
    m1 = rng.uniform(0.05 * D, D, (12, 64))
    return D, np.stack([m1, m1 * m1 + rng.uniform(0.0, (0.2 * D) ** 2, (12, 64))], -1).astype(np.float32)


def stage_alpha(P, K, seed=33):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (P, K)).astype(np.float32)


def stage_case(nu, nv, visible):
    """the per-ray stage test's case at irradiance_volume_cases.GEN_POINTS: a dict of hit (of `hits`), alpha, B (float64), B32 (the float32
    form), safe (P, K), dev = the largest |B32 - B| on safe rays and allow = 256 ULP of the source volume's largest |E| / pi +
    mesh_cases.GPU_FACTOR dev"""
    key = ("stage", nu, nv, visible)
    if key not in _cache:
        import mesh_cases as mc
        from irradiance_volume_cases import GEN_POINTS

        sh, res, lo, hi = stage_volume()
        D, maps = stage_maps()
        src = source(sh, res, lo, hi, maps, D, STAGE_BIAS) if visible else source(sh, res, lo, hi)
        hit = hits(stage_meshes(), GEN_POINTS, nu, nv)
        alpha = stage_alpha(GEN_POINTS.shape[0], nu * nv)
        B, info = bounce_rays(hit, GEN_POINTS, nu, nv, STAGE_ALBEDO, alpha, src)
        B32, _ = bounce_rays(hit, GEN_POINTS, nu, nv, STAGE_ALBEDO, alpha, src, np.float32)
        safe = ~hit["unsafe"]
        dev = float(np.abs(B32.astype(np.float64) - B)[safe].max()) if safe.any() else 0.0
        _cache[key] = {"hit": hit, "alpha": alpha, "B": B, "B32": B32, "safe": safe, "dev": dev, "info": info,
                       "allow": 256 * 2.0 ** -24 * volume_scale(sh) / np.pi + mc.GPU_FACTOR * dev}
    return _cache[key]


# A probe sees the NeRF only from inside the NeRF's own box (the tracer marches inside it), and the synthetic test model leaves the box empty
# below y = 0.2. Both lattices below therefore lie inside the unit cube, above a floor slab just under it (y in [-0.105, -0.095] as the
# loader leaves it): their lowest probes look down through empty space, so nothing attenuates what the floor throws back at them.
# the end-to-end test: the floor and irradiance_volume_cases' torus, which reaches into the cube: (res, lo, hi, n_u, n_v)
E2E_CASE = ((3, 2, 2), np.float32([0.08, 0.06, 0.1]), np.float32([0.92, 0.7, 0.9]), 8, 8)
E2E_ALBEDO = np.float32([0.8, 0.6, 0.4])
# the effect test: the floor alone: (albedo, res, lo, hi, n_u, n_v)
FLOOR_CASE = (0.8, (2, 2, 2), np.float32([0.1, 0.05, 0.1]), np.float32([0.9, 0.6, 0.9]), 16, 16)
FLOOR_CENTER = (0.0, -0.6, 0.0)


def floor_scene():
    """[(triangles, centre)]: mesh_cases.cube scaled to (4, 0.04, 4)"""
    import mesh_cases as mc

    return [((mc.cube().astype(np.float64) * np.array([4.0, 0.04, 4.0])).astype(np.float32), FLOOR_CENTER)]


def e2e_scene():
    from irradiance_volume_cases import gen_meshes

    return floor_scene() + gen_meshes()[1:]


def normalised(scene):
    return [ref.normalise(tris, c) for tris, c in scene]
