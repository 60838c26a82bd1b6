"""What test_ambient_change_cpu.py and test_ambient_change_gpu.py share (include/ngp_hip.h, "ambient: what the inserted meshes change in
the ambient light on the NeRF"): the two volumes of the case, the float64 restatement of the ratio g = E_after / E_before with its states
and clamps, the tolerance and tie rule of a float32 evaluation of it, and the composite.

The scene and camera are nerf_mesh_shadow_cases' own (floor plus plate, 64 x 48, the unit model). The volumes are built in float64 from the
meshes alone, so that the CPU can check the case: a lattice of RES probes over [LO, HI], N_U x N_V sphere rays a probe, the rays' hits from
irradiance_bounce_reference.hits, the records from irradiance_sh_reference.project. BEFORE sees the sky SKY on every ray; AFTER sees SKY on
open rays and BOUNCE, a reddish dim surface, on blocked ones. Float 27 of a record is the probe's open share in both volumes, so a probe
inside a mesh would be dead in both (the case has none). The records are rounded to float32, as a context holds them, and every
restatement reads those.

The ratio at (p, N): (E_a, W_a) and (E_b, W_b) are irradiance_sh_reference.lookup in AFTER and BEFORE. state = 1 and g = 1 where W_a = 0
or W_b = 0, else state = 2 and per channel a = max(E_a, 0), b = E_b, g = b > min_irradiance ? min(a / b, max_gain) : 1.

Tolerance of a float32 evaluation, derived: g = a / b with a off by dE_a and b by dE_b moves by at most (dE_a + g dE_b) / E_b to first
order; dE = LOOKUP_ULPS x 2^-24 x the absolute=True lookup's scale, LOOKUP_ULPS = 256 being what test_irradiance_volume.py grants
irradiance_volume_lookup, the device function both lookups are. Tie cases, left out (at most TIE_CAP of the points): a point within
mesh_volume_cases.FACE_MARGIN cells of a cell face, W_a or W_b below MIN_WEIGHT, E_a within CLAMP_MARGIN of its scale of 0, E_b within it
of min_irradiance, a within it of max_gain b."""
import numpy as np

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import mesh_volume_cases as mv
import nerf_mesh_shadow_cases as nc

RES = (4, 4, 4)
LO, HI = np.float32([-0.25, -0.25, -0.25]), np.float32([1.25, 1.45, 1.25])
N_U, N_V = 8, 8
SKY = (0.9, 0.8, 0.7)
BOUNCE = (0.25, 0.05, 0.05)
MIN_IRRADIANCE, MAX_GAIN = 1e-3, 4.0  # the bindings' defaults
LOOKUP_ULPS = 256                     # test_irradiance_volume.py's allowance for irradiance_volume_lookup, in ULP of the absolute scale
TIE_CAP = 0.02
STAGE_SEED, STAGE_POINTS, STAGE_PAD = 41, 400, 0.2  # (the pad: a share of the box's extent on every side)

_cache = {}


def volumes():
    """(after, before, hit): records (64, 28) float32 each in index order, and the float64 hits they were made from; once per process"""
    if "v" not in _cache:
        probes = sh_ref.volume_points(RES, LO, HI).astype(np.float32)
        hit = br.hits(nc.meshes(), probes, N_U, N_V)
        dirs = sh_ref.sphere_dirs(N_U, N_V)
        is_open = np.isinf(hit["t"])
        share = is_open.mean(1)[:, None]
        sky = np.broadcast_to(np.float64(SKY), is_open.shape + (3,))
        lit = np.where(is_open[..., None], sky, np.float64(BOUNCE))
        before = np.concatenate([sh_ref.project(sky, dirs).reshape(-1, 27), share], 1).astype(np.float32)
        after = np.concatenate([sh_ref.project(lit, dirs).reshape(-1, 27), share], 1).astype(np.float32)
        _cache["v"] = (after, before, hit)
    return _cache["v"]


def ratio(after, before, res, lo, hi, p, n, min_irradiance=MIN_IRRADIANCE, max_gain=MAX_GAIN):
    """the ratio in float64 at points p (k, 3) with normals n (k, 3). Returns a dict: g (k, 3), state (k,), E_a, E_b, W_a, W_b, scale_a,
    scale_b (the absolute=True lookups), allow (k, 3: the tolerance of a float32 evaluation) and tie (k,)"""
    p, n = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(n, np.float64).reshape(-1, 3)
    lo_, hi_ = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    mi, mg = float(np.float32(min_irradiance)), float(np.float32(max_gain))
    Ea, Wa = sh_ref.lookup(after, res, lo_, hi_, p, n)
    Eb, Wb = sh_ref.lookup(before, res, lo_, hi_, p, n)
    sa, _ = sh_ref.lookup(after, res, lo_, hi_, p, n, absolute=True)
    sb, _ = sh_ref.lookup(before, res, lo_, hi_, p, n, absolute=True)
    none = (Wa == 0) | (Wb == 0)
    a = np.maximum(Ea, 0.0)
    use = (Eb > mi) & ~none[:, None]
    g = np.where(use, np.minimum(a / np.where(use, Eb, 1.0), mg), 1.0)
    state = np.where(none, 1.0, 2.0)
    ulp = LOOKUP_ULPS * mv.ULP
    allow = np.where(use, (ulp * sa + g * ulp * sb) / np.where(use, Eb, 1.0), 0.0)
    near_face = np.zeros(p.shape[0], bool)
    lo64, hi64 = lo_.astype(np.float64), hi_.astype(np.float64)
    for ax in range(3):
        if res[ax] > 1:
            s = (p[:, ax] - lo64[ax]) / (hi64[ax] - lo64[ax]) * (res[ax] - 1)
            near_face |= (np.abs(s - np.round(s)) < mv.FACE_MARGIN) & (s > -mv.FACE_MARGIN) & (s < res[ax] - 1 + mv.FACE_MARGIN)
    clamp = (np.abs(Ea) < mv.CLAMP_MARGIN * sa) | (np.abs(Eb - mi) < mv.CLAMP_MARGIN * sb) | (np.abs(a - mg * Eb) < mv.CLAMP_MARGIN * (sa + mg * sb))
    tie = near_face | (~none & ((Wa < mv.MIN_WEIGHT) | (Wb < mv.MIN_WEIGHT))) | (~none & clamp.any(1))
    return dict(g=g, state=state, E_a=Ea, E_b=Eb, W_a=Wa, W_b=Wb, scale_a=sa, scale_b=sb, allow=allow, tie=tie, near_face=near_face)


def case_ratio(p, n, **kw):
    """ratio() in the case's two volumes"""
    after, before, _ = volumes()
    return ratio(after, before, RES, LO, HI, p, n, **kw)


def stage_points(res, lo, hi, seed=STAGE_SEED, count=STAGE_POINTS):
    """(p, n) float32: points inside the box and up to STAGE_PAD of its extent outside it, normals of any length; what the stage tests evaluate"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p = rng.uniform(lo - STAGE_PAD * (hi - lo), hi + STAGE_PAD * (hi - lo), (count, 3)).astype(np.float32)
    n = (rng.normal(size=(count, 3)) * rng.uniform(0.1, 10.0, (count, 1))).astype(np.float32)
    return p, n


def varying_pair():
    """(after, before, res, lo, hi): mesh_volume_cases.varying_volume, which has dead probes, under two seeds, with the constant term it
    moves up by 3.5 moved down again by 2.5 and 3 and one whole cell of `before` dead: E_after below zero, E_before below min_irradiance, ratios
    above the cap and points without an estimate all occur"""
    after, res, lo, hi = mv.varying_volume()
    before, _, _, _ = mv.varying_volume(seed=mv.VARYING_SEED + 1)
    after, before = after.copy(), before.copy()
    after[:, :3] -= np.float32(2.5)
    before[:, :3] -= np.float32(3.0)
    for i, j, k in np.ndindex(2, 2, 2):  # and the eight probes of the first cell dead in `before`: W_before = 0 throughout that cell
        before[i + res[0] * (j + res[1] * k), 27] = 0.0
    return after, before, res, lo, hi


def composite(n, m, g, f):
    """the frame in float32: (fl(fl(n.rgb g) f) + fl(m.rgb k), n.a + fl(m.a k)), k = fl(1 - n.a); a pixel with n.a == 0 stays m.
    n, m: (..., 4) float32, g: (..., 3), f: (...)"""
    n = np.asarray(n, np.float32)
    scaled = np.concatenate([(n[..., :3] * np.asarray(g, np.float32)).astype(np.float32), n[..., 3:4]], -1)
    return nc.composite(scaled, m, f)


def normals_from_gradient(grad, aabb_diag=(1.0, 1.0, 1.0)):
    """the marching-cubes export's rule in float32: N = -(grad / diag) / |grad / diag|, the length the square root of (x x + y y) + z z;
    (N (k, 3), ok (k,)): zeros and False where the length is zero or not finite"""
    f = np.float32
    g = (np.asarray(grad, f) / np.asarray(aabb_diag, f)).astype(f)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ln = np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(f) + g[:, 2] * g[:, 2]).astype(f)).astype(f)
        ok = (ln > 0) & np.isfinite(ln)
        N = np.where(ok[:, None], (-g / np.where(ok, ln, f(1))[:, None]).astype(f), f(0))
    return N.astype(f), ok
