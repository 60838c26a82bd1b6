"""The meshes, ray classes, scenes and frames shared by test_mesh_reference_cpu.py and test_mesh_reference_gpu.py, and the measured
deviations of the oracle from the float64 reference that the GPU tolerances derive from.

Tolerances. ORACLE_DEV_POS, ORACLE_DEV_OVERLAP, ORACLE_DEV_NORMAL and ORACLE_DEV_FRAME hold the largest deviation of the oracle (plain C,
float32, the same formulae as the kernels) from the float64 reference on safe rays and pixels, per mesh and ray class and per frame, as
test_mesh_reference_cpu.py measures and prints it, rounded up to two digits. That test fails if a measurement exceeds its entry, so the
tables cannot go stale. The GPU tests allow GPU_FACTOR = 4 times the entry, distances scaled by max(1, t), and for positions never more
than POSITION_TOL_CAP = 1e-4. A class whose rays come back untouched (far150: the box lies beyond the range) measures 0: equality.

Every mesh is small; each is picked for something the BVH builder or the traversal can get wrong:
  icosphere   320 triangles, closed and convex
  torus       576 triangles, closed, not convex (a ray crosses up to four surfaces)
  cube        12 triangles: every leaf box is flat on one axis, the diagonals of the faces are edges
  triangle    1 triangle: the root still has four children, three of them empty leaves with a box of (+inf, -inf)
  fan8/9/33   cones of 8, 9 and 33 triangles: a leaf holds 8, so exactly one leaf's worth, one more, and the first second-level node
  grid        72 triangles in a plane z = const: the mesh box and every node box are flat, one axis has zero centroid variance
  degenerate  the icosphere plus one triangle without area and four exact copies of another: coincident centroids, a 1 / 0 in the
              intersection
"""
import numpy as np

from conftest import pkg

import mesh_reference as ref

N_RAYS = 2000  # per class and mesh
UNSAFE_CAP = 0.02

# ------------------------------------------------------------------------------------------------------------ tolerances
GPU_FACTOR = 4.0            # the GPU compiler contracts a * b + c into one rounding and approximates rsqrt and log; the oracle's C does neither
POSITION_TOL_CAP = 1e-4     # no position may be further off than test_mesh_trace_parity allows, whatever the oracle's deviation
ORACLE_DEV_NORMAL = 1.5e-7  # largest component difference of the normal, every mesh and class (measured 1.3e-7, fan33)
ORACLE_DEV_POS = {          # (mesh, class) -> largest position difference on safe rays, relative to max(1, t)
    ("icosphere", "random"): 1.6e-7, ("icosphere", "axis"): 8.0e-7, ("icosphere", "surface_out"): 7.5e-8, ("icosphere", "surface_in"): 2.4e-7, ("icosphere", "far150"): 0.0, ("icosphere", "far50"): 2.2e-7,
    ("torus", "random"): 9.5e-8, ("torus", "axis"): 1.9e-7, ("torus", "surface_out"): 1.8e-7, ("torus", "surface_in"): 1.4e-7, ("torus", "far150"): 0.0, ("torus", "far50"): 2.4e-7,
    ("cube", "random"): 1.5e-7, ("cube", "axis"): 2.1e-7, ("cube", "surface_in"): 4.2e-8, ("cube", "far150"): 0.0, ("cube", "far50"): 1.9e-7,
    ("triangle", "random"): 2.7e-7, ("triangle", "axis"): 1.2e-6, ("triangle", "surface_out"): 7.0e-8, ("triangle", "surface_in"): 5.0e-6, ("triangle", "far150"): 0.0, ("triangle", "far50"): 2.2e-7,
    ("fan8", "random"): 2.0e-7, ("fan8", "axis"): 4.3e-7, ("fan8", "surface_out"): 7.6e-8, ("fan8", "surface_in"): 2.4e-6, ("fan8", "far150"): 0.0, ("fan8", "far50"): 2.1e-7,
    ("fan9", "random"): 2.0e-7, ("fan9", "axis"): 1.1e-6, ("fan9", "surface_out"): 7.1e-8, ("fan9", "surface_in"): 2.0e-6, ("fan9", "far150"): 0.0, ("fan9", "far50"): 2.8e-7,
    ("fan33", "random"): 3.7e-7, ("fan33", "axis"): 2.0e-6, ("fan33", "surface_out"): 7.6e-8, ("fan33", "surface_in"): 4.1e-6, ("fan33", "far150"): 0.0, ("fan33", "far50"): 2.9e-7,
    ("grid", "random"): 7.6e-8, ("grid", "axis"): 1.7e-7, ("grid", "surface_out"): 7.4e-8, ("grid", "surface_in"): 4.6e-8, ("grid", "far150"): 0.0, ("grid", "far50"): 1.6e-7,
    ("degenerate", "random"): 1.4e-7, ("degenerate", "axis"): 3.8e-7, ("degenerate", "surface_out"): 7.5e-8, ("degenerate", "surface_in"): 1.2e-7, ("degenerate", "far150"): 0.0, ("degenerate", "far50"): 2.4e-7,
}
ORACLE_DEV_OVERLAP = 2.3e-7  # the two-mesh scene
ORACLE_DEV_FRAME = {        # frame -> (depth relative to max(1, depth), rgb relative to max(1, |rgb_ref|))
    "defaults": (3.4e-7, 1.5e-6), "metallic": (3.4e-7, 5.1e-6), "rough0": (3.4e-7, 1.8e-7), "rough1_coat": (3.4e-7, 3.7e-7), "gloss_sheen_ss": (3.4e-7, 1.9e-6),
    "black": (3.4e-7, 1.5e-6), "sun_up": (4.5e-7, 4.8e-6), "sun_down": (3.4e-7, 2.8e-8), "ambient_x": (3.4e-7, 1.4e-6),
}


def position_tolerance(dev, t):
    """what a GPU result may differ by from the reference position at distance t, given the oracle's measured deviation"""
    return np.minimum(GPU_FACTOR * dev * np.maximum(1.0, t), POSITION_TOL_CAP)


# ---------------------------------------------------------------------------------------------------------------- meshes
def cube():
    v = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # outward winding
    tris = []
    for a, b, c, d in quads:
        tris += [[v[a], v[b], v[c]], [v[a], v[c], v[d]]]
    return np.asarray(tris, np.float32)


def fan(n):
    """a cone of n triangles around the apex (0, 0.5, 0), rim of radius 1 in y = 0; the winding normal points up and outwards"""
    a = np.linspace(0, 2 * np.pi, n, endpoint=False) + 0.1
    rim = np.stack([np.cos(a), np.zeros(n), np.sin(a)], 1)
    apex = np.array([0.0, 0.5, 0.0])
    return np.asarray([[apex, rim[(i + 1) % n], rim[i]] for i in range(n)], np.float32)


def grid(n=6):
    tris = []
    for i in range(n):
        for j in range(n):
            p = [np.array([i + di, j + dj, 0.25]) for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1))]
            tris += [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
    return np.asarray(tris, np.float32)


def degenerate():
    ico = pkg("meshio").icosphere(2)
    flat = ico[7].copy()
    flat[1] = flat[0]  # two equal corners: no area
    return np.concatenate([ico, flat[None], np.repeat(ico[100:101], 4, 0)]).astype(np.float32)


def meshes():
    """name -> (triangles in file space, centre, closed and convex)"""
    mi = pkg("meshio")
    return {
        "icosphere": (mi.icosphere(2), (0.0, 0.0, 0.0), True),
        "torus": (mi.torus(24, 12), (0.3, -0.2, 0.1), False),
        "cube": (cube(), (0.0, 0.0, 0.0), True),
        "triangle": (np.asarray([[[0.0, 0.0, 0.0], [1.0, 0.2, 0.1], [0.3, 0.9, 0.4]]], np.float32), (-0.4, 0.2, 0.0), False),
        "fan8": (fan(8), (0.0, 0.0, 0.0), False),
        "fan9": (fan(9), (0.0, 0.0, 0.0), False),
        "fan33": (fan(33), (0.1, 0.1, 0.1), False),
        "grid": (grid(), (0.0, 0.0, 0.0), False),
        "degenerate": (degenerate(), (0.0, 0.0, 0.0), True),
    }


MESH_NAMES = ["icosphere", "torus", "cube", "triangle", "fan8", "fan9", "fan33", "grid", "degenerate"]


def overlap_scene():
    """the torus and the icosphere, the icosphere's box covering about half of the torus's: rays that enter the torus's box first and pass
    through its hole hit nothing by the reference's rule, although the icosphere is in their way"""
    mi = pkg("meshio")
    return [(mi.torus(24, 12), (0.0, 0.0, 0.0)), (mi.icosphere(2), (0.5, 0.0, 0.0))]


def render_scene():
    """the icosphere hovering over the cube's top face, the torus standing upright next to the cube. Swapping y and z stands the torus on
    its rim (its axis along z) and, being a reflection, turns its winding normals from into the tube to out of it, so the BRDF runs on it;
    it is the one mesh here on which a lit face (NdotL > 0) can lie in shadow: the bottom of its hole under the top of its ring."""
    mi = pkg("meshio")
    return [(cube(), (0.0, 0.0, 0.0)), (mi.icosphere(2), (0.3, 1.6, 0.3)), (np.ascontiguousarray(mi.torus(24, 12)[..., [0, 2, 1]]), (1.15, 0.3, 0.0))]


def normalised(scene):
    return [ref.normalise(t, c) for t, c in scene]


# ------------------------------------------------------------------------------------------------------------------ rays
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _surface_points(T, rng, n, centroid):
    """n points on triangles with an area: their centroids, or random interior points; with the winding normals there"""
    normals, rel = ref.winding_normals(T)
    good = np.nonzero(rel > 1e-6)[0]
    k = good[rng.integers(0, good.size, n)]
    if centroid:
        w = np.full((n, 3), 1.0 / 3.0)
    else:
        w = rng.dirichlet([2.0, 2.0, 2.0], n)
    p = (np.asarray(T, np.float64)[k] * w[:, :, None]).sum(1)
    return p, normals[k]


def ray_classes(name, T, convex, seed=0):
    """class -> (origins, directions, expectation) for the normalised mesh T; expectation: "hit", "miss" or None"""
    rng = np.random.default_rng([seed, MESH_NAMES.index(name) if name in MESH_NAMES else 99])
    lo, hi = [b.astype(np.float64) for b in ref.mesh_box(T)]
    c, ext = (lo + hi) / 2, hi - lo
    n = N_RAYS
    out = {}
    out["random"] = (rng.uniform(c - 0.75 * ext - 0.05, c + 0.75 * ext + 0.05, (n, 3)), _unit(rng.normal(size=(n, 3))), None)
    # axis-aligned: two zero components (+-e_k) and one (a random direction in a coordinate plane), through a point of the slightly grown box
    d = np.zeros((n, 3))
    k = rng.integers(0, 3, n)
    d[np.arange(n), k] = rng.choice([-1.0, 1.0], n)
    half = n // 2
    ang = rng.uniform(0, 2 * np.pi, n - half)
    plane = np.stack([np.cos(ang), np.sin(ang)], 1)
    d[half:] = 0
    for i in range(half, n):
        d[i, [a for a in range(3) if a != k[i]]] = plane[i - half]
    target = rng.uniform(lo - 0.05 * ext - 0.02, hi + 0.05 * ext + 0.02, (n, 3))
    out["axis"] = (target - 1.5 * d, d, None)
    # the shadow-ray pattern: from just above the surface, outwards and inwards
    p, nrm = _surface_points(T, rng, n, centroid=True)
    h = _unit(rng.normal(size=(n, 3)))
    h = np.where(((h * nrm).sum(1) < 0)[:, None], -h, h)
    if name != "cube":  # (the cube's faces lie in the planes of its neighbours' edges: outward rays from a face graze them by construction)
        out["surface_out"] = (p + 1e-3 * nrm, h, "miss" if convex else None)
    out["surface_in"] = (p + 1e-3 * nrm, -h, None)  # (a grazing one may pass over the rim of its own facet and miss)
    # far away, aimed at a point of the surface: beyond the 100-unit range and within it
    p, _ = _surface_points(T, rng, n, centroid=False)
    away = _unit(rng.normal(size=(n, 3)))
    out["far150"] = (p + 150.0 * away, -away, "miss")
    # (from 50 units away t = -(n . (o - a)) / (n . d) is a small difference of large products; at a grazing angle float32 loses most of its
    # digits there, so these rays arrive within 37 degrees of the facet's normal, from either side of it)
    p, nrm = _surface_points(T, rng, n, centroid=False)
    tangent = _unit(np.cross(nrm, rng.normal(size=(n, 3))))
    cos = rng.uniform(0.8, 1.0, (n, 1))
    away = (cos * nrm + np.sqrt(1.0 - cos * cos) * tangent) * rng.choice([-1.0, 1.0], (n, 1))
    out["far50"] = (p + 50.0 * away, -away, "hit")
    return {k_: (o.astype(np.float32), d_.astype(np.float32), e) for k_, (o, d_, e) in out.items()}


def overlap_rays(Ts, seed=5):
    rng = np.random.default_rng(seed)
    lo = np.min([ref.mesh_box(T)[0] for T in Ts], 0).astype(np.float64)
    hi = np.max([ref.mesh_box(T)[1] for T in Ts], 0).astype(np.float64)
    c, ext = (lo + hi) / 2, hi - lo
    n = 2 * N_RAYS
    o = rng.uniform(c - 0.75 * ext, c + 0.75 * ext, (n, 3))
    target = rng.uniform(lo, hi, (n, 3))
    d = _unit(np.where(rng.uniform(size=(n, 1)) < 0.5, target - o, rng.normal(size=(n, 3))))
    return o.astype(np.float32), d.astype(np.float32)


def irradiance_points(Ts, seed=6, n=240):
    """points just above the surfaces of the overlap scene with their normals; the last 40 normals are +-z exactly"""
    rng = np.random.default_rng(seed)
    p0, n0 = _surface_points(Ts[0], rng, n // 2, centroid=False)
    p1, n1 = _surface_points(Ts[1], rng, n - n // 2, centroid=False)
    p, nrm = np.concatenate([p0, p1]), np.concatenate([n0, n1])
    nrm[-40:-20] = (0.0, 0.0, 1.0)
    nrm[-20:] = (0.0, 0.0, -1.0)
    return p.astype(np.float32), nrm.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- frames
WIDTH, HEIGHT = 64, 36


def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    """camera-to-world [right | down | forward | position], 3 x 4 float32"""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    fwd = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross(fwd, np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.stack([right, down, fwd, pos], 1).astype(np.float32)


def camera_matrix(name="defaults"):
    """Most frames look straight down from above the cube's top face, so the cube's sides (whose normals are at right angles to a vertical
    sun) stay out of sight. By the reference's rule a shadow ray only ever looks at the mesh it starts on (its own box is entered behind its
    origin, which is the smallest entry), so every shadow is a self-shadow, and under a vertical sun those lie below their caster, out of
    sight from above. That frame looks at the upright torus along its axis, a little from above and so narrowly that every ray enters the
    torus's box first: the top of the ring is lit, the bottom of the hole (which faces the sun) lies in the shadow of the top, and the
    undersides face away from the sun."""
    if name == "sun_up":
        return look_at((2.0, 1.4, 3.5), (1.65, 0.8, 0.5), up=(1.0, 0.0, 0.0))
    return look_at((0.93, 6.3, 0.57), (1.0, 0.5, 0.5))


def focal(name="defaults"):
    return (180.0, 180.0) if name == "sun_up" else (100.0, 100.0)


FRAMES = {  # name -> geometry options that differ from the defaults
    "defaults": {},
    "metallic": {"metallic": 1.0},
    "rough0": {"roughness": 0.0},
    "rough1_coat": {"roughness": 1.0, "clearcoat": 1.0, "clearcoat_gloss": 0.0},
    "gloss_sheen_ss": {"clearcoat": 1.0, "clearcoat_gloss": 1.0, "sheen": 1.0, "subsurface": 1.0},
    "black": {"basecolor": (0.0, 0.0, 0.0)},
    "sun_up": {"sun_dir": (0.0, 1.0, 0.0)},
    "sun_down": {"sun_dir": (0.0, -1.0, 0.0), "ambientcolor": (0.3, 0.2, 0.1)},  # (ambient is all that is left: it must not be black)
    "ambient_x": {"ambientcolor": (0.3, 0.2, 0.1), "up_dir": (1.0, 0.0, 0.0)},
}

_frame_cache = {}


def reference_frame(name):
    """the float64 frame, computed once per process"""
    if name not in _frame_cache:
        _frame_cache[name] = ref.render(normalised(render_scene()), camera_matrix(name), WIDTH, HEIGHT, focal(name), **FRAMES[name])
    return _frame_cache[name]


def check_frame_reaches_its_branch(name, fr):
    if name == "sun_down":
        assert fr["lit"].sum() == 0 and fr["covered"].sum() > 500 and fr["rgba"][..., :3].max() > 0.05
    else:
        assert fr["shadowed"].sum() > 30 and fr["lit"].sum() > 100, (name, fr["shadowed"].sum(), fr["lit"].sum())
    if name == "sun_up":  # faces that look at the sun and lie in shadow: the pixels whose colour the shadow ray decides
        assert fr["occluded"].sum() > 30, fr["occluded"].sum()


# ------------------------------------------------------------------------------------------- what a tracer and a renderer are held to
def compare_trace(name, cls, o, d, expect, got_pos, got_dir, meshes, report):
    """(position, direction) a tracer returned against the reference's rule: the unsafe share under the cap, hit / miss equal on every safe
    ray, the expectation of the class met, untouched rays untouched. Returns (largest position difference relative to max(1, t), largest
    normal difference) on safe rays, and the per-ray position error, reference distance and safe mask."""
    pos, direction, hit, unsafe = ref.trace(meshes, o, d)
    share = unsafe.mean()
    safe = ~unsafe
    moved = np.linalg.norm(got_pos.astype(np.float64) - o, axis=1)
    got_hit = ~np.all(got_dir == d, axis=1) | ((moved > 0) & (moved < ref.T_RANGE - 0.1))  # (a winding normal may equal the ray's direction)
    assert share <= UNSAFE_CAP, (name, cls, share)
    wrong = np.nonzero(safe & (got_hit != hit))[0]
    assert wrong.size == 0, (name, cls, "hit/miss differs on %d safe rays" % wrong.size, wrong[:5], o[wrong[:5]], d[wrong[:5]])
    if expect == "hit":
        assert hit[safe].all(), (name, cls, "the reference misses", (~hit[safe]).sum())
    if expect == "miss":
        assert not hit[safe].any(), (name, cls, "the reference hits", hit[safe].sum())
    # a miss keeps its direction; a ray that enters a box and hits nothing ends at o + 100 d (checked with the positions), one that enters no
    # box is untouched
    s_miss = safe & ~hit
    assert np.array_equal(got_dir[s_miss], d[s_miss]), (name, cls, "a missed ray's direction changed")
    t_ref = np.linalg.norm(pos - o.astype(np.float64), axis=1)
    err = np.abs(got_pos.astype(np.float64) - pos).max(1)
    untouched = s_miss & np.all(pos == o, axis=1)
    assert np.array_equal(got_pos[untouched], o[untouched])
    s_hit = safe & hit
    dn = np.abs(got_dir[s_hit].astype(np.float64) - direction[s_hit]).max() if s_hit.any() else 0.0  # (the winding normal, not its negative)
    dt = (err / np.maximum(1.0, t_ref))[safe].max() if safe.any() else 0.0
    report.append("%-10s %-11s rays %5d  hits %5d  unsafe %5.2f %%  dpos/max(1,t) %.2e  dnormal %.2e" % (name, cls, o.shape[0], hit.sum(), 100 * share, dt, dn))
    return dt, dn, err, t_ref, safe


def compare_frame(name, fr, rgba, depth):
    """coverage equal on every safe pixel; returns the largest depth and (relative) colour deviation on them"""
    safe = ~fr["unsafe"]
    assert np.array_equal(rgba[..., 3][safe], fr["rgba"][..., 3][safe]), (name, "coverage differs on safe pixels")
    both = safe & fr["covered"]
    assert np.all(depth[safe & ~fr["covered"]] == ref.MAX_DEPTH) and np.all(rgba[safe & ~fr["covered"]] == 0)
    dd = np.abs(depth[both] - fr["depth"][both]) / np.maximum(1.0, fr["depth"][both])
    want = fr["rgba"][..., :3][both]
    dc = np.abs(rgba[..., :3][both] - want) / np.maximum(1.0, np.abs(want))
    return dd.max(), dc.max()


def bvh_depth(nodes):
    """depth of the deepest leaf, the root being 0"""
    def visit(i, d):
        nd = nodes[i]
        if nd["left_idx"] < 0:
            return d
        return max(visit(c, d + 1) for c in range(nd["left_idx"], nd["left_idx"] + 4))
    return visit(0, 0)
