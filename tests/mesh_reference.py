"""A plain float64 reference of the mesh side of Geometry mode: brute-force nearest triangle, the reference's mesh selection, the
shadow ray and the Disney-style shade. numpy only; nothing here comes from oracle/ or from the package, and nothing is a BVH.

Written from the definitions: Moeller-Trumbore ("Fast, minimum storage ray/triangle intersection", 1997) for the triangle, the slab test
for boxes, Burley's "Physically based shading at Disney" (2012) for the BRDF. What the renderer does differently from Burley's BRDF is
listed at `shade`.

Every function also reports which rays (pixels) are *unsafe*: those where a float32 evaluation may legitimately decide differently from
this one (a hit within 1e-4 barycentric units of a triangle edge, two surfaces within 1e-5 of each other, a hit within 1e-3 of the end
of the range, ...). The tests demand equality of hit / miss on every other ray and cap the share of unsafe ones.

The clearcoat lobe GTR1(NdotH, a) has a branch a >= 1 (a constant 1 / pi). The renderer calls it with a = mix(0.1, 0.001, gloss) < 1
for every gloss in [0, 1], so the branch cannot be reached through the API; `gtr1` keeps it for completeness and no test aims at it.
"""
import numpy as np

T_RANGE = 100.0        # the traversal's range: no hit at or beyond it
EDGE_EPS = 1e-4        # barycentric distance from a triangle edge below which a float32 evaluation may differ
TIE_EPS = 1e-5         # two hits (or two box entries) closer than this are a tie
RANGE_EPS = 1e-3       # distance from the end of the range below which a hit is ambiguous
SHADOW_OFFSET = 1e-3   # the shadow ray starts this far above the surface
MAX_DEPTH = 16384.0    # depth of a pixel without a mesh


def normalise(vertices, center):
    """The loader's normalisation: the mesh box, inflated by 0.5 % of its diagonal, is scaled (uniformly, by its longest side) and moved so
    that its centre sits at `center` + 0.5. float32 throughout, in the loader's order of operations; returns float32 (n, 3, 3)."""
    f = np.float32
    v = np.asarray(vertices, f).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    d0 = hi - lo
    amount = f(np.sqrt(f(f(d0[0] * d0[0] + d0[1] * d0[1]) + d0[2] * d0[2]))) * f(0.005)
    lo, hi = lo - amount, hi + amount
    diag = hi - lo
    scale = diag.max()
    q = ((v - lo) - diag * f(0.5)) / scale
    q = (q + f(0.5)) + np.asarray(center, f)
    return q.astype(f).reshape(-1, 3, 3)


def winding_normals(T):
    """(b - a) x (c - a) normalised (zero for a triangle without area), and twice the area relative to the longest edge squared"""
    T = np.asarray(T, np.float64)
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    n = np.cross(e1, e2)
    ln = np.linalg.norm(n, axis=1)
    longest = np.maximum.reduce([(e1 * e1).sum(1), (e2 * e2).sum(1), ((e2 - e1) ** 2).sum(1)])
    rel = np.where(longest > 0, ln / np.where(longest > 0, longest, 1), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where(ln[:, None] > 0, n / ln[:, None], 0.0)
    return unit, rel


def nearest_hit(T, o, d, t_range=T_RANGE, chunk=2048):
    """Moeller-Trumbore of every ray against every triangle. Returns (t, index, normal, unsafe): the nearest t in [0, t_range) (inf: none),
    its triangle (-1), that triangle's winding normal (zeros) and the unsafe flag described in the module docstring."""
    T = np.asarray(T, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    a, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    normals, rel_area = winding_normals(T)
    flat = rel_area < 1e-9  # a triangle without area is never hit
    n_rays = o.shape[0]
    t_out = np.full(n_rays, np.inf)
    i_out = np.full(n_rays, -1, np.int64)
    unsafe = np.zeros(n_rays, bool)
    for r0 in range(0, n_rays, chunk):
        oo, dd = o[r0:r0 + chunk, None, :], d[r0:r0 + chunk, None, :]
        p = np.cross(dd, e2[None])
        det = (e1[None] * p).sum(-1)
        ok = (det != 0) & ~flat[None]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
            s = oo - a[None]
            u = (s * p).sum(-1) * inv
            q = np.cross(s, e1[None])
            v = (dd * q).sum(-1) * inv
            t = (e2[None] * q).sum(-1) * inv
        edge = np.minimum(np.minimum(u, v), 1.0 - u - v)
        inside = ok & (edge >= 0)
        hit = inside & (t >= 0) & (t < t_range)
        th = np.where(hit, t, np.inf)
        idx = th.argmin(1)
        rows = np.arange(th.shape[0])
        tn = th[rows, idx]
        found = np.isfinite(tn)
        # 1. a triangle crossed within the range (a little beyond it, too) close to one of its edges, from either side
        near_edge = ok & (np.abs(edge) < EDGE_EPS) & (t >= 0) & (t < t_range + RANGE_EPS)
        bad = near_edge.any(1)
        # 2. the two nearest hits closer than TIE_EPS with different normals
        if th.shape[1] > 1:
            th2 = th.copy()
            th2[rows, idx] = np.inf
            # (exact duplicates of the nearest triangle are no tie: skip every triangle with the same normal)
            same = (np.abs(normals[None] - normals[idx][:, None]).max(-1) == 0)
            th2[same] = np.inf
            bad |= found & (th2.min(1) - np.where(found, tn, 0.0) < TIE_EPS)
        # 3. a crossing within RANGE_EPS of the end of the range
        bad |= (inside & (np.abs(t - t_range) < RANGE_EPS)).any(1)
        # 4. the nearest triangle has (next to) no area
        bad |= found & (rel_area[idx] < 1e-6)
        t_out[r0:r0 + chunk] = tn
        i_out[r0:r0 + chunk] = np.where(found, idx, -1)
        unsafe[r0:r0 + chunk] = bad
    n_out = np.where(i_out[:, None] >= 0, normals[np.maximum(i_out, 0)], 0.0)
    return t_out, i_out, n_out, unsafe


def box_entry(lo, hi, o, d):
    """Slab test of the line o + t d against [lo, hi]: (entry, exit) with entry = the largest near-plane distance, exit = the smallest
    far-plane distance; entry = inf when they do not overlap. As in the renderer's mesh selection the sign is not looked at: a box behind the
    origin is entered at a negative distance."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    near, far = np.fmin(t0, t1), np.fmax(t0, t1)
    # a zero component: the slab is all of the line (origin strictly inside it) or none of it
    zero = d == 0
    inside = (o > lo) & (o < hi)
    near = np.where(zero, np.where(inside, -np.inf, np.inf), near)
    far = np.where(zero, np.where(inside, np.inf, -np.inf), far)
    entry, exit_ = near.max(1), far.min(1)
    return np.where(entry <= exit_, entry, np.inf), exit_, entry


def mesh_box(T):
    p = np.asarray(T, np.float32).reshape(-1, 3)
    return p.min(0), p.max(0)


def reference_rule_hit(meshes, o, d):
    """The renderer's (the reference's) mesh selection: of the meshes whose box the line enters at a finite distance below 100, only the one
    entered first is traced. Returns (t, mesh, index, normal, unsafe, entered): mesh = -1 when no box qualifies (the ray is left untouched);
    t = inf when the chosen mesh has no hit."""
    n = np.asarray(o).shape[0]
    entries, graze = [], np.zeros(n, bool)
    for T in meshes:
        lo, hi = mesh_box(T)
        e, ex, raw = box_entry(lo, hi, o, d)
        graze |= np.abs(raw - T_RANGE) < RANGE_EPS   # the box is entered at the end of the range
        if len(meshes) > 1:                          # which of several boxes comes first: a line that touches one at an edge or a corner
            graze |= np.abs(ex - raw) < TIE_EPS      # (with one mesh a triangle behind such a spot is met within EDGE_EPS of its own edge)
        entries.append(np.where(np.isfinite(e) & (e < T_RANGE), e, np.inf))
    E = np.stack(entries, 1)
    mesh = E.argmin(1)
    best = E[np.arange(n), mesh]
    entered = best < np.inf
    unsafe = graze.copy()
    if E.shape[1] > 1:
        E2 = E.copy()
        E2[np.arange(n), mesh] = np.inf
        with np.errstate(invalid="ignore"):
            unsafe |= entered & (np.abs(E2.min(1) - best) < TIE_EPS)
    t = np.full(n, np.inf)
    idx = np.full(n, -1, np.int64)
    nrm = np.zeros((n, 3))
    for m, T in enumerate(meshes):
        sel = entered & (mesh == m)
        if sel.any():
            tt, ii, nn, uu = nearest_hit(T, np.asarray(o)[sel], np.asarray(d)[sel])
            t[sel], idx[sel], nrm[sel] = tt, ii, nn
            unsafe[sel] |= uu
    return t, np.where(entered, mesh, -1), idx, nrm, unsafe, entered


def trace(meshes, o, d):
    """What tracing a ray leaves behind, by the rule above: (position, direction, hit, unsafe). A hit: o + t d and the winding normal. A mesh
    chosen but not hit: o + 100 d, direction unchanged. No mesh chosen: untouched."""
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    t, mesh, idx, nrm, unsafe, entered = reference_rule_hit(meshes, o64, d64)
    hit = idx >= 0
    step = np.where(hit, t, np.where(entered, T_RANGE, 0.0))
    with np.errstate(invalid="ignore"):
        pos = np.where(step[:, None] != 0, o64 + step[:, None] * d64, o64)
    return pos, np.where(hit[:, None], nrm, d64), hit, unsafe


def global_nearest(meshes, o, d):
    """the nearest hit over all the triangles of all the meshes: (t, unsafe)"""
    T = np.concatenate([np.asarray(m, np.float32) for m in meshes])
    t, _, _, unsafe = nearest_hit(T, o, d)
    return t, unsafe


# --------------------------------------------------------------------------------------------------------------- shading
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def schlick(u):
    """Schlick's Fresnel weight (1 - u)^5, the argument clamped to [0, 1]"""
    return np.clip(1.0 - u, 0.0, 1.0) ** 5


def gtr1(ndh, a):
    """Burley's GTR with gamma = 1 (the clearcoat lobe); a >= 1 is its limit 1 / pi (unreachable, see the module docstring)"""
    if a >= 1:
        return np.full_like(ndh, 1.0 / np.pi)
    a2 = a * a
    return (a2 - 1.0) / (np.pi * np.log(a2) * (1.0 + (a2 - 1.0) * ndh * ndh))


def gtr2(ndh, a):
    """Burley's GTR with gamma = 2 (GGX / Trowbridge-Reitz), the specular lobe"""
    a2 = a * a
    return a2 / (np.pi * (1.0 + (a2 - 1.0) * ndh * ndh) ** 2)


def smith_ggx(ndv, alpha):
    a, b = alpha * alpha, ndv * ndv
    return 1.0 / (ndv + np.sqrt(a + b - a * b))


def _mix(a, b, t):
    return a + (b - a) * t


def shade(base, ambient, light, L, V, N, metallic=0.0, subsurface=0.0, specular=1.0, roughness=0.5, sheen=0.0, clearcoat=0.0, clearcoat_gloss=0.0):
    """Burley's Disney BRDF times the light and NdotL, plus an ambient term. base (3,), ambient / light / V / N (n, 3), L (3,). Where the
    renderer departs from Burley's published BRDF:
      - `base` arrives squared (the caller squares the base colour, a cheap gamma);
      - specular tint and sheen tint are 0, so the tint colour base / luminance never shows;
      - an ambient term mix(0.2, FV, metallic) * ambient * base is added, and it is all that is returned when NdotL < 0 or NdotV < 0;
      - the clearcoat lobe is GTR1 at mix(0.1, 0.001, gloss), its masking term Smith GGX at 0.25;
      - the specular roughness is alpha = max(0.001, roughness^2)."""
    base = np.asarray(base, np.float64)
    ndl, ndv = (N * L).sum(-1), (N * V).sum(-1)
    H = _unit(L + V)
    ndh, ldh = (N * H).sum(-1), (L * H).sum(-1)
    FL, FV, FH = schlick(ndl), schlick(ndv), schlick(ldh)
    amb = ambient * _mix(0.2, FV, metallic)[:, None] * base
    back = (ndl < 0) | (ndv < 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # diffuse: Burley's retro-reflective diffuse and the Hanrahan-Krueger-like subsurface approximation
        fd90 = 0.5 + 2.0 * ldh * ldh * roughness
        fd = _mix(1.0, fd90, FL) * _mix(1.0, fd90, FV)
        fss90 = ldh * ldh * roughness
        fss = _mix(1.0, fss90, FL) * _mix(1.0, fss90, FV)
        ss = 1.25 * (fss * (1.0 / (ndl + ndv) - 0.5) + 0.5)
        diffuse = base * ((1.0 / np.pi) * _mix(fd, ss, subsurface))[:, None] + (FH * sheen)[:, None] * np.ones(3)
        # specular: GGX, Schlick Fresnel from the specular colour, Smith masking
        alpha = max(0.001, roughness * roughness)
        cspec0 = _mix(np.ones(3) * specular * 0.08, base, metallic)
        Fs = _mix(cspec0, np.ones(3), FH[:, None])
        spec = Fs * (gtr2(ndh, alpha) * smith_ggx(ndl, alpha) * smith_ggx(ndv, alpha))[:, None]
        # clearcoat: ior 1.5 -> F0 = 0.04
        coat = 0.25 * clearcoat * smith_ggx(ndl, 0.25) * smith_ggx(ndv, 0.25) * _mix(0.04, 1.0, FH) * gtr1(ndh, _mix(0.1, 0.001, clearcoat_gloss))
        brdf = diffuse * (1.0 - metallic) + spec + coat[:, None]
        lit = brdf * light * ndl[:, None] + amb
    return np.where(back[:, None], amb, lit), ndl, ndv


def _inside(lo, hi, p):
    return np.all((p >= lo) & (p <= hi), axis=-1)


def scene_box(meshes):
    """the box of all the meshes, inflated by 4 (float32, as the loader keeps it)"""
    los, his = zip(*[mesh_box(T) for T in meshes])
    return np.min(los, 0) - np.float32(4.0), np.max(his, 0) + np.float32(4.0)


SUN_COLOUR = np.array([255.0, 225.0, 195.0]) / 255.0 * 4.0
SKY_COLOUR = np.array([195.0, 215.0, 255.0]) / 255.0 * 4.0


def render(meshes, matrix_3x4, width, height, focal, sun_dir=(1.0, 1.0, 1.0), up_dir=(0.0, 1.0, 0.0), basecolor=(0.8, 0.8, 0.8), ambientcolor=(0.0, 0.0, 0.0),
           pixel_offset=(0.5, 0.5), **brdf):
    """One frame of the mesh pass through a pinhole camera (camera-to-world [R | t], pixel centres, principal point in the middle):
    primary ray from the entry into the scene box, nearest hit by `trace`, shadow ray from the hit moved SHADOW_OFFSET along the normal
    facing the viewer, towards the sun; in shadow when the shadow ray ends inside the scene box. Returns a dict: rgba (h, w, 4), depth
    (h, w), and per pixel unsafe, covered, shadowed, lit (NdotL >= 0 and NdotV >= 0 and not shadowed), occluded (NdotL >= 0 and NdotV >= 0 and
    shadowed: the pixels whose colour the shadow ray decides)."""
    meshes = [np.asarray(T, np.float32) for T in meshes]
    M = np.asarray(matrix_3x4, np.float32).astype(np.float64)
    lo, hi = [b.astype(np.float64) for b in scene_box(meshes)]
    ys, xs = np.mgrid[0:height, 0:width]
    u = (xs.reshape(-1) + pixel_offset[0]) / width
    v = (ys.reshape(-1) + pixel_offset[1]) / height
    local = np.stack([(u - 0.5) * width / focal[0], (v - 0.5) * height / focal[1], np.ones_like(u)], 1)
    d = _unit(local @ M[:, :3].T)
    origin = np.broadcast_to(M[:, 3], d.shape)
    entry, _, _ = box_entry(lo, hi, origin, d)
    start = origin + (np.maximum(np.where(np.isfinite(entry), entry, 0.0), 0.0) + 1e-6)[:, None] * d
    pos, nrm, hit, unsafe = trace(meshes, start, d)
    covered = _inside(lo, hi, pos) & np.isfinite(entry)  # (a primary ray that misses the scene box goes nowhere)
    # shadow ray
    facing = np.where(((nrm * d).sum(1) < 0)[:, None], nrm, -nrm)
    sun = _unit(np.asarray(sun_dir, np.float64))
    spos = pos + SHADOW_OFFSET * _unit(facing)
    s_entry, _, _ = box_entry(lo, hi, spos, np.broadcast_to(sun, spos.shape))
    s_entry = np.where(np.isfinite(s_entry), s_entry, 3.402823466e+38)
    spos = spos + np.maximum(s_entry + 1e-6, 0.0)[:, None] * sun
    alive = _inside(lo, hi, spos)
    sdir = np.where(alive[:, None], sun, d)  # a shadow ray that starts outside the scene box keeps the primary direction
    send, _, _, s_unsafe = trace(meshes, spos, sdir)
    shadowed = _inside(lo, hi, send)
    N = _unit(np.where(hit[:, None], nrm, d))
    up = _unit(np.asarray(up_dir, np.float64))
    sky = SKY_COLOUR * (-(N * up).sum(1) * 0.5 + 0.5)[:, None]
    light = SUN_COLOUR * np.where(shadowed, 0.0, 1.0)[:, None]
    base = np.asarray(basecolor, np.float32).astype(np.float64)
    amb = np.asarray(ambientcolor, np.float32).astype(np.float64) * sky
    f32 = {k: float(np.float32(x)) for k, x in brdf.items()}
    rgb, ndl, ndv = shade(base * base, amb, light, sun, -d, N, **f32)
    rgba = np.zeros((width * height, 4))
    rgba[covered, :3], rgba[covered, 3] = rgb[covered], 1.0
    depth = np.where(covered, ((pos - M[:, 3]) * M[:, 2]).sum(1), MAX_DEPTH)
    unsafe = unsafe | (covered & (s_unsafe | (np.abs(ndl) < EDGE_EPS) | (np.abs(ndv) < EDGE_EPS)))
    shape = (height, width)
    return {"rgba": rgba.reshape(height, width, 4), "depth": depth.reshape(shape), "unsafe": unsafe.reshape(shape), "covered": covered.reshape(shape),
            "shadowed": (covered & shadowed).reshape(shape), "lit": (covered & ~shadowed & (ndl >= 0) & (ndv >= 0)).reshape(shape),
            "occluded": (covered & shadowed & (ndl >= 0) & (ndv >= 0)).reshape(shape)}
