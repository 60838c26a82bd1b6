"""What test_mesh_reflection_meshes_cpu.py and test_mesh_reflection_meshes_gpu.py share (include/ngp_hip.h, "mesh reflection, the meshes in
it"): the three cases and mesh_reflection_cases.render_with_reflection restated with the shade of the mirror ray's mesh hit behind the NeRF.

A pixel owns a hit when it owns a mirror ray whose t_hit is finite. With r^ = unit(r), in float64:
    p2 = rq + r^ t_hit,   n2 = the hit triangle's winding normal (mesh_reference.nearest_hit over all the triangles),
    ff2 = n2 turned against r^,   q2 = p2 + SHADOW_OFFSET unit(ff2),   shadow2 = 0 where mesh_reference.global_nearest finds a triangle from q2
    along the sun, else 1,   C2 = mesh_reference.shade(base^2, ambient(p2, n2), SUN_COLOUR shadow2, sun, -r^, n2)
    L = rgb_r + max(1 - alpha_r, 0) C2,   added = strength F L where alpha_r > 0 or the ray owns a hit
(rgb_r, alpha_r) and, for the colour tests, C2 are what the caller hands in. A hit is unsafe where the mirror ray's t_unsafe is set, where the
hit's shadow ray is unsafe, or where |N.L| or |N.V| at the hit is below mesh_reference.EDGE_EPS. p2_32 and q2_32 are p2 and q2 as a float32
program forms them from q32, r32 and t_hit32 on the reference's own triangle; they exist only to price float32.

Case A: mesh_reflection_cases' floor, no ray is cut. Case B: its plate, with its sun: rays are cut on both meshes and most sun-facing hits lie
in a mesh's shadow. Case C: the floor and a wall behind the object (mesh_cases.cube scaled to (0.04, 1, 1) at centre (0.95, 0.4, 0): after the
loader's normalisation at x = 1.43 .. 1.47, y = 0.41 .. 1.39) under the sun (-1, 1, -0.3), which lights the wall's near face: the floor mirrors
the wall, in the open and behind the captured object."""
import numpy as np

import irradiance_bounce_reference as br
import mesh_cases as mc
import mesh_reference as ref
import mesh_reflection_cases as rc
import mesh_sun_nerf_shadow_cases as sc

WIDTH, HEIGHT, FOCAL, CAMERA = rc.WIDTH, rc.HEIGHT, rc.FOCAL, rc.CAMERA
WALL_SCALE, WALL_CENTER = (0.04, 1.0, 1.0), (0.95, 0.4, 0.0)
SUN = {"A": rc.SUN, "B": rc.SUN, "C": (-1.0, 1.0, -0.3)}
MIN_LIT_OPEN, MIN_LIT_HIDDEN, MIN_SHADOWED = 100, 20, 100  # case C: lit hits at alpha_r = 0 and at alpha_r > 0.9; case B: sun-facing hits in a mesh's shadow
_cache = {}


def scene(case="A"):
    """[(triangles, centre)]: A the floor, B the floor and the plate, C the floor and the wall"""
    if case != "C":
        return rc.scene(case)
    wall = (mc.cube().astype(np.float64) * np.array(WALL_SCALE)).astype(np.float32)
    return br.floor_scene() + [(wall, WALL_CENTER)]


def meshes(case="A"):
    return br.normalised(scene(case))


def _unit32_twice(n, against):
    """the unit normal turned against `against` and normalised once more, as the pass forms it, in float32"""
    f = np.float32
    nn = (n / np.sqrt(rc._dot32(n, n))[:, None]).astype(f)
    nff = np.where((rc._dot32(nn, against) < 0)[:, None], nn, -nn).astype(f)
    return (nff / np.sqrt(rc._dot32(nff, nff))[:, None]).astype(f)


def _hit32(T, idx, rq32, r32, t_hit32):
    """(p2_32, q2_32) of cut rays as a float32 program forms them on the reference's own triangles T[idx]: r^ by one square root and three
    quotients, p2 = q + fl(r^ t_hit), n2 from the float32 cross product, q2 = p2 + fl(n^ 1e-3)"""
    f = np.float32
    rh = rc.unit32(r32)
    p2 = (rq32 + (rh * t_hit32[:, None]).astype(f)).astype(f)
    _, n = br._tri_t32(T[idx].astype(f), rq32, rh)
    nh = _unit32_twice(n, rh)
    return p2, (p2 + (nh * f(ref.SHADOW_OFFSET)).astype(f)).astype(f)


def render_with_reflection_meshes(meshes, matrix_3x4, width, height, focal, ambient_fn, factor=None, reflected=None, hit_colour=None, strength=1.0, sun_dir=rc.SUN,
                                  basecolor=(0.8, 0.8, 0.8), pixel_offset=(0.5, 0.5), **brdf):
    """mesh_reflection_cases.render_with_reflection with the mesh hit's colour behind the NeRF along the mirror ray. hit_colour: None (the hits
    add nothing: that function's arrays, every one), "shade" (C2 of the reference), or (h, w, 3), a C2 handed in, looked at on owners of a hit
    only. Adds to that function's dict, per pixel: cut (h, w), p2, n2, q2 (h, w, 3; zeros without a hit), shadow2 (1 open, 0 blocked or no hit),
    C2 (the reference's), faces_sun (N.L >= 0 and N.V >= 0 at the hit), hit_unsafe, ndv2, p2_32, q2_32, L (h, w, 3) and L_used (the L of the
    colour handed in), and p2_dev / q2_dev, the largest |p2_32 - p2| / max(1, t_hit) (|q2_32 - q2| alike) on safe hits. rgba, added and added32
    are those of the hit colour in use."""
    fr = rc.render_with_reflection(meshes, matrix_3x4, width, height, focal, ambient_fn, factor, reflected, strength, sun_dir, basecolor, pixel_offset, **brdf)
    if hit_colour is None:
        return fr
    out = dict(fr)
    meshes = [np.asarray(T, np.float32) for T in meshes]
    n_px = width * height
    owns, t_hit = fr["owns"].reshape(-1), fr["t_hit"].reshape(-1)
    cut = owns & np.isfinite(t_hit)
    rq, r = fr["rq"].reshape(-1, 3), fr["r"].reshape(-1, 3)
    p2, n2, q2, C2 = np.zeros((n_px, 3)), np.zeros((n_px, 3)), np.zeros((n_px, 3)), np.zeros((n_px, 3))
    shadow2, faces, unsafe, ndv2 = np.zeros(n_px), np.zeros(n_px, bool), np.zeros(n_px, bool), np.zeros(n_px)
    p2_32, q2_32 = np.zeros((n_px, 3), np.float32), np.zeros((n_px, 3), np.float32)
    sun = ref._unit(np.asarray(sun_dir, np.float64))
    base = np.asarray(basecolor, np.float32).astype(np.float64)
    if cut.any():
        T = np.concatenate(meshes)
        rh = ref._unit(r[cut])
        t, idx, nrm, t_unsafe = ref.nearest_hit(T, rq[cut], rh)
        assert np.array_equal(t, t_hit[cut])
        p2[cut] = rq[cut] + rh * t[:, None]
        n2[cut] = nrm
        ff = np.where(((nrm * rh).sum(1) < 0)[:, None], nrm, -nrm)
        q2[cut] = p2[cut] + ref.SHADOW_OFFSET * ref._unit(ff)
        t_s, s_unsafe = ref.global_nearest(meshes, q2[cut], np.broadcast_to(sun, rh.shape))
        shadow2[cut] = np.where(np.isfinite(t_s), 0.0, 1.0)
        f32 = {k: float(np.float32(x)) for k, x in brdf.items()}
        amb = np.asarray(ambient_fn(p2[cut], nrm), np.float64)
        C2[cut], ndl, ndv = ref.shade(base * base, amb, ref.SUN_COLOUR * shadow2[cut][:, None], sun, -rh, nrm, **f32)
        faces[cut] = (ndl >= 0) & (ndv >= 0)
        ndv2[cut] = ndv
        unsafe[cut] = t_unsafe | fr["t_unsafe"].reshape(-1)[cut] | s_unsafe | (np.abs(ndl) < ref.EDGE_EPS) | (np.abs(ndv) < ref.EDGE_EPS)
        p2_32[cut], q2_32[cut] = _hit32(T, idx, fr["rq32"].reshape(-1, 3)[cut], fr["r32"].reshape(-1, 3)[cut], fr["t_hit32"].reshape(-1)[cut])
    refl = np.zeros((n_px, 4), np.float32) if reflected is None else np.asarray(reflected, np.float32).reshape(-1, 4)
    refl = np.where(owns[:, None], refl, np.float32(0))
    used = C2 if isinstance(hit_colour, str) else np.where(cut[:, None], np.asarray(hit_colour, np.float32).reshape(-1, 3).astype(np.float64), 0.0)
    through = np.maximum(1.0 - refl[:, 3].astype(np.float64), 0.0)
    L = refl[:, :3].astype(np.float64) + through[:, None] * C2
    L_used = refl[:, :3].astype(np.float64) + through[:, None] * used
    adds = owns & ((refl[:, 3] > 0) | cut)
    F = fr["F"].reshape(-1, 3)
    added = np.where(adds[:, None], F * L_used * float(np.float32(strength)), 0.0)
    # the float32 form of the term, in the pass's order, from the float32 values handed in
    f = np.float32
    shading = dict(basecolor=basecolor, **{k: x for k, x in brdf.items() if k in ("metallic", "specular")})
    F32 = rc.fresnel(fr["c32"].reshape(-1), dtype=f, **shading)
    through32 = np.maximum((f(1) - refl[:, 3]).astype(f), f(0))
    L32 = np.where(cut[:, None], (refl[:, :3] + (used.astype(f) * through32[:, None]).astype(f)).astype(f), refl[:, :3])
    added32 = np.where(adds[:, None], ((F32 * L32).astype(f) * f(strength)).astype(f), f(0))
    covered = fr["covered"].reshape(-1)
    rgba = fr["rgba"].reshape(-1, 4).copy()
    rgba[covered, :3] = (rgba[:, :3] - fr["added"].reshape(-1, 3) + added)[covered]
    m = cut & ~unsafe
    scale = np.maximum(1.0, t_hit[m])[:, None] if m.any() else 1.0
    shape = (height, width)
    out.update(rgba=rgba.reshape(height, width, 4), added=added.reshape(height, width, 3), added32=added32.reshape(height, width, 3), cut=cut.reshape(shape),
               p2=p2.reshape(height, width, 3), n2=n2.reshape(height, width, 3), q2=q2.reshape(height, width, 3), shadow2=shadow2.reshape(shape),
               C2=C2.reshape(height, width, 3), faces_sun=faces.reshape(shape), hit_unsafe=unsafe.reshape(shape), ndv2=ndv2.reshape(shape),
               p2_32=p2_32.reshape(height, width, 3), q2_32=q2_32.reshape(height, width, 3), L=L.reshape(height, width, 3), L_used=L_used.reshape(height, width, 3),
               p2_dev=float((np.abs(p2_32.astype(np.float64) - p2)[m] / scale).max()) if m.any() else 0.0,
               q2_dev=float((np.abs(q2_32.astype(np.float64) - q2)[m] / scale).max()) if m.any() else 0.0)
    return out


def frame(case="A", reflected=None, hit_colour="shade", strength=1.0, ambient_fn=sc.no_ambient, **opts):
    """the float64 frame of a case under the case's sun; the one with no radiance handed in is computed once per process and case"""
    plain = reflected is None and isinstance(hit_colour, str) and strength == 1.0 and ambient_fn is sc.no_ambient and not opts
    if plain and case in _cache:
        return _cache[case]
    fr = render_with_reflection_meshes(meshes(case), CAMERA, WIDTH, HEIGHT, FOCAL, ambient_fn, None, reflected, hit_colour, strength, **dict(dict(sun_dir=SUN[case]), **opts))
    if plain:
        _cache[case] = fr
    return fr


def frame_bound(rgb_ref):
    return rc.frame_bound(rgb_ref)
