"""What test_mesh_materials_cpu.py and test_mesh_materials_gpu.py share (include/ngp_hip.h, "mesh materials"): the scene, the three materials
and the float64 frame in which every mesh is shaded with its own material, restated on top of mesh_reflection_meshes_cases without editing it.

The scene is mesh_reflection_meshes_cases' case B, the floor (mesh 0) and the plate (mesh 1), with that module's camera, sun and 64 x 48 frame.
The floor owns FLOOR, the plate owns PLATE, and the context holds CONTEXT: a covered pixel whose primary ray found no triangle is the context's.

The per-mesh frame. owner (h, w): the mesh of the primary hit by mesh_reference.reference_rule_hit on the frame's own primary rays, -1 without a
triangle. One render_with_reflection_meshes frame is rendered per material. A cut mirror ray's hit mesh comes from mesh_reference.nearest_hit
over the concatenated triangles; the C2 of a hit is the C2 of the frame of the hit mesh's material (C2 depends on the hit's material alone).
A second round renders each material's frame with hit_colour = that mixed C2, so its added term is F of that material times the mixed L; a
pixel then takes the frame of its owner's material."""
import numpy as np

import mesh_reference as ref
import mesh_reflection_meshes_cases as hc
import mesh_sun_nerf_shadow_cases as sc

CASE = "B"
WIDTH, HEIGHT, FOCAL, CAMERA, SUN = hc.WIDTH, hc.HEIGHT, hc.FOCAL, hc.CAMERA, hc.SUN[CASE]
AMBIENT = 0.3
CONTEXT = dict(basecolor=(0.8, 0.8, 0.8))
FLOOR = dict(basecolor=(0.6, 0.6, 0.65), metallic=0.9, roughness=0.2)
PLATE = dict(basecolor=(0.9, 0.15, 0.1), metallic=0.0, roughness=0.8, specular=0.5)
MATERIALS = {-1: CONTEXT, 0: FLOOR, 1: PLATE}  # by owner mesh
MIN_CLASS = 100         # pixels of each class the case must have
UNSAFE_CAP = 0.03       # the share of pixels and of hits the float64 tracer may flag
MIN_SEPARATION = 100    # a material's pixels differ from the context-material frame by at least this many frame_bound
_cache = {}


def scene():
    s = hc.scene(CASE)
    assert len(s) == 2
    return s


def meshes():
    return hc.meshes(CASE)


def constant_ambient(pos, N):
    return np.full(np.asarray(pos).shape, AMBIENT)


def owner(width=WIDTH, height=HEIGHT, pixel_offset=(0.5, 0.5)):
    """(owner (h, w) int64: the mesh of the primary hit, -1 without a triangle; unsafe (h, w): reference_rule_hit's flag). The primary rays are
    mesh_reflection_cases.render_with_reflection's, statement for statement."""
    key = ("owner", width, height, tuple(pixel_offset))
    if key not in _cache:
        T = [np.asarray(t, np.float32) for t in meshes()]
        M = np.asarray(CAMERA, np.float32).astype(np.float64)
        lo, hi = [b.astype(np.float64) for b in ref.scene_box(T)]
        ys, xs = np.mgrid[0:height, 0:width]
        u = (xs.reshape(-1) + pixel_offset[0]) / width
        v = (ys.reshape(-1) + pixel_offset[1]) / height
        local = np.stack([(u - 0.5) * width / FOCAL[0], (v - 0.5) * height / FOCAL[1], np.ones_like(u)], 1)
        d = ref._unit(local @ M[:, :3].T)
        origin = np.broadcast_to(M[:, 3], d.shape)
        entry, _, _ = ref.box_entry(lo, hi, origin, d)
        start = origin + (np.maximum(np.where(np.isfinite(entry), entry, 0.0), 0.0) + 1e-6)[:, None] * d
        t, mesh, _, _, unsafe, _ = ref.reference_rule_hit(T, start, d)
        own = np.where(np.isfinite(t) & (mesh >= 0), mesh, -1).astype(np.int64)
        _cache[key] = (own.reshape(height, width), np.asarray(unsafe, bool).reshape(height, width))
    return _cache[key]


def hit_mesh(fr):
    """(h, w) int64: the mesh each cut mirror ray of a render_with_reflection_meshes frame hits, -1 where the ray is not cut"""
    T = [np.asarray(t, np.float32) for t in meshes()]
    cut = fr["cut"].reshape(-1)
    out = np.full(cut.size, -1, np.int64)
    if cut.any():
        rq, r = fr["rq"].reshape(-1, 3)[cut], fr["r"].reshape(-1, 3)[cut]
        _, idx, _, _ = ref.nearest_hit(np.concatenate(T), rq, ref._unit(r))
        out[cut] = np.searchsorted(np.cumsum([len(t) for t in T]), idx, side="right")
    return out.reshape(fr["cut"].shape)


def uniform_frame(material, reflected=None, hit_colour="shade", ambient_fn=constant_ambient, **opts):
    """case B's float64 frame with every mesh shaded with one material"""
    return hc.render_with_reflection_meshes(meshes(), CAMERA, WIDTH, HEIGHT, FOCAL, ambient_fn, None, reflected, hit_colour, 1.0, **dict(dict(sun_dir=SUN, **material), **opts))


def material_frame(reflected=None, ambient_fn=constant_ambient, materials=MATERIALS, **opts):
    """the float64 frame with the floor and the plate shaded with their own materials (module docstring). Returns a dict: rgba (h, w, 4), owner,
    hit_mesh, C2 (h, w, 3: the mixed hit colour), unsafe (h, w: the primary ray, the shadow ray, the mirror ray or the hit is flagged),
    uniform (material key -> the second-round frame of that material) and cut."""
    own, own_unsafe = owner()
    first = {k: uniform_frame(m, reflected, "shade", ambient_fn, **opts) for k, m in materials.items()}
    any_fr = first[-1]
    hm = hit_mesh(any_fr)
    C2 = np.zeros((HEIGHT, WIDTH, 3))
    for k in materials:
        if k >= 0:
            C2 = np.where((hm == k)[..., None], first[k]["C2"], C2)
    second = {k: uniform_frame(m, reflected, C2, ambient_fn, **opts) for k, m in materials.items()}
    rgba = np.zeros((HEIGHT, WIDTH, 4))
    for k in materials:
        rgba = np.where((own == k)[..., None], second[k]["rgba"], rgba)
    unsafe = own_unsafe | any_fr["unsafe"] | (any_fr["owns"] & any_fr["t_unsafe"]) | any_fr["hit_unsafe"]
    return dict(rgba=rgba, owner=own, hit_mesh=hm, C2=C2, unsafe=unsafe, uniform=second, cut=any_fr["cut"], covered=any_fr["covered"], first=first)


def frame_bound(rgb_ref):
    return hc.frame_bound(rgb_ref)
