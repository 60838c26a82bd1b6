"""What test_frame_options_cpu.py and test_frame_options_gpu.py share: one hybrid Geometry frame in which every one of the six frame options
(include/ngp_hip.h: ngp_set_sun_nerf_shadow, ngp_set_sun_disk, ngp_set_mesh_reflection, ngp_set_mesh_reflection_meshes,
ngp_set_mesh_shadow_on_nerf, ngp_set_ambient_change_on_nerf) has pixels to act on, the 48 option sets, and the float64 reference of a frame
under any of them, composed from the single-option restatements the other cases modules hold.

The scene: the unit model over irradiance_bounce_reference.floor_scene(); nerf_mesh_shadow_cases' plate between the sun and half of the model;
sun_disk_cases' low plate moved to LOW_PLATE_CENTER, where it stands 0.25 above the floor beside the model, so that the floor shows its
shadow with a penumbra; mesh_reflection_meshes_cases' wall moved to the far side of the floor (x = -0.47 .. -0.43), where the sun (1, 1, 1)
lights the face the floor's mirror rays reach. The camera stands on the sun's side and looks down across the model at the wall. The sun, the
disk (5 degrees, 16 rays) and the NeRF-side descriptors are the other modules' own; the two SH9 volumes are ambient_change_cases.volumes().

The pixel classes (SHARES) are shares of the frame's pixels. "Mesh-covered" means that the pixel's primary ray found a triangle (the owner of
sun_disk_cases.mesh_geometry); every ray of this camera enters the inflated scene box, so the mesh pass's `covered` holds on all of them and
a pixel without a triangle is the mesh pass's opaque black at no depth: that is "no mesh covers it".

The reference, per option set (a frozenset of OPTIONS), in the order the header gives. Mesh layer (mesh_layer): M1-M4 by
sun_disk_cases.mesh_geometry; V = (K - count) / K on owners with the disk, else M4's boolean; with the sun shadow T_s = max(1 - alpha_s, 0)
on the pixels whose shadow-list entry is live (V > 0 with the disk, unshadowed by M4 without it); M5 by sun_disk_cases.mesh_colour; with the
reflection strength F (.) L_r is added, L_r = rgb_r, or rgb_r + max(1 - alpha_r, 0) C2 on cut rays with the sub-option, C2 shaded with the
central sun ray against all meshes (mesh_reflection_meshes_cases). NeRF layer (nerf_layer): n scaled by g with the ambient change, by f with
the meshes' shadow (1 - strength where blocked, or sun_disk_cases.factor of the count with the disk), composited over the mesh layer by
nerf_mesh_shadow_cases.composite. The ambient ratio is applied before the shadow's factor: fl(fl(n g) f). What only the network can supply
(alpha_s, rgb_r and alpha_r, n and its depth, the normal N) is handed in by the caller."""
import itertools

import numpy as np

import ambient_change_cases as ac
import irradiance_bounce_reference as br
import mesh_cases as mc
import mesh_reference as ref
import mesh_reflection_cases as rc
import mesh_reflection_meshes_cases as hc
import mesh_sun_nerf_shadow_cases as sc
import nerf_mesh_shadow_cases as nc
import sun_disk_cases as sd

WIDTH, HEIGHT = 60, 44                 # partial tiles on both axes
WALK_SIZES = ((52, 36), (120, 88))     # the frames rendered between two sets of the walk: smaller, and large enough to grow every buffer
FOCAL = sd.FOCAL
SUN, RADIUS, K = sd.SUN, sd.RADIUS, sd.K
CAMERA = mc.look_at((1.62, 1.12, 0.42), (0.5, 0.22, 0.49), up=(0.0, 1.0, 0.0))
LOW_PLATE_CENTER = (0.03, -0.35, 0.49)
WALL_SCALE, WALL_CENTER = hc.WALL_SCALE, (-0.95, 0.4, 0.0)
SUN_NERF = (0.01, 0.0)                 # min_transmittance, t_min
REFLECTION = dict(strength=1.0, min_transmittance=0.01, t_min=0.0)
SHADOW = dict(strength=nc.STRENGTH, bias=nc.BIAS)
DISK = dict(angular_radius=RADIUS, n_rays=K)
OPTIONS = ("sun", "disk", "refl", "hits", "shadow", "ambient")
ALL = frozenset(OPTIONS)
TRIPLES = (frozenset(("disk", "refl", "hits")), frozenset(("disk", "ambient", "shadow")), frozenset(("refl", "ambient", "shadow")))
# conditions on the case: the least share of the frame's pixels in each class, and the cap on the pixels the float64 tracer flags
SHARES = dict(mesh_alone=0.10, nerf_alone=0.10, nerf_over_mesh=0.05, disk_partial=0.03, disk_full=0.03, mirror_cut=0.03, mirror_open=0.03, nerf_soft=0.02, ambient_changed=0.05)
UNSAFE_CAP = sd.UNSAFE_CAP
COMPOSITE_ROUNDINGS = 4                # fl(n g), fl(. f), fl(m k) and their sum: the float32 roundings between the float64 composite and the frame's
_cache = {}


def option_sets():
    """the 48 distinct sets: the sub-option exists with the reflection alone"""
    out = []
    for bits in itertools.product((False, True), repeat=len(OPTIONS)):
        s = frozenset(o for o, b in zip(OPTIONS, bits) if b)
        if "hits" in s and "refl" not in s:
            continue
        out.append(s)
    return out


def gray_order():
    """the 48 sets, neighbours one option apart wherever the missing sets allow it: the 64 Gray-coded sets with the 16 that do not exist left out"""
    out = []
    for i in range(1 << len(OPTIONS)):
        code = i ^ (i >> 1)
        s = frozenset(o for k, o in enumerate(OPTIONS) if code >> k & 1)
        if not ("hits" in s and "refl" not in s):
            out.append(s)
    return out


def name(options):
    return "+".join(o for o in OPTIONS if o in options) or "none"


def scene():
    """[(triangles, centre)]: the floor, the plate above the model, the low plate, the wall"""
    low = (mc.cube().astype(np.float64) * np.array([1.0, 0.02, 1.0])).astype(np.float32)
    wall = (mc.cube().astype(np.float64) * np.array(WALL_SCALE)).astype(np.float32)
    return nc.scene() + [(low, LOW_PLATE_CENTER), (wall, WALL_CENTER)]


def meshes():
    if "meshes" not in _cache:
        _cache["meshes"] = br.normalised(scene())
    return _cache["meshes"]


def _cam(width, height, pixel_offset):
    return dict(matrix_3x4=CAMERA, width=width, height=height, focal=FOCAL, pixel_offset=tuple(pixel_offset))


def geometry(width=WIDTH, height=HEIGHT, pixel_offset=(0.5, 0.5), s=0):
    """what the mesh layer is before any radiance is handed in, once per process and view: sun_disk_cases.mesh_geometry's dict with, per pixel
    (h w), the disk's count and flagged under the table of spp index s, and `mirror`, mesh_reflection_meshes_cases' frame with nothing
    handed in (owns, rq, r, t_hit, cut, p2, shadow2, C2 and their flags)"""
    key = ("geometry", width, height, tuple(pixel_offset), s)
    if key not in _cache:
        g = dict(sd.mesh_geometry(pixel_offset, width, height, meshes(), CAMERA))
        own = g["owner"]
        count, flagged = np.zeros(own.size, np.int64), np.zeros(own.size, bool)
        count[own], flagged[own] = sd.counts(g["meshes"], g["q"][own], sd.directions(SUN, RADIUS, K, s))
        g.update(count=count, flagged=flagged, s=s, pixel_offset=tuple(pixel_offset),
                 mirror=hc.render_with_reflection_meshes(meshes(), CAMERA, width, height, FOCAL, sc.no_ambient, hit_colour="shade", sun_dir=SUN, pixel_offset=tuple(pixel_offset)))
        _cache[key] = g
    return _cache[key]


def mesh_layer(options, geo, alpha_s=None, reflected=None, ambient_fn=sc.no_ambient, hit_colour="shade", **brdf):
    """the mesh pass's frame under the option set. alpha_s (h, w) float32: the alpha of each live shadow-list entry's ray through the NeRF;
    reflected (h, w, 4) float32: (rgb_r, alpha_r) of each mirror ray; both looked at only where the option set and the pixel call for them.
    Returns a dict: rgba (h, w, 4) float64, unsafe (h, w: the pixels a float32 tracer may decide otherwise, over all the rays the pixel owns
    under this set), V and T_s (h, w, float64), live (h, w), mirror (the reflection's frame, None without it) and bound (h, w, 3): the sum of
    the single-option tests' colour bounds for the terms present -- mesh_sun_nerf_shadow_cases.frame_bound of the colour; with the reflection
    GPU_FACTOR x the float32 form's own deviation of the added term; with the sub-option, on cut rays, strength F max(1 - alpha_r, 0) x
    frame_bound(C2), what test_mesh_reflection_meshes_gpu.py grants the hit's colour."""
    h, w = geo["shape"]
    owner, shadowed = geo["owner"], geo["shadowed"]
    hard = np.where(shadowed, 0.0, 1.0)
    V = np.where(owner, sd.visibility(geo["count"], K).astype(np.float64), hard) if "disk" in options else hard
    live = geo["covered"] & (V > 0)
    T = np.ones(h * w)
    if "sun" in options:
        T = np.where(live, sc.factor_of(np.asarray(alpha_s, np.float32).reshape(-1)).astype(np.float64), 1.0)
    rgba, unsafe = sd.mesh_colour(geo, V, T, ambient_fn, **brdf)
    unsafe = unsafe | (owner & (geo["flagged"] if "disk" in options else geo["shadow_unsafe"])).reshape(h, w)
    bound = sc.frame_bound(rgba[..., :3])
    mirror = None
    if "refl" in options:
        mirror = hc.render_with_reflection_meshes(meshes(), CAMERA, w, h, FOCAL, ambient_fn, None, reflected, hit_colour if "hits" in options else None, REFLECTION["strength"],
                                                  sun_dir=SUN, pixel_offset=geo["pixel_offset"], **brdf)
        covered = geo["covered"].reshape(h, w)
        rgba[..., :3] = np.where(covered[..., None], rgba[..., :3] + mirror["added"], rgba[..., :3])
        unsafe = unsafe | (mirror["owns"] & mirror["t_unsafe"])
        bound = sc.frame_bound(rgba[..., :3]) + mc.GPU_FACTOR * np.abs(mirror["added32"].astype(np.float64) - mirror["added"])
        if "hits" in options:
            unsafe = unsafe | mirror["hit_unsafe"]
            through = np.maximum(1.0 - np.where(mirror["owns"], np.asarray(reflected, np.float32).reshape(h, w, 4)[..., 3], 0).astype(np.float64), 0.0)
            bound = bound + np.where(mirror["cut"][..., None], REFLECTION["strength"] * mirror["F"] * through[..., None] * hc.frame_bound(mirror["C2"]), 0.0)
    return dict(rgba=rgba, unsafe=unsafe, V=V.reshape(h, w), T_s=T.reshape(h, w), live=live.reshape(h, w), mirror=mirror, bound=bound)


def nerf_shadow(options, nerf_alpha, depth, p=None, width=WIDTH, height=HEIGHT, pixel_offset=(0.5, 0.5), s=0):
    """the meshes' shadow on the NeRF restated from the NeRF's alpha (h, w) and depth (h, w): nerf_mesh_shadow_cases.shadow on this scene and
    camera, and with the disk sun_disk_cases' count from q = p + bias s^ along the table of spp index s. p (h, w, 3): the points to trace
    from in place of the restated ones (the record's own, as the single-option tests trace). Returns that function's dict with count, flagged
    (h, w), f (float32: 1 without the option) and w, the record's fourth float."""
    sh = nc.shadow(nerf_alpha, depth, meshes(), SHADOW["strength"], SHADOW["bias"], SUN, **_cam(width, height, pixel_offset))
    owner = sh["owner"].reshape(-1)
    shape = sh["owner"].shape
    pts = sh["p"].reshape(-1, 3) if p is None else np.asarray(p, np.float64).reshape(-1, 3)
    count, flagged = np.zeros(owner.size, np.int64), np.zeros(owner.size, bool)
    if "disk" in options:
        q = pts[owner] + SHADOW["bias"] * sc.s_hat(SUN).astype(np.float64)
        count[owner], flagged[owner] = sd.counts(meshes(), q, sd.directions(SUN, RADIUS, K, s))
        f = np.where(owner, sd.factor(count, K, SHADOW["strength"]), np.float32(1)).astype(np.float32)
        rec_w = np.where(owner, np.float32(1) + (count.astype(np.float32) / np.float32(K)).astype(np.float32), np.float32(0))
    else:
        blocked, flagged[owner] = nc.blocked_from(pts[owner], meshes(), SHADOW["bias"], SUN)
        count[owner] = np.where(blocked, K, 0)
        f = np.where(count == K, np.float32(1) - np.float32(SHADOW["strength"]), np.float32(1)).astype(np.float32)
        rec_w = np.where(owner, np.where(count == K, np.float32(2), np.float32(1)), np.float32(0))
    if "shadow" not in options:
        f = np.ones(owner.size, np.float32)
    return dict(sh, count=count.reshape(shape), flagged=flagged.reshape(shape), f=f.reshape(shape), w=rec_w.reshape(shape).astype(np.float32))


def nerf_layer(options, n, m, f=None, g=None):
    """the frame in float32 from the NeRF's own premultiplied pixel n, the mesh layer m (both (h, w, 4) float32), the shadow's factor f (h, w)
    and the ambient ratio g (h, w, 3): ambient_change_cases.composite, g first, then f; an option that is off contributes 1"""
    n = np.asarray(n, np.float32)
    one = np.ones(n.shape[:2], np.float32)
    f = one if "shadow" not in options or f is None else np.asarray(f, np.float32)
    g = np.ones(n.shape[:2] + (3,), np.float32) if "ambient" not in options or g is None else np.asarray(g, np.float32)
    return ac.composite(n, m, g, f)


def frame(options, measured=None, width=WIDTH, height=HEIGHT, pixel_offset=(0.5, 0.5), s=0, **shading):
    """the frame under the option set: colour, depth and every pass's record. measured: a dict of what only the network supplies, each entry
    looked at only where the set calls for it: alpha_s (h, w), reflected (h, w, 4), n (h, w, 4: the NeRF's own pixel, what the depth test
    culls taken out), n_depth (h, w: the NeRF pass's depth of its owners), g (h, w, 3: the ambient ratio; ambient_change_cases.ratio at the
    recorded p and N rounded to float32 is what the caller hands in) and p (h, w, 3: the owners' points to trace the shadow from). Without n
    the NeRF layer is empty. Returns a dict: rgba (h, w, 4) float64, the composite formed in float64; rgba32, the same through the float32
    composite over the float64 mesh layer rounded to float32 (as bytes it is the frame's wherever the mesh layer is the opaque black of no
    mesh); depth; bound (h, w, 3); unsafe (h, w); mesh (mesh_layer's dict), shadow (nerf_shadow's, None without n); and records, a dict by
    the getter's name of the arrays the passes of this set leave, None for a pass the set does not run."""
    options = frozenset(options)
    measured = measured or {}
    geo = geometry(width, height, pixel_offset, s)
    mesh = mesh_layer(options, geo, measured.get("alpha_s"), measured.get("reflected"), **shading)
    h, w = height, width
    own = geo["owner"].reshape(h, w)
    m64 = mesh["rgba"]
    depth = np.where(geo["covered"], ((geo["pos"] - geo["M"][:, 3]) * geo["M"][:, 2]).sum(1), ref.MAX_DEPTH).reshape(h, w)
    rec = dict.fromkeys(("frame_sun_shadow", "frame_sun_disk", "frame_mesh_reflection", "frame_mesh_reflection_hits", "frame_mesh_shadow", "frame_ambient_change"))
    q = geo["q"].reshape(h, w, 3)
    if "sun" in options:
        live = mesh["live"]
        a_s = np.zeros((h, w), np.float32) if measured.get("alpha_s") is None else np.asarray(measured["alpha_s"], np.float32)
        rec["frame_sun_shadow"] = dict(live=live, q=np.where(live[..., None], q, 0.0), alpha_s=np.where(live, a_s, np.float32(0)))
    if "disk" in options:
        rec["frame_sun_disk"] = dict(owner=own, q=q, count=geo["count"].reshape(h, w), flagged=geo["flagged"].reshape(h, w))
    if "refl" in options:
        mr = mesh["mirror"]
        rec["frame_mesh_reflection"] = dict(owns=mr["owns"], q=mr["rq"], r=mr["r"], t_hit=mr["t_hit"], t_unsafe=mr["t_unsafe"])
        if "hits" in options:
            rec["frame_mesh_reflection_hits"] = dict(cut=mr["cut"], p2=mr["p2"], shadow2=mr["shadow2"], C2=mr["C2"], hit_unsafe=mr["hit_unsafe"])
    out = dict(mesh=mesh, shadow=None, records=rec, unsafe=mesh["unsafe"].copy(), depth=depth)
    n = measured.get("n")
    if n is None:
        out.update(rgba=m64, rgba32=m64.astype(np.float32), bound=mesh["bound"])
        return out
    n = np.asarray(n, np.float32)
    sh = nerf_shadow(options, n[..., 3], measured["n_depth"], measured.get("p"), width, height, pixel_offset, s)
    f = sh["f"]
    g = np.ones((h, w, 3), np.float32) if "ambient" not in options else np.where(sh["owner"][..., None], np.asarray(measured["g"], np.float32), np.float32(1))
    k = 1.0 - n[..., 3:4].astype(np.float64)
    scaled = n[..., :3].astype(np.float64) * g.astype(np.float64) * f.astype(np.float64)[..., None]
    rgba = np.where(n[..., 3:4] == 0, m64, np.concatenate([scaled + m64[..., :3] * k, n[..., 3:4].astype(np.float64) + m64[..., 3:4] * k], -1))
    bound = mesh["bound"] * np.where(n[..., 3:4] == 0, 1.0, np.abs(k)) + np.where(n[..., 3:4] == 0, 0.0, COMPOSITE_ROUNDINGS * 2.0 ** -24 * np.maximum(1.0, np.abs(rgba[..., :3])))
    if "shadow" in options:
        rec["frame_mesh_shadow"] = dict(owner=sh["owner"], p=sh["p"], w=sh["w"], count=sh["count"], flagged=sh["flagged"])
        out["unsafe"] |= sh["flagged"]
    if "ambient" in options:
        rec["frame_ambient_change"] = dict(owner=sh["owner"], p=sh["p"], g=g)
    out.update(rgba=rgba, rgba32=nerf_layer(options, n, m64.astype(np.float32), f, g), bound=bound, shadow=sh, depth=np.where(sh["owner"], np.asarray(measured["n_depth"], np.float64), depth))
    return out


def classes(geo, nerf_alpha_alone, nerf_alpha, nerf_count, changed):
    """the shares of SHARES, as fractions of the frame's pixels, from the geometry, the model's own alpha (h, w; before the depth test),
    its alpha behind the depth test (an owner there is nearer than the mesh), the NeRF owners' soft-shadow count and the mask of owners
    whose ambient ratio has state 2 and g != 1 in some channel. A pixel is counted where it is on its class's side of the 0.2 owner
    threshold by nerf_mesh_shadow_cases.OWNER_ALPHA, the margin the depth write itself uses: alpha > 0.2 is an owner, alpha = 0 is empty."""
    h, w = geo["shape"]
    own = geo["owner"].reshape(h, w)
    mr = geo["mirror"]
    owner_n = np.asarray(nerf_alpha, np.float32) > np.float32(nc.OWNER_ALPHA)
    count = geo["count"].reshape(h, w)
    n = float(h * w)
    return dict(mesh_alone=(own & (np.asarray(nerf_alpha_alone) == 0)).sum() / n, nerf_alone=(~own & owner_n).sum() / n, nerf_over_mesh=(own & owner_n).sum() / n,
                disk_partial=(own & (count > 0) & (count < K)).sum() / n, disk_full=(own & (count == K)).sum() / n, mirror_cut=(mr["owns"] & mr["cut"]).sum() / n,
                mirror_open=(mr["owns"] & ~mr["cut"]).sum() / n, nerf_soft=(owner_n & (np.asarray(nerf_count) > 0)).sum() / n, ambient_changed=(owner_n & np.asarray(changed, bool)).sum() / n)


def flagged_pixels(geo, nerf_flagged=None):
    """(h, w): the pixels the float64 tracer flags as ties over all the rays a pixel owns with every option on: the primary ray, the K disk
    rays, the mirror ray, the mirrored hit's shadow ray and shading, and the NeRF owner's K rays"""
    h, w = geo["shape"]
    mr = geo["mirror"]
    out = (geo["primary_unsafe"] | (geo["owner"] & geo["flagged"])).reshape(h, w) | mr["unsafe"] & ~geo["owner"].reshape(h, w) | (mr["owns"] & (mr["t_unsafe"] | mr["hit_unsafe"]))
    # (mirror["unsafe"] holds M4's own shadow ray, which an owner's disk replaces; it counts where the pixel owns no disk)
    return out if nerf_flagged is None else out | np.asarray(nerf_flagged, bool)
