"""Mesh materials on the GPU (include/ngp_hip.h, "mesh materials"): the identities the contract promises as bytes, the id plane against the
float64 owner, the per-pixel selection as bytes against the uniform frames that ngp_set_geometry_opts renders through the kernels without
materials, the mixed pixels of cut mirror rays against the float64 restatement, all six frame options at once, the other frame layouts and
devices, lifetime on a device and the bindings. The scene and the materials are mesh_material_cases'; every material carries the ambient
colour 0.3, so that the sky term is at work. The measured figures are in DESIGN 3.22."""
import json
import subprocess

import numpy as np
import pytest

from conftest import pkg

import ambient_change_cases as ac
import frame_options_cases as fo
import mesh_cases as mc
import mesh_material_cases as mm
import mesh_reflection_meshes_cases as hc
import mesh_volume_cases as mv

pytestmark = pytest.mark.gpu

W, H = mm.WIDTH, mm.HEIGHT
ON = dict(strength=1.0, min_transmittance=0.01, t_min=0.0)
AMBIENT = (mm.AMBIENT,) * 3
UP = (1.0, 0.0, 0.0)  # the sky term reaches every normal of the case: with the default up a floor pixel in the plate's shadow is black under every material
MATERIALS = {k: dict(m, ambientcolor=AMBIENT) for k, m in mm.MATERIALS.items()}  # by owner mesh; -1: the context's
VOLUME_BOX = (np.float32([-0.1, -0.2, -0.1]), np.float32([1.6, 1.5, 1.1]))
MODES = ("Shade", "ShadeEnvMap", "ShadeIrradianceVolume", "ShadeIrradianceVolumeVisible")
GETTERS = (("frame_sun_shadow", 4), ("frame_sun_disk", 4), ("frame_mesh_reflection", 12), ("frame_mesh_reflection_hits", 8), ("frame_mesh_shadow", 4), ("frame_ambient_change", 12))


def _mode(native, mode):
    return {"Shade": native.RENDER_SHADE, "ShadeEnvMap": native.RENDER_SHADE_ENVMAP}.get(mode, native.RENDER_SHADE_IRRADIANCE_VOLUME)


def _opts(native, mode="Shade", **kw):
    return native.make_opts(**dict(dict(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0), render_mode=_mode(native, mode)), **kw))


def _cam(native, w=W, h=H, **kw):
    return native.make_camera(mm.CAMERA, w, h, mm.FOCAL, **kw)


def _render(c, native, mode="Shade", cam=None, **kw):
    return c.render(cam or _cam(native), _opts(native, mode, **kw), want_depth=True)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _uniform(c, material):
    """every mesh shaded with one material through the context's options: no mesh owns a material, the kernels are those without materials"""
    for i in range(c.n_meshes()):
        c.set_mesh_material(i, None)
    c.set_geometry_opts(sun_dir=mm.SUN, up_dir=UP, **material)


def _per_mesh(c, materials=MATERIALS):
    c.set_geometry_opts(sun_dir=mm.SUN, up_dir=UP, **materials[-1])
    for i in range(c.n_meshes()):
        c.set_mesh_material(i, materials.get(i))


def _copies(c, material):
    """every mesh owns a copy of the context's material"""
    c.set_geometry_opts(sun_dir=mm.SUN, up_dir=UP, **material)
    for i in range(c.n_meshes()):
        c.set_mesh_material(i, material)


def _sources(c, mode):
    c.clear_irradiance_volume()
    if mode == "ShadeEnvMap":
        c.compute_envmap(n_theta=16, n_phi=8)
    elif mode.startswith("ShadeIrradianceVolume"):
        c.compute_irradiance_volume((3, 2, 3), VOLUME_BOX, 8, 8, occlude_by_meshes=False)
        if mode.endswith("Visible"):
            c.compute_irradiance_volume_visibility(n_u=8, n_v=8, sharpness_log2=4, max_distance=0.0, normal_bias=0.01)


def _context(native, scene_unit, model=True, devices=None):
    c = native.Context(0) if devices is None else native.Context(devices=devices)
    if model:
        c.set_model(scene_unit)
    for tris, center in mm.scene():
        c.add_mesh(tris, center)
    c.set_geometry_opts(sun_dir=mm.SUN, up_dir=UP, **MATERIALS[-1])
    return c


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    c = _context(native, scene_unit)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare(gpu_ctx, native, scene_unit):
    c = _context(native, scene_unit, model=False)
    yield c
    c.close()


@pytest.fixture()
def clean(hybrid, bare):
    """every test leaves both contexts with no materials, no options and the context's material"""
    yield
    for c in (hybrid, bare):
        _uniform(c, MATERIALS[-1])
        c.set_mesh_reflection(None)
        c.set_mesh_reflection_meshes(False)
        c.set_sun_nerf_shadow(None)
        c.set_sun_disk(None)
        c.set_mesh_shadow_on_nerf(None)
        c.set_ambient_change_on_nerf(None)
        c.clear_irradiance_volume()


@pytest.fixture(scope="module")
def owner():
    own, unsafe = mm.owner()
    return own, ~unsafe


@pytest.fixture(scope="module")
def fused(bare, native):
    """the meshes alone in Shade: the three uniform frames, the per-mesh frame and its ids"""
    out = {}
    for k, m in MATERIALS.items():
        _uniform(bare, m)
        out[k] = _render(bare, native)
    _per_mesh(bare)
    out["materials"] = _render(bare, native)
    out["ids"] = bare.frame_mesh_ids(W * H).reshape(H, W)
    _uniform(bare, MATERIALS[-1])
    return out


def _selected(frames, ids):
    """the frame that takes each pixel from the uniform frame of that pixel's material"""
    colour = np.zeros_like(frames[-1][0])
    for k in MATERIALS:
        colour[ids == k] = frames[k][0][ids == k]
    return colour


# ------------------------------------------------------------------------------------------------------------------ 1 identities
@pytest.mark.parametrize("mode", MODES)
def test_identities_as_bytes(mode, hybrid, bare, native, clean):
    """no materials against every mesh owning the context's copy, colour and depth: the fused pass (meshes alone, Shade) and the split pass
    (the reflection on over the unit model) under every ambient source"""
    rich = dict(MATERIALS[0], clearcoat=0.5, sheen=0.5, subsurface=0.2)
    if mode == "Shade":
        _uniform(bare, rich)
        plain = _render(bare, native)
        with pytest.raises(RuntimeError, match="ran without mesh materials"):
            bare.frame_mesh_ids(W * H)
        _copies(bare, rich)
        assert _same(_render(bare, native), plain) and (bare.frame_mesh_ids(W * H) >= 0).sum() >= 800
    _sources(hybrid, mode)
    hybrid.set_mesh_reflection(ON)
    hybrid.set_mesh_reflection_meshes(True)
    _uniform(hybrid, rich)
    plain = _render(hybrid, native, mode)
    records = [hybrid.frame_mesh_reflection(W * H), hybrid.frame_mesh_reflection_hits(W * H)]
    _copies(hybrid, rich)
    assert _same(_render(hybrid, native, mode), plain) and (plain[0][..., 3] == 1).sum() > 2000
    assert hybrid.frame_mesh_reflection(W * H).tobytes() == records[0].tobytes() and hybrid.frame_mesh_reflection_hits(W * H).tobytes() == records[1].tobytes()


# -------------------------------------------------------------------------------------------------------------------------- 2 ids
def test_ids_are_the_float64_owner(hybrid, fused, owner, native, clean):
    """on safe pixels frame_mesh_ids is the float64 owner; -1 on the 2205 others; the fused and the split pass give equal bytes"""
    own, safe = owner
    ids = fused["ids"]
    print("\nids: floor %d, plate %d, none %d; safe pixels %d" % ((ids == 0).sum(), (ids == 1).sum(), (ids == -1).sum(), safe.sum()))
    assert np.array_equal(ids[safe], own[safe]) and safe.sum() >= (1 - mm.UNSAFE_CAP) * W * H
    assert (ids == -1).sum() == (own == -1).sum() == 2205 and set(np.unique(ids)) == {-1, 0, 1}
    _per_mesh(hybrid)
    hybrid.set_mesh_reflection(ON)
    _render(hybrid, native)
    assert hybrid.frame_mesh_ids(W * H).tobytes() == ids.tobytes()
    hybrid.set_mesh_reflection(None)
    hybrid.set_sun_disk(dict(angular_radius=0.05, n_rays=4))
    _render(hybrid, native)
    assert hybrid.frame_mesh_ids(W * H).tobytes() == ids.tobytes()


# -------------------------------------------------------------------------------------------------------------------- 3 selection
@pytest.mark.parametrize("mode", MODES)
def test_selection_per_pixel_as_bytes(mode, hybrid, bare, fused, owner, native, clean):
    """the fused pass: on safe pixels the material frame is, pixel by pixel as bytes, the uniform frame of that pixel's material; depth is
    every frame's. The split pass with the reflection on and the mirrored meshes off: the same on every pixel, F being the pixel's own."""
    own, safe = owner
    if mode == "Shade":
        frames, mat, ids = fused, fused["materials"], fused["ids"]
    else:  # (the probes and the volume are traced through the model: the fused mesh pass of the hybrid context, the NeRF pass composited over it)
        _sources(hybrid, mode)
        frames = {}
        for k, m in MATERIALS.items():
            _uniform(hybrid, m)
            frames[k] = _render(hybrid, native, mode)
        _per_mesh(hybrid)
        mat, ids = _render(hybrid, native, mode), hybrid.frame_mesh_ids(W * H).reshape(H, W)
    want = _selected(frames, own)
    assert mat[0][safe].tobytes() == want[safe].tobytes()
    assert mat[0].tobytes() == _selected(frames, ids).tobytes() and all(mat[1].tobytes() == frames[k][1].tobytes() for k in MATERIALS)
    differs = {k: (np.abs(mat[0] - frames[-1][0]).max(-1) > 0)[ids == k].sum() for k in (0, 1)}
    print("\n%s: pixels that differ from the context-material frame: floor %d of %d, plate %d of %d" % (mode, differs[0], (ids == 0).sum(), differs[1], (ids == 1).sum()))
    if mode == "Shade":  # (the meshes alone: every mesh pixel shows; over the model an opaque NeRF pixel hides its mesh pixel whole)
        assert differs[0] == (ids == 0).sum() >= mm.MIN_CLASS and differs[1] == (ids == 1).sum() >= mm.MIN_CLASS
    assert not _same(mat, frames[-1])
    # the split pass
    _sources(hybrid, mode)
    hybrid.set_mesh_reflection(ON)
    split = {}
    for k, m in MATERIALS.items():
        _uniform(hybrid, m)
        split[k] = _render(hybrid, native, mode)
    _per_mesh(hybrid)
    got = _render(hybrid, native, mode)
    sids = hybrid.frame_mesh_ids(W * H).reshape(H, W)
    assert got[0].tobytes() == _selected(split, sids).tobytes() and got[1].tobytes() == split[-1][1].tobytes()
    assert not _same(got, split[-1])


# ------------------------------------------------------------------------------------------------------------------ 4 mixed pixels
def test_mixed_pixels_match_the_restatement(hybrid, fused, native, clean):
    """mesh_reflection_meshes on over the unit model (the reflection serves hybrid frames alone: a frame of the meshes alone traces no mirror
    ray, and the bare context's frame with both options on is its plain frame as bytes): a cut pixel multiplies its own material's F by the C2
    of the hit mesh's material. The cut pixels the NeRF pass left alone are compared against the float64 restatement fed with the recorded
    (rgb_r, alpha_r). The allowance is measured first: the largest deviation of the uniform frames of the floor and the plate material from
    their float64 references on those pixels, in frame_bound; the mixed pixels get frame_bound where that is <= 0.5, else twice the measured
    value."""
    c = hybrid
    ambient = mv.sky_ambient_fn(AMBIENT, UP)
    plain = _render(c, native)  # clear pixels: the plain hybrid frame is the frame of the meshes alone as bytes, the NeRF pass added nothing
    clear = np.all(plain[0].view(np.uint32) == fused[-1][0].view(np.uint32), axis=-1) & (plain[1].view(np.uint32) == fused[-1][1].view(np.uint32))
    c.set_mesh_reflection(ON)
    c.set_mesh_reflection_meshes(True)
    measured = 0.0
    for k in (0, 1):
        _uniform(c, MATERIALS[k])
        got = _render(c, native)
        rec = c.frame_mesh_reflection(W * H).reshape(H, W, 12)
        fr = mm.uniform_frame(mm.MATERIALS[k], rec[..., 8:12], "shade", ambient)
        m = fr["cut"] & ~fr["unsafe"] & ~fr["t_unsafe"] & ~fr["hit_unsafe"] & clear
        dev = (np.abs(got[0][..., :3].astype(np.float64) - fr["rgba"][..., :3]) / mm.frame_bound(fr["rgba"][..., :3]))[m].max()
        measured = max(measured, float(dev))
    allowance = 1.0 if measured <= 0.5 else 2.0 * measured
    _per_mesh(c)
    got = _render(c, native)
    rec = c.frame_mesh_reflection(W * H).reshape(H, W, 12)
    ids = c.frame_mesh_ids(W * H).reshape(H, W)
    fr = mm.material_frame(rec[..., 8:12], ambient)
    m = fr["cut"] & ~fr["unsafe"] & clear
    ratio = (np.abs(got[0][..., :3].astype(np.float64) - fr["rgba"][..., :3]) / mm.frame_bound(fr["rgba"][..., :3]))[m]
    both = ((fr["owner"] == 0) & (fr["hit_mesh"] == 1) & m).sum(), ((fr["owner"] == 1) & (fr["hit_mesh"] == 0) & m).sum()
    print("\nuniform frames deviate by %.3f frame_bound on cut pixels -> allowance %.3f; mixed pixels %d of %d cut (floor onto plate %d, plate onto floor %d): largest %.3f"
          % (measured, allowance, m.sum(), fr["cut"].sum(), both[0], both[1], ratio.max()))
    assert np.array_equal(ids[~fr["unsafe"]], fr["owner"][~fr["unsafe"]])
    assert both[0] >= 50 and both[1] >= 50
    assert ratio.max() <= allowance, ratio.max()


# --------------------------------------------------------------------------------------------------------------- 5 all six options
def test_all_six_options_on(hybrid, native, clean):
    """every frame option on: depth and every geometric record -- the sun shadow, the sun disk, the mesh shadow on the NeRF, the ambient change,
    the reflection's three float4 and the hits' (p2, shadow2) -- are the no-material frame's as bytes. C2 differs on every cut ray, which is
    both cut classes (120 and 159). The colour differs on every floor and plate pixel that the NeRF pass left alone (an opaque NeRF pixel in
    front hides its mesh pixel whole, under any material), and on at least 100 floor pixels; the plate shows on fewer than 100 pixels of
    this frame beside the model, so its count is printed and held to the pixels the NeRF left alone."""
    c = hybrid
    after, before, _ = ac.volumes()
    c.set_irradiance_volume(mv.as_grid(after, ac.RES), (ac.LO, ac.HI), ac.N_U, ac.N_V)
    c.set_reference_irradiance_volume(mv.as_grid(before, ac.RES), (ac.LO, ac.HI), ac.N_U, ac.N_V)
    c.set_sun_nerf_shadow(fo.SUN_NERF)
    c.set_sun_disk(fo.DISK)
    c.set_mesh_reflection(fo.REFLECTION)
    c.set_mesh_reflection_meshes(True)
    c.set_mesh_shadow_on_nerf(fo.SHADOW)
    c.set_ambient_change_on_nerf(True)
    _uniform(c, MATERIALS[-1])
    plain = _render(c, native)
    plain_rec = {name: getattr(c, name)(W * H) for name, _ in GETTERS}
    _per_mesh(c)
    got = _render(c, native)
    rec = {name: getattr(c, name)(W * H) for name, _ in GETTERS}
    ids = c.frame_mesh_ids(W * H).reshape(H, W)
    assert got[1].tobytes() == plain[1].tobytes()
    for name, _ in GETTERS:
        if name != "frame_mesh_reflection_hits":
            assert rec[name].tobytes() == plain_rec[name].tobytes(), name
    hits, plain_hits = rec["frame_mesh_reflection_hits"].reshape(H, W, 8), plain_rec["frame_mesh_reflection_hits"].reshape(H, W, 8)
    assert hits[..., :4].tobytes() == plain_hits[..., :4].tobytes() and hits[..., 7].tobytes() == plain_hits[..., 7].tobytes()
    cut = hits[..., 7] != 0
    c2_differs = (np.abs(hits[..., 4:7] - plain_hits[..., 4:7]).max(-1) > 0) & cut
    colour_differs = np.abs(got[0] - plain[0]).max(-1) > 0
    print("\nall six on: cut rays %d, C2 differs on %d; the colour differs on %d floor and %d plate pixels" % (cut.sum(), c2_differs.sum(), (colour_differs & (ids == 0)).sum(), (colour_differs & (ids == 1)).sum()))
    assert c2_differs.sum() == cut.sum() == 279
    c.set_mesh_shadow_on_nerf(None)
    c.set_ambient_change_on_nerf(None)
    c.set_sun_nerf_shadow(None)
    c.set_sun_disk(None)
    c.set_mesh_reflection(None)
    _uniform(c, MATERIALS[-1])
    hybrid_plain = _render(c, native)
    b = native.Context(0)
    try:
        for tris, center in mm.scene():
            b.add_mesh(tris, center)
        b.set_geometry_opts(sun_dir=mm.SUN, up_dir=UP, **MATERIALS[-1])
        alone = _render(b, native)
    finally:
        b.close()
    clear = np.all(hybrid_plain[0].view(np.uint32) == alone[0].view(np.uint32), axis=-1)  # the NeRF pass added nothing
    print("pixels the NeRF pass left alone: floor %d, plate %d" % ((clear & (ids == 0)).sum(), (clear & (ids == 1)).sum()))
    assert np.all(colour_differs[clear & (ids >= 0)]) and (clear & (ids == 1)).sum() >= 50
    assert (colour_differs & (ids == 0)).sum() >= mm.MIN_CLASS


# ------------------------------------------------------------------------------------------------------------------ 6 other layouts
def _tiles(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // 8) * ((w + 7) // 8) + xs // 8, (xs % 8) + 8 * (ys % 8)


def test_two_samples_ids_of_the_last(bare, native, clean):
    _per_mesh(bare)
    cam = _cam(native, snap=False)
    _render(bare, native, cam=cam, spp=2)
    ids2 = bare.frame_mesh_ids(W * H)
    _render(bare, native, cam=_cam(native, snap=False, spp_index=1))
    last = bare.frame_mesh_ids(W * H)
    _render(bare, native, cam=cam)
    first = bare.frame_mesh_ids(W * H)
    assert ids2.tobytes() == last.tobytes() and ids2.tobytes() != first.tobytes()


@pytest.mark.parametrize("split", [False, True])
def test_shards_and_packed_shards(split, hybrid, bare, native, clean):
    """three shards in image layout and tile-packed at 60 x 44 against the whole frame: colour, depth and ids, which follow the frame's pixel order"""
    import torch

    c = hybrid if split else bare
    if split:
        c.set_mesh_reflection(ON)
        c.set_mesh_reflection_meshes(True)
    _per_mesh(c)
    w, h, world = 60, 44, 3
    cam = _cam(native, w=w, h=h)
    tile, slot = _tiles(w, h)
    full, full_depth = _render(c, native, cam=cam)
    full_ids = c.frame_mesh_ids(w * h).reshape(h, w)
    assert (full_ids == 0).sum() > 100 and (full_ids == 1).sum() > 100
    total, total_depth, total_ids = np.zeros_like(full), np.zeros_like(full_depth), np.full_like(full_ids, -1)
    packed, packed_depth, packed_ids = np.zeros_like(full), np.zeros_like(full_depth), np.full_like(full_ids, -1)
    for rank in range(world):
        mine = tile % world == rank
        part, part_depth = _render(c, native, cam=cam, shard_index=rank, shard_count=world)
        ids = c.frame_mesh_ids(w * h).reshape(h, w)
        assert not np.any(part[~mine]) and np.all(ids[~mine] == -1)
        total[mine], total_depth[mine], total_ids[mine] = part[mine], part_depth[mine], ids[mine]
        n = native.load_library().ngp_packed_tiles(w, h, rank, world) * 64
        rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
        c.render_device(cam, _opts(native, shard_index=rank, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
        ids = c.frame_mesh_ids(n)  # (synchronises the context's stream)
        src = (tile // world) * 64 + slot
        packed[mine], packed_depth[mine], packed_ids[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]], ids[src[mine]]
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes() and total_ids.tobytes() == full_ids.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes() and packed_ids.tobytes() == full_ids.tobytes()


def test_two_devices_a_callers_stream_and_run_to_run(hybrid, native, scene_unit, clean):
    """the split pass with the mirrored meshes on. Twice on one context: the same bytes. On a caller's stream: the same bytes. On a context of
    two devices (the same ordinal twice): the materials reach the replica with the geometry, set before and changed after the first frame;
    the ids are the primary's tile-packed share"""
    import torch

    hybrid.set_mesh_reflection(ON)
    hybrid.set_mesh_reflection_meshes(True)
    _per_mesh(hybrid)
    one = _render(hybrid, native)
    ids = hybrid.frame_mesh_ids(W * H).reshape(H, W)
    hits = hybrid.frame_mesh_reflection_hits(W * H)
    assert _same(_render(hybrid, native), one) and hybrid.frame_mesh_reflection_hits(W * H).tobytes() == hits.tobytes()
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    hybrid.render_device(_cam(native), _opts(native), rgba.data_ptr(), dep.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert rgba.cpu().numpy().tobytes() == one[0].tobytes() and dep.cpu().numpy().tobytes() == one[1].tobytes()
    assert hybrid.frame_mesh_ids(W * H).tobytes() == ids.tobytes()
    swapped = {-1: MATERIALS[-1], 0: MATERIALS[1], 1: MATERIALS[0]}
    _per_mesh(hybrid, swapped)
    other = _render(hybrid, native)
    assert not _same(other, one)
    multi = _context(native, scene_unit, devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_mesh_reflection(ON)
        multi.set_mesh_reflection_meshes(True)
        _per_mesh(multi)
        assert _same(_render(multi, native), one)
        n = native.load_library().ngp_packed_tiles(W, H, 0, 2) * 64
        tile, slot = _tiles(W, H)
        mine = tile % 2 == 0
        assert multi.frame_mesh_ids(n)[((tile // 2) * 64 + slot)[mine]].tobytes() == ids[mine].tobytes()
        _per_mesh(multi, swapped)  # the materials alone change: the replica's table follows
        assert _same(_render(multi, native), other)
        _uniform(multi, MATERIALS[-1])
        _uniform(hybrid, MATERIALS[-1])
        assert _same(_render(multi, native), _render(hybrid, native))
    finally:
        multi.close()


# ---------------------------------------------------------------------------------------------------------- 7 lifetime on a device
def test_lifetime_and_refusals_on_a_device(bare, fused, native, clean):
    """the ids refuse after a no-material frame; a material set before ngp_clear_meshes does not reappear on a new mesh 0;
    ngp_set_geometry_opts after set_mesh_material changes only the pixels of meshes without a material, as bytes against the selection"""
    c = bare
    _uniform(c, MATERIALS[-1])
    _render(c, native)
    with pytest.raises(RuntimeError, match="ran without mesh materials"):
        c.frame_mesh_ids(W * H)
    c.set_mesh_material(0, MATERIALS[0])
    _render(c, native)
    with pytest.raises(RuntimeError, match="n_pixels"):
        c.frame_mesh_ids(W * H - 1)
    c.clear_meshes()
    for tris, center in mm.scene():
        c.add_mesh(tris, center)
    assert c.mesh_material(0) is None and c.mesh_material(1) is None
    assert _same(_render(c, native), fused[-1])
    with pytest.raises(RuntimeError, match="ran without mesh materials"):
        c.frame_mesh_ids(W * H)
    # the floor owns FLOOR; the context's options then become PLATE: the plate's pixels and the pixels without a triangle follow, the floor's do not
    c.set_mesh_material(0, MATERIALS[0])
    c.set_geometry_opts(sun_dir=mm.SUN, up_dir=UP, **MATERIALS[1])
    got = _render(c, native)
    ids = c.frame_mesh_ids(W * H).reshape(H, W)
    want = np.where((ids == 0)[..., None], fused[0][0], fused[1][0])
    assert ids.tobytes() == fused["ids"].tobytes() and got[0].tobytes() == want.tobytes() and got[1].tobytes() == fused[-1][1].tobytes()
    assert c.mesh_material(0)["metallic"] == float(np.float32(0.9))


# -------------------------------------------------------------------------------------------------------------------- 8 bindings
# for the command line's level default camera at z = 2 (test_mesh_reflection_meshes_gpu.py's): the floor raised to just under the object's base
# plate, and a wall across the far side of the floor that faces the camera and the default sun
LEVEL_SCENE = [(hc.scene("A")[0][0], (0.0, -0.405, 0.0)), ((mc.cube().astype(np.float64) * np.array([1.0, 1.0, 0.04])).astype(np.float32), (0.0, 0.1, -0.95))]


def _write_scene(tmp_path, c, meshes=None, name="m"):
    mi = pkg("meshio")
    entries = []
    for i, (tris, center) in enumerate(meshes or mm.scene()):
        mi.save_obj(str(tmp_path / ("%s%d.obj" % (name, i))), tris)
        mat = {k: (list(v) if isinstance(v, tuple) else v) for k, v in MATERIALS[i].items()}
        entries.append({"center": [float(x) for x in center], "path": "%s%d.obj" % (name, i), "type": "Mesh", "material": mat})
    c.save_snapshot_file(str(tmp_path / "unit.ingp"))
    entries.append({"center": [0, 0, 0], "path": "unit.ingp", "type": "Nerf"})
    path = tmp_path / ("%s_geometry_scene.json" % name)
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def test_scene_file_pyngp_and_command_line(tmp_path, hybrid, native, clean):
    """one scene file with materials: native's load_scene, pyngp's Testbed and the command line render the same frame; set_mesh_material and
    clear_mesh_material of the Testbed act, and what the Testbed set comes back after load_training_data"""
    from PIL import Image

    scene = _write_scene(tmp_path, hybrid)
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts(sun_dir=mm.SUN, up_dir=UP)
        want = _render(c, native)
        assert c.mesh_material(0)["roughness"] == float(np.float32(0.2)) and (c.frame_mesh_ids(W * H) == 1).sum() >= mm.MIN_CLASS
        _per_mesh(hybrid, {**MATERIALS, -1: {}})
        assert _same(_render(hybrid, native), want)
        c.set_mesh_material(1, None)
        without_plate = _render(c, native)
    finally:
        c.close()
    pyngp = pkg("build").import_pyngp()

    level = _write_scene(tmp_path, hybrid, LEVEL_SCENE, "level")

    def testbed(camera=True):
        tb = pyngp.Testbed()
        tb.load_training_data(scene if camera else level)
        assert tb.mode == pyngp.TestbedMode.Geometry
        tb.background_color = [0.0, 0.0, 0.0, 0.0]
        tb.render_mode = pyngp.RenderMode.Shade
        if camera:
            tb.snap_to_pixel_centers = True
            tb.sun_dir = [float(x) for x in mm.SUN]
            tb.up_dir = [float(x) for x in UP]
            tb.fov_axis = 0
            tb.relative_focal_length = [mm.FOCAL[0] / W, mm.FOCAL[1] / W]
            tb.camera_matrix = mm.CAMERA
        return tb

    tb = testbed()
    assert tb.render(W, H, 1, True).tobytes() == want[0].tobytes()
    assert abs(tb.mesh_material(1).specular - 0.5) < 1e-7 and tb.mesh_material(0).roughness == np.float32(0.2)
    tb.clear_mesh_material(1)
    assert tb.mesh_material(1) is None and tb.render(W, H, 1, True).tobytes() == without_plate[0].tobytes()
    b = pyngp.Testbed.BRDFParams()
    b.basecolor, b.ambientcolor, b.metallic, b.roughness, b.specular = list(MATERIALS[1]["basecolor"]), list(AMBIENT), 0.0, 0.8, 0.5
    tb.set_mesh_material(1, b)
    assert tb.render(W, H, 1, True).tobytes() == want[0].tobytes()
    b.roughness = 0.3
    tb.set_mesh_material(1, b)
    changed = tb.render(W, H, 1, True)
    assert changed.tobytes() != want[0].tobytes()
    tb.load_training_data(scene)  # the file says 0.8; what the Testbed was given comes back over it
    assert tb.mesh_material(1).roughness == np.float32(0.3) and tb.render(W, H, 1, True).tobytes() == changed.tobytes()
    del tb
    # the command line writes the frame of its default camera: un-premultiplied, sRGB-encoded, 8 bits (pow may round the last bit)
    tb = testbed(camera=False)
    frame = tb.render(W, H, 1, True)
    tb.clear_mesh_material(0)
    tb.clear_mesh_material(1)
    plain = tb.render(W, H, 1, True)
    del tb

    def as_png(f):
        a = np.clip(f[..., 3:4], 0, 1)
        v = np.clip(np.where(a > 0, f[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
        srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
        return np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)

    expect = as_png(frame)
    print("\ncommand line: the materials change %d of %d pixels of the file" % ((expect != as_png(plain)).any(-1).sum(), W * H))
    assert (expect != as_png(plain)).any(-1).sum() > 20
    exe = pkg("build").build_main()
    out = tmp_path / "shot.png"
    res = subprocess.run([exe, "--no-gui", "--scene", level, "--render_mode", "Shade", "--width", str(W), "--height", str(H), "--screenshot", str(out)], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr
    png = np.asarray(Image.open(out)).astype(np.int64)
    assert png.shape == (H, W, 4) and np.abs(png - expect).max() <= 1 and (png != expect).mean() < 0.01, np.abs(png - expect).max()
