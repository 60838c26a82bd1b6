"""Mesh materials without a GPU (include/ngp_hip.h, "mesh materials"): the case has the pixel classes the GPU tests lean on and the three
materials are far enough apart that a build ignoring them cannot pass; on a host-only context the set / get round trip, the lifetime rules,
every refusal and the scene file's "material" object; and the library's exports."""
import json

import numpy as np
import pytest

from conftest import pkg

import mesh_material_cases as mm

W, H = mm.WIDTH, mm.HEIGHT
TRIANGLE = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
PLATE_F32 = {k: (tuple(float(np.float32(x)) for x in v) if isinstance(v, tuple) else float(np.float32(v))) for k, v in mm.PLATE.items()}


@pytest.fixture(scope="module")
def frame():
    return mm.material_frame()


def test_the_case_has_every_pixel_class(frame):
    """of 64 x 48 pixels the primary ray hits the floor, the plate, or no triangle, each on at least 100; mirror rays are cut from floor pixels
    onto the plate and from plate pixels onto the floor, each at least 100 times; at most 3 % of the pixels and of the hits are flagged"""
    own, hm, cut = frame["owner"], frame["hit_mesh"], frame["cut"]
    sizes = dict(floor=(own == 0).sum(), plate=(own == 1).sum(), none=(own == -1).sum(), floor_onto_plate=(cut & (own == 0) & (hm == 1)).sum(),
                 plate_onto_floor=(cut & (own == 1) & (hm == 0)).sum())
    any_fr = frame["first"][-1]
    owner_unsafe = mm.owner()[1]
    flagged_px = owner_unsafe | any_fr["unsafe"]
    flagged_hits = cut & ((any_fr["owns"] & any_fr["t_unsafe"]) | any_fr["hit_unsafe"])
    print("\nclasses %s; cut rays %d; flagged pixels %d, flagged hits %d" % ({k: int(v) for k, v in sizes.items()}, cut.sum(), flagged_px.sum(), flagged_hits.sum()))
    assert own.size == W * H and sizes["floor"] + sizes["plate"] + sizes["none"] == W * H
    for k, v in sizes.items():
        assert v >= mm.MIN_CLASS, (k, v)
    safe = ~flagged_px  # the owner by reference_rule_hit names a mesh exactly where the restated frame's pixel owns a mirror ray
    assert np.array_equal((own >= 0)[safe], any_fr["owns"][safe]) and np.all(any_fr["covered"][safe & (own >= 0)])
    assert np.all((hm >= 0) == cut)
    assert flagged_px.sum() <= mm.UNSAFE_CAP * W * H and flagged_hits.sum() <= mm.UNSAFE_CAP * max(cut.sum(), 1)


def test_the_materials_are_far_apart(frame):
    """with an ambient of 0.3 every floor pixel of the floor-material frame, and every plate pixel of the plate-material frame, differs from
    the context-material frame by at least 100 frame_bound in some channel; the per-mesh frame takes each pixel from its owner's frame"""
    own = frame["owner"]
    ctx_fr = frame["first"][-1]["rgba"][..., :3]
    ratios = {}
    for k, name in ((0, "floor"), (1, "plate")):
        fr = frame["first"][k]["rgba"][..., :3]
        ratio = (np.abs(fr - ctx_fr) / np.maximum(mm.frame_bound(fr), mm.frame_bound(ctx_fr))).max(-1)
        ratios[name] = float(ratio[own == k].min())
    print("\nsmallest separation in frame_bound: floor %.0f, plate %.0f" % (ratios["floor"], ratios["plate"]))
    assert ratios["floor"] >= mm.MIN_SEPARATION and ratios["plate"] >= mm.MIN_SEPARATION
    for k in mm.MATERIALS:
        assert np.array_equal(frame["rgba"][own == k], frame["uniform"][k]["rgba"][own == k])
    uncut = ~frame["cut"]
    for k in mm.MATERIALS:  # an uncut pixel does not see another mesh's material: the second round changes nothing there
        assert np.array_equal(frame["uniform"][k]["rgba"][uncut], frame["first"][k]["rgba"][uncut])


# ------------------------------------------------------------------------------------------------------ the host-only context
@pytest.fixture()
def host(native):
    c = native.Context(-1)
    c.add_mesh(TRIANGLE, (0.0, 0.0, 0.0))
    c.add_mesh(TRIANGLE, (1.0, 0.0, 0.0))
    yield c
    c.close()


def test_set_get_round_trip(host, native):
    assert host.mesh_material(0) is None and host.mesh_material(1) is None
    host.set_mesh_material(1, mm.PLATE)
    got = host.mesh_material(1)
    assert host.mesh_material(0) is None
    for k, v in dict(native.MATERIAL_DEFAULTS, **PLATE_F32).items():
        assert got[k] == v, k
    host.set_mesh_material(1, None)
    assert host.mesh_material(1) is None
    # ngp_get_mesh_material hands out the context's BRDF fields for a mesh without a material
    import ctypes as C

    host.set_geometry_opts(metallic=0.25, basecolor=(0.1, 0.2, 0.3))
    m, own = native.MeshMaterial(), C.c_int(7)
    assert native.load_library().ngp_get_mesh_material(host.h, 0, C.byref(m), C.byref(own)) == 0
    assert own.value == 0 and m.metallic == 0.25 and tuple(m.basecolor) == tuple(float(np.float32(x)) for x in (0.1, 0.2, 0.3)) and m.specular == 1.0


def test_lifetime_rules(host, tmp_path):
    """ngp_clear_meshes and ngp_load_scene drop every material; an added mesh has none; ngp_set_geometry_opts never touches one"""
    host.set_mesh_material(0, mm.FLOOR)
    host.set_geometry_opts(metallic=0.7, roughness=0.1)
    assert host.mesh_material(0)["metallic"] == float(np.float32(0.9)) and host.mesh_material(1) is None
    host.add_mesh(TRIANGLE, (2.0, 0.0, 0.0))
    assert host.mesh_material(2) is None and host.mesh_material(0) is not None
    host.clear_meshes()
    host.add_mesh(TRIANGLE, (0.0, 0.0, 0.0))
    assert host.mesh_material(0) is None
    host.set_mesh_material(0, mm.FLOOR)
    pkg("meshio").save_obj(str(tmp_path / "t.obj"), TRIANGLE)
    scene = tmp_path / "scene.json"
    scene.write_text(json.dumps({"geometry": [{"center": [0, 0, 0], "path": "t.obj", "type": "Mesh"}]}))
    host.load_scene(str(scene))
    assert host.n_meshes() == 1 and host.mesh_material(0) is None


def test_refusals_leave_the_state_alone(host):
    host.set_mesh_material(0, mm.FLOOR)
    before = host.mesh_material(0)
    for bad in (-1, 2, 100):
        with pytest.raises(RuntimeError, match="mesh: index"):
            host.set_mesh_material(bad, mm.PLATE)
        with pytest.raises(RuntimeError, match="mesh: index"):
            host.mesh_material(bad)
    for key in ("metallic", "subsurface", "specular", "roughness", "sheen", "clearcoat", "clearcoat_gloss"):
        for value in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(RuntimeError, match="'%s' is not finite" % key):
                host.set_mesh_material(0, {key: value})
    for key in ("basecolor", "ambientcolor"):
        for i in range(3):
            colour = [0.5, 0.5, 0.5]
            colour[i] = float("nan")
            with pytest.raises(RuntimeError, match="'%s' is not finite" % key):
                host.set_mesh_material(0, {key: tuple(colour)})
            with pytest.raises(RuntimeError, match="'%s' is not finite" % key):
                host.set_mesh_material(1, {key: tuple(colour)})
    assert host.mesh_material(0) == before and host.mesh_material(1) is None
    with pytest.raises(ValueError, match="unknown key"):
        host.set_mesh_material(0, dict(colour=(1, 0, 0)))


# ---------------------------------------------------------------------------------------------------------------- scene files
def _scene(tmp_path, entries):
    pkg("meshio").save_obj(str(tmp_path / "t.obj"), TRIANGLE)
    path = tmp_path / "scene.json"
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def _mesh(material=None, **kw):
    e = dict({"center": [0, 0, 0], "path": "t.obj", "type": "Mesh"}, **kw)
    if material is not None:
        e["material"] = material
    return e


def test_scene_file_materials_and_defaults(host, native, tmp_path):
    """a "Mesh" entry's "material" object: the keys it gives, the header's defaults for the rest; an entry without one owns none"""
    full = dict(basecolor=[0.9, 0.15, 0.1], ambientcolor=[0.3, 0.2, 0.1], metallic=0.1, subsurface=0.2, specular=0.5, roughness=0.8, sheen=0.3, clearcoat=0.4, clearcoat_gloss=0.6)
    host.load_scene(_scene(tmp_path, [_mesh({}), _mesh(), _mesh(dict(roughness=0.25, basecolor=[0.1, 0.2, 0.3])), _mesh(full)]))
    assert host.n_meshes() == 4 and host.mesh_material(1) is None
    assert host.mesh_material(0) == {k: (tuple(float(np.float32(x)) for x in v) if isinstance(v, tuple) else float(np.float32(v))) for k, v in native.MATERIAL_DEFAULTS.items()}
    third = host.mesh_material(2)
    assert third["roughness"] == 0.25 and third["basecolor"] == tuple(float(np.float32(x)) for x in (0.1, 0.2, 0.3)) and third["specular"] == 1.0 and third["metallic"] == 0.0
    got = host.mesh_material(3)
    for k, v in full.items():
        assert got[k] == (tuple(float(np.float32(x)) for x in v) if isinstance(v, list) else float(np.float32(v))), k


@pytest.mark.parametrize("material, message", [
    (dict(colour=[1, 0, 0]), "unknown material key 'colour'"),
    (dict(metallic="shiny"), "material key 'metallic' must be a number"),
    (dict(roughness=[0.5]), "material key 'roughness' must be a number"),
    (dict(basecolor=[1, 0]), "material key 'basecolor' must be an array of 3 numbers"),
    (dict(ambientcolor=[1, 0, 0, 1]), "material key 'ambientcolor' must be an array of 3 numbers"),
    (dict(basecolor=0.5), "material key 'basecolor' must be an array of 3 numbers"),
    (dict(basecolor=[1, "x", 0]), "material key 'basecolor' must be an array of 3 numbers"),
    ([0.5], "'material' must be an object"),
])
def test_scene_file_refusals(material, message, host, tmp_path):
    """each refusal names what it refuses and leaves the scene and its materials as they were"""
    host.set_mesh_material(0, mm.FLOOR)
    before = host.mesh_material(0)
    with pytest.raises(RuntimeError, match=message):
        host.load_scene(_scene(tmp_path, [_mesh(), _mesh(material)]))
    assert host.n_meshes() == 2 and host.mesh_material(0) == before


def test_scene_file_refuses_a_material_on_a_nerf_entry(host, tmp_path):
    with pytest.raises(RuntimeError, match="'material' applies to a 'Mesh' entry, not to 'Nerf'"):
        host.load_scene(_scene(tmp_path, [_mesh(), {"center": [0, 0, 0], "path": "none.ingp", "type": "Nerf", "material": {}}]))
    assert host.n_meshes() == 2


def test_library_exports_the_new_symbols(native):
    lib = native.load_library()
    for name in ("ngp_set_mesh_material", "ngp_get_mesh_material", "ngp_get_frame_mesh_ids"):
        assert name in native.EXPORTS and hasattr(lib, name), name
