"""Mesh albedos without a GPU (include/ngp_hip.h, "mesh albedos"): the cases have both meshes among the rays the GPU tests compare, the
composed reference is the uniform one where every mesh's albedo is the call's and is linear in each mesh's albedo; on a host-only context
the set / get round trip, the lifetime rules, every refusal and the scene file's "albedo"; material_albedo; and the library's exports."""
import json

import numpy as np
import pytest

from conftest import pkg

import irradiance_bounce_reference as br
import irradiance_sun_reference as sr
import mesh_albedo_cases as ma
import mesh_material_cases as mm
from irradiance_volume_cases import GEN_POINTS, UNSAFE_CAP

TRIANGLE = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
REFUSAL = r"mesh albedo must be finite and in \[0, 1\] on every channel"


def _f32(rgb):
    return tuple(float(np.float32(x)) for x in rgb)


# ------------------------------------------------------------------------------------------------------------------ the cases
def test_both_meshes_are_among_the_safe_hits():
    """the bounce stage: (20, 1), (89, 8), (111, 10) and (354, 32) safe hits on the two meshes at K = 15, 64, 81, 256, no unsafe ray at any
    shape, mesh 0 alone at K = 1; the sun stage: (25, 2), (29, 2), (100, 7) lit safe rays at K = 64, 81, 256"""
    for nu, nv in br.RAY_SHAPES:
        c = ma.bounce_case(nu, nv, False)
        hits = [int((c["safe"] & (c["mesh"] == m)).sum()) for m in (0, 1)]
        assert not (~c["safe"]).any() and (~c["safe"]).mean() <= UNSAFE_CAP
        assert np.array_equal(c["mesh"] >= 0, np.isfinite(c["hit"]["t"]))
        if (nu, nv) in ma.BOUNCE_SHAPES:
            assert tuple(hits) == ma.BOUNCE_HITS[nu * nv], (nu, nv, hits)
        else:
            assert (nu, nv) == (1, 1) and hits == [1, 0]
    assert [s for s in br.RAY_SHAPES if s != (1, 1)] == ma.BOUNCE_SHAPES
    for nu, nv in ma.SUN_SHAPES:
        c = ma.sun_case(nu, nv)
        lit = c["safe"] & c["info"]["lit"]
        assert tuple(int((lit & (c["mesh"] == m)).sum()) for m in (0, 1)) == ma.SUN_LIT[nu * nv], (nu, nv)
        assert (~c["safe"]).mean() <= UNSAFE_CAP and (nu, nv) in br.RAY_SHAPES


def test_the_end_to_end_lattice_hits_both_meshes():
    """12 probes x 64 rays of E2E_CASE: 122 floor hits, 92 torus hits, 1 unsafe ray of 768"""
    hit, mesh = ma.e2e_hits()
    assert mesh.shape == (12, 64)
    assert (int((mesh == 0).sum()), int((mesh == 1).sum()), int(hit["unsafe"].sum())) == ma.E2E_HITS
    assert hit["unsafe"].mean() <= UNSAFE_CAP
    assert ((mesh == 1) & ~hit["unsafe"]).any(1).all() and (mesh == 0).any(1).sum() == 10  # (every probe has the torus in sight, ten the floor)


def test_the_albedos_are_far_apart():
    """at K = 64 the composed B differs from the uniform one (STAGE_ALBEDO) by up to 0.43 on mesh 0's rays and 0.85 on mesh 1's: some
    10^4 allowances, so a build that ignores the meshes' albedos cannot pass"""
    for visible in (False, True):
        c = ma.bounce_case(8, 8, visible)
        d = np.abs(c["B"] - c["uniform"]["B"]).max(-1)
        far = [float(d[c["safe"] & (c["mesh"] == m)].max()) for m in (0, 1)]
        print("\nK = 64 %s: composed against uniform %.3f, %.3f; allowance %.2e" % ("visible" if visible else "plain", far[0], far[1], c["allow"]))
        assert min(far) > 1000 * c["allow"]
        if not visible:
            assert abs(far[0] - 0.43) < 0.005 and abs(far[1] - 0.85) < 0.005 and abs(c["allow"] - 5.0e-5) < 0.05e-5
        assert np.all(d[c["mesh"] < 0] == 0)
    c = ma.sun_case(8, 8)
    d = np.abs(c["B"] - c["uniform"]["B"]).max(-1)
    lit = c["safe"] & c["info"]["lit"]
    assert min(float(d[lit & (c["mesh"] == m)].max()) for m in (0, 1)) > 1000 * c["allow"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_composed_with_the_calls_albedo_is_the_uniform_reference(dtype):
    """every A_m = the call's albedo: the composed B is the uniform reference's, value by value, in float64 and in the float32 form"""
    same = (br.STAGE_ALBEDO, br.STAGE_ALBEDO)
    key = "B" if dtype == np.float64 else "B32"
    for nu, nv in ((3, 5), (8, 8)):
        for visible in (False, True):
            c = ma.bounce_case(nu, nv, visible, same)
            assert np.array_equal(c[key], c["uniform"][key])
    c = ma.sun_case(8, 8, same)
    assert np.array_equal(c[key], c["uniform"][key]) and np.abs(c[key]).max() > 1e-2


def test_composed_is_linear_in_each_meshes_albedo():
    """B(s A, A_1) - B(0, A_1) = s (B(A, A_1) - B(0, A_1)), and likewise in mesh 1's albedo with mesh 0's held: float64, to rounding"""
    zero = np.float32([0, 0, 0])
    nu, nv = 8, 8
    for make in (lambda al: ma.bounce_case(nu, nv, True, al)["B"], lambda al: ma.sun_case(nu, nv, al)["B"]):
        for m in (0, 1):
            def at(a):
                return make((a, ma.A1) if m == 0 else (ma.A0, a))

            base, full, half = at(zero), at(ma.ALBEDOS[m]), at(np.float32(0.5) * ma.ALBEDOS[m])
            assert np.abs(full - base).max() > 1e-2
            assert np.abs((half - base) - 0.5 * (full - base)).max() <= 1e-12 * np.abs(full).max()
            mesh = ma.bounce_case(nu, nv, True)["mesh"]
            assert np.array_equal(full[mesh != m], base[mesh != m])  # (the other mesh's rays do not move at all)


# ------------------------------------------------------------------------------------------------------ the host-only context
@pytest.fixture()
def host(native):
    c = native.Context(-1)
    c.add_mesh(TRIANGLE, (0.0, 0.0, 0.0))
    c.add_mesh(TRIANGLE, (1.0, 0.0, 0.0))
    yield c
    c.close()


def test_set_get_round_trip(host, native):
    import ctypes as C

    assert host.mesh_albedo(0) is None and host.mesh_albedo(1) is None
    host.set_mesh_albedo(1, ma.A1)
    assert host.mesh_albedo(1) == _f32(ma.A1) and host.mesh_albedo(0) is None
    host.set_mesh_albedo(0, 0.25)  # (one number: all three channels)
    assert host.mesh_albedo(0) == (0.25, 0.25, 0.25)
    for edge in ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 1.0, 0.5)):
        host.set_mesh_albedo(0, edge)
        assert host.mesh_albedo(0) == edge
    host.set_mesh_albedo(1, None)
    assert host.mesh_albedo(1) is None
    # ngp_get_mesh_albedo hands out zeros and own = 0 for a mesh without one, and takes NULL for either output
    lib = native.load_library()
    out, own = (C.c_float * 3)(7, 7, 7), C.c_int(7)
    assert lib.ngp_get_mesh_albedo(host.h, 1, C.byref(out), C.byref(own)) == 0
    assert own.value == 0 and tuple(out) == (0.0, 0.0, 0.0)
    assert lib.ngp_get_mesh_albedo(host.h, 0, None, C.byref(own)) == 0 and own.value == 1
    assert lib.ngp_get_mesh_albedo(host.h, 0, C.byref(out), None) == 0 and tuple(out) == (0.0, 1.0, 0.5)


def test_lifetime_rules(host, tmp_path):
    """ngp_clear_meshes and ngp_load_scene drop every albedo; an added mesh has none; ngp_set_geometry_opts and ngp_set_mesh_material never
    touch one, and ngp_set_mesh_albedo never touches a material"""
    host.set_mesh_albedo(0, ma.A0)
    host.set_geometry_opts(metallic=0.7, basecolor=(0.1, 0.2, 0.3))
    host.set_mesh_material(0, mm.FLOOR)
    host.set_mesh_material(1, mm.PLATE)
    assert host.mesh_albedo(0) == _f32(ma.A0) and host.mesh_albedo(1) is None
    host.set_mesh_material(0, None)
    assert host.mesh_albedo(0) == _f32(ma.A0)
    before = host.mesh_material(1)
    host.set_mesh_albedo(1, ma.A1)
    host.set_mesh_albedo(1, None)
    assert host.mesh_material(1) == before and host.mesh_material(0) is None
    host.add_mesh(TRIANGLE, (2.0, 0.0, 0.0))
    assert host.mesh_albedo(2) is None and host.mesh_albedo(0) == _f32(ma.A0)
    host.clear_meshes()
    host.add_mesh(TRIANGLE, (0.0, 0.0, 0.0))
    assert host.mesh_albedo(0) is None
    host.set_mesh_albedo(0, ma.A0)
    host.load_scene(_scene(tmp_path, [_mesh()]))
    assert host.n_meshes() == 1 and host.mesh_albedo(0) is None


def test_refusals_leave_the_state_alone(host):
    host.set_mesh_albedo(0, ma.A0)
    for bad in (-1, 2, 100):
        with pytest.raises(RuntimeError, match="mesh: index"):
            host.set_mesh_albedo(bad, ma.A1)
        with pytest.raises(RuntimeError, match="mesh: index"):
            host.set_mesh_albedo(bad, None)
        with pytest.raises(RuntimeError, match="mesh: index"):
            host.mesh_albedo(bad)
    for value in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01, 2.0):
        for i in range(3):
            rgb = [0.5, 0.5, 0.5]
            rgb[i] = value
            for mesh in (0, 1):
                with pytest.raises(RuntimeError, match=REFUSAL):
                    host.set_mesh_albedo(mesh, rgb)
    assert host.mesh_albedo(0) == _f32(ma.A0) and host.mesh_albedo(1) is None


# ---------------------------------------------------------------------------------------------------------------- scene files
def _scene(tmp_path, entries):
    pkg("meshio").save_obj(str(tmp_path / "t.obj"), TRIANGLE)
    path = tmp_path / "scene.json"
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def _mesh(**kw):
    return dict({"center": [0, 0, 0], "path": "t.obj", "type": "Mesh"}, **kw)


def test_scene_file_albedos(host, tmp_path):
    """a "Mesh" entry's "albedo": three numbers; an entry without one owns none; it stands beside a "material" """
    host.load_scene(_scene(tmp_path, [_mesh(albedo=[0.9, 0.1, 0.1]), _mesh(), _mesh(albedo=[0, 1, 0.5], material=dict(roughness=0.25))]))
    assert host.n_meshes() == 3
    assert host.mesh_albedo(0) == _f32((0.9, 0.1, 0.1)) and host.mesh_albedo(1) is None and host.mesh_albedo(2) == (0.0, 1.0, 0.5)
    assert host.mesh_material(0) is None and host.mesh_material(2)["roughness"] == 0.25


@pytest.mark.parametrize("albedo, message", [
    ([1, 0], "'albedo' must be an array of 3 numbers"),
    ([1, 0, 0, 1], "'albedo' must be an array of 3 numbers"),
    (0.5, "'albedo' must be an array of 3 numbers"),
    ([1, "x", 0], "'albedo' must be an array of 3 numbers"),
    ({"r": 1}, "'albedo' must be an array of 3 numbers"),
    ([0.5, 1.5, 0.5], REFUSAL),
    ([-0.1, 0.5, 0.5], REFUSAL),
    ([0.5, 0.5, 1e39], REFUSAL),
])
def test_scene_file_refusals(albedo, message, host, tmp_path):
    """each refusal names what it refuses (and the entry) and leaves the scene and its albedos as they were"""
    host.set_mesh_albedo(0, ma.A0)
    with pytest.raises(RuntimeError, match=r"geometry\[1\]: " + message):
        host.load_scene(_scene(tmp_path, [_mesh(), _mesh(albedo=albedo)]))
    assert host.n_meshes() == 2 and host.mesh_albedo(0) == _f32(ma.A0) and host.mesh_albedo(1) is None


def test_scene_file_refuses_an_albedo_on_a_nerf_entry(host, tmp_path):
    host.set_mesh_albedo(1, ma.A1)
    with pytest.raises(RuntimeError, match="'albedo' applies to a 'Mesh' entry, not to 'Nerf'"):
        host.load_scene(_scene(tmp_path, [_mesh(), {"center": [0, 0, 0], "path": "none.ingp", "type": "Nerf", "albedo": [0.5, 0.5, 0.5]}]))
    assert host.n_meshes() == 2 and host.mesh_albedo(1) == _f32(ma.A1)


# -------------------------------------------------------------------------------------------------------------------- bindings
def test_material_albedo_is_the_shims_rule(native):
    """the base colour squared per channel, clamped to [0, 1], formed in float32: csrc/testbed_shim.h material_albedo"""
    for base in ((0.8, 0.8, 0.8), (0.9, 0.15, 0.1), (1.5, -2.0, 0.0), (1.0, 0.3, 1e-30)):
        b = np.float32(base)
        want = tuple(float(x) for x in np.minimum(np.maximum((b * b).astype(np.float32), np.float32(0)), np.float32(1)))
        got = native.material_albedo(dict(basecolor=base))
        assert got == want and all(0.0 <= x <= 1.0 for x in got), base
    assert native.material_albedo({}) == native.material_albedo(dict(native.MATERIAL_DEFAULTS))
    assert native.material_albedo(dict(roughness=0.1)) == (float(np.float32(0.8) * np.float32(0.8)),) * 3
    assert native.material_albedo(mm.PLATE) == native.material_albedo(dict(basecolor=mm.PLATE["basecolor"]))


def test_library_exports_the_new_symbols(native):
    lib = native.load_library()
    for name in ("ngp_set_mesh_albedo", "ngp_get_mesh_albedo"):
        assert name in native.EXPORTS and hasattr(lib, name), name
