"""The oracle's mesh path (BVH4 traversal, mesh selection, shadow ray, BRDF) and the BVH builder against the float64 brute force of
mesh_reference.py, on the meshes, rays and frames of mesh_cases.py. No GPU.

On every safe ray hit / miss must agree; the share of unsafe rays of every class, and of unsafe pixels of every frame, is capped at 2 %.
The deviations measured here (printed; run with -s) are what the GPU tolerances in mesh_cases.py derive from, and each test fails if its
measurement exceeds the value recorded there.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import pkg

import mesh_cases as mc
import mesh_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _sorted_rows(T):
    r = np.asarray(T, np.float32).reshape(-1, 9)
    return r[np.lexsort(r.T[::-1])]


@pytest.fixture(scope="module")
def host_ctx(native):
    c = native.Context(-1)
    yield c
    c.close()


@pytest.mark.parametrize("name", mc.MESH_NAMES)
def test_normalise_equals_the_loader(name, host_ctx):
    tris, center, _ = mc.meshes()[name]
    host_ctx.clear_meshes()
    host_ctx.add_mesh(tris, center)
    _, built = host_ctx.mesh_bvh(0)
    mine = ref.normalise(tris, center)
    theirs = np.stack([built["a"], built["b"], built["c"]], 1)
    assert np.array_equal(_sorted_rows(mine), _sorted_rows(theirs))
    lo, hi = host_ctx.mesh_info(0)["aabb"]
    assert np.array_equal(lo, ref.mesh_box(mine)[0]) and np.array_equal(hi, ref.mesh_box(mine)[1])
    host_ctx.clear_meshes()


@pytest.mark.parametrize("name", mc.MESH_NAMES)
def test_oracle_trace_matches_brute_force(name, oracle):
    tris, center, convex = mc.meshes()[name]
    T = ref.normalise(tris, center)
    h = oracle.mesh_scene([(tris, center)])
    report = []
    for cls, (o, d, expect) in mc.ray_classes(name, T, convex).items():
        p, n = oracle.trace_mesh(h, o, d)
        dt, dn = mc.compare_trace(name, cls, o, d, expect, p, n, [T], report)[:2]
        assert dt <= mc.ORACLE_DEV_POS[name, cls] and dn <= mc.ORACLE_DEV_NORMAL, (cls, dt, dn, report[-1])
    oracle.mesh_scene_destroy(h)
    print("\n" + "\n".join(report))


def test_oracle_follows_the_reference_rule_on_overlapping_boxes(oracle):
    scene = mc.overlap_scene()
    Ts = mc.normalised(scene)
    (lo0, hi0), (lo1, hi1) = ref.mesh_box(Ts[0]), ref.mesh_box(Ts[1])
    overlap = np.prod(np.maximum(np.minimum(hi0, hi1) - np.maximum(lo0, lo1), 0)) / np.prod(hi0 - lo0)
    assert 0.3 < overlap < 0.7  # the icosphere's box covers about half of the torus's
    o, d = mc.overlap_rays(Ts)
    h = oracle.mesh_scene(scene)
    p, n = oracle.trace_mesh(h, o, d)
    oracle.mesh_scene_destroy(h)
    report = []
    dt, dn = mc.compare_trace("overlap", "random", o, d, None, p, n, Ts, report)[:2]
    print("\n" + report[0])
    assert dt <= mc.ORACLE_DEV_OVERLAP and dn <= mc.ORACLE_DEV_NORMAL
    # the scene tells the reference's rule from the true nearest hit
    t_rule, _, _, _, unsafe, _ = ref.reference_rule_hit(Ts, o, d)
    t_all, unsafe_all = ref.global_nearest(Ts, o, d)
    finite = lambda t: np.where(np.isfinite(t), t, 0.0)
    differ = ~unsafe & ~unsafe_all & ((np.isfinite(t_rule) != np.isfinite(t_all)) | (np.abs(finite(t_rule) - finite(t_all)) > 1e-3))
    print("rays on which the rule and the nearest hit differ: %d of %d" % (differ.sum(), o.shape[0]))
    assert differ.sum() >= 50


@pytest.mark.parametrize("name", list(mc.FRAMES))
def test_oracle_render_matches_reference(name, oracle):
    fr = mc.reference_frame(name)
    share = fr["unsafe"].mean()
    assert share <= mc.UNSAFE_CAP, (name, share)
    h = oracle.mesh_scene(mc.render_scene())
    fb, db = oracle.render_mesh(h, oracle.make_camera(mc.camera_matrix(name), mc.WIDTH, mc.HEIGHT, mc.focal(name)), oracle.make_mesh_opts(**mc.FRAMES[name]))
    oracle.mesh_scene_destroy(h)
    dd, dc = mc.compare_frame(name, fr, fb, db)
    print("\n%-15s covered %4d  shadowed %4d  lit %4d  lit faces in shadow %4d  unsafe %5.2f %%  ddepth %.2e  drgb/max(1,|rgb|) %.2e  max rgb %.3g"
          % (name, fr["covered"].sum(), fr["shadowed"].sum(), fr["lit"].sum(), fr["occluded"].sum(), 100 * share, dd, dc, fr["rgba"][..., :3].max()))
    assert dd <= mc.ORACLE_DEV_FRAME[name][0] and dc <= mc.ORACLE_DEV_FRAME[name][1], (dd, dc)
    mc.check_frame_reaches_its_branch(name, fr)


def test_bvh_depth_fits_the_traversal_stack(host_ctx, tmp_path):
    """With the deepest leaf at depth D (root 0) the traversal's stack holds at most 3 D + 1 nodes: a pop pushes at most 4. The kernel's stack
    has 32 entries, so D <= 10; the builder's median split reaches D only beyond 8 * 4^(D - 1) triangles. This checks the formula on the
    BVHs that are built here; the builder's refusal of a deeper one is test_builder_refuses_a_bvh_deeper_than_its_limit."""
    depths = {}
    for name in mc.MESH_NAMES:
        tris, center, _ = mc.meshes()[name]
        host_ctx.clear_meshes()
        host_ctx.add_mesh(tris, center)
        nodes, _ = host_ctx.mesh_bvh(0)
        depths[name] = (tris.shape[0], mc.bvh_depth(nodes))
    g = np.load(os.path.join(GOLDEN, "mesh_bunny_v1.npz"))
    host_ctx.clear_meshes()
    host_ctx.add_mesh(g["verts"][g["faces"]].astype(np.float32))
    nodes, _ = host_ctx.mesh_bvh(0)
    depths["bunny"] = (g["faces"].shape[0], mc.bvh_depth(nodes))
    host_ctx.clear_meshes()
    print("\n" + "  ".join("%s: %d triangles, depth %d" % (k, n, d) for k, (n, d) in depths.items()))
    for name, (n, depth) in depths.items():
        assert 3 * depth + 1 <= 32, name
        want = 1
        while 8 * 4 ** want < n:
            want += 1
        assert depth == want, (name, n, depth)  # the median split: depth D holds up to 8 * 4^D triangles
    assert depths["triangle"][1] == 1 and depths["fan8"][1] == 1 and depths["fan9"][1] == 1 and depths["fan33"][1] == 2


def test_builder_refuses_a_bvh_deeper_than_its_limit(tmp_path):
    """build_bvh4 with the depth limit lowered to 1 .. 4 and leaves of 1, 3 and 8 triangles: leaf * 4^D triangles build, with the deepest leaf
    at depth D and every triangle in one leaf; one triangle more is refused with an error that names the limit. The limit's default is what
    the traversal's stack covers: 3 D + 1 <= 32 < 3 (D + 1) + 1 (tests/aux/bvh4_depth_check.cpp, host only)."""
    exe = tmp_path / "bvh4_depth_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, pkg("build").CSRC),
                           "-o", str(exe), os.path.join(ROOT, "tests", "aux", "bvh4_depth_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr
