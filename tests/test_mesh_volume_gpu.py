"""ShadeIrradianceVolume on the GPU: the mesh pass whose ambient light is max(E(p, N), 0) / pi from the SH9 irradiance volume, against the
float64 frames of mesh_volume_cases.py (whose docstring derives the per-pixel colour bound), and through every layer: sharding, several
devices, the hybrid NeRF + mesh frame, the other modes, the refusals, pyngp and the command line."""
import json
import os

import numpy as np
import pytest

from conftest import pkg

import irradiance_sh_reference as sh_ref
import mesh_cases as mc
import mesh_reference as ref
import mesh_volume_cases as mv

pytestmark = pytest.mark.gpu

REFUSAL = "ngp_compute_irradiance_volume or ngp_set_irradiance_volume"


@pytest.fixture(scope="module")
def ctx(gpu_ctx, native):
    """meshes only, a context of this module's own"""
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF and the render scene's meshes"""
    c = native.Context(0)
    c.set_model(scene_unit)
    _load(c, mc.render_scene())
    yield c
    c.close()


def _load(c, scene):
    c.clear_meshes()
    for tris, center in scene:
        c.add_mesh(tris, center)


def _opts(native, mode=None, **kw):
    return native.make_opts(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0), render_mode=native.RENDER_SHADE_IRRADIANCE_VOLUME if mode is None else mode, **kw)


def _camera(native, name="defaults", w=mc.WIDTH, h=mc.HEIGHT):
    return native.make_camera(mc.camera_matrix(name), w, h, mc.focal(name))


def _set(c, sh, res, lo, hi):
    c.set_irradiance_volume(mv.as_grid(sh, res), (lo, hi))


def _sky_tolerance(name):
    return mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME[name][1] + 256 * mv.ULP * mv.sky_scale() / np.pi


@pytest.mark.parametrize("name", ["ambient_x", "sun_down"])
def test_sky_volume_is_the_shade_frame(name, ctx, native):
    """the volume that holds the frame's own sky term (ambientcolor (0.3, 0.2, 0.1); up x for ambient_x, y for sun_down), and no ambient
    colour: the existing reference frame"""
    fr = mc.reference_frame(name)
    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts(**dict(mc.FRAMES[name], ambientcolor=(0.0, 0.0, 0.0), up_dir=(0.0, 1.0, 0.0)))
    _set(ctx, *mv.sky_volume(mc.FRAMES[name].get("up_dir", (0.0, 1.0, 0.0))))
    img, depth = ctx.render(_camera(native, name), _opts(native), want_depth=True)
    ctx.set_geometry_opts()
    ctx.clear_irradiance_volume()
    ctx.clear_meshes()
    dd, dc = mc.compare_frame(name, fr, img, depth)
    print("\n%-10s ddepth %.2e  drgb/max(1,|rgb|) %.2e  (allowed %.2e, of which the lookup %.2e)" % (name, dd, dc, _sky_tolerance(name), 256 * mv.ULP * mv.sky_scale() / np.pi))
    assert dd <= mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME[name][0] and dc <= _sky_tolerance(name), (dd, dc)
    mc.check_frame_reaches_its_branch(name, fr)


@pytest.mark.parametrize("metallic", [0.0, 1.0])
def test_varying_volume_matches_reference(metallic, ctx, native):
    fr = mv.varying_frame(metallic)
    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts(metallic=metallic)
    _set(ctx, *mv.varying_volume())
    img, depth = ctx.render(_camera(native), _opts(native), want_depth=True)
    ctx.set_geometry_opts()
    ctx.clear_irradiance_volume()
    ctx.clear_meshes()
    dd, ratio, n = mv.check_volume_frame(fr, img, depth)
    print("\nmetallic %g: safe covered pixels %d, ddepth %.2e, largest colour deviation / bound %.3f" % (metallic, n, dd, ratio))
    assert dd <= mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][0] and ratio <= 1.0, (dd, ratio)


def test_traced_volume_end_to_end(ctx, hybrid, native):
    """trace a volume in the NeRF, read it back, and hold the frame lit by it to the reference fed the same records. With the meshes
    occluding the records are all zero in this scene (the cube mesh is the unit NeRF's own box: no ray reaches it), so the same is done
    with the occlusion off, where the probes near the NeRF see it."""
    _traced_volume(ctx, hybrid, native, True)
    _traced_volume(ctx, hybrid, native, False)


def _traced_volume(ctx, hybrid, native, occlude):
    lo, hi = mv.volume_box()
    res = (3, 3, 3)
    hybrid.compute_irradiance_volume(res, (lo, hi), 8, 8, occlude_by_meshes=occlude)
    d, grid = hybrid.get_irradiance_volume()
    hybrid.clear_irradiance_volume()
    assert tuple(d.res) == res and grid.shape == (3, 3, 3, 28)
    sh = grid.reshape(-1, 28)
    assert occlude or np.abs(sh[:, :27]).max() > 1e-3, "the probes saw nothing"
    fr = mv.volume_frame(mc.normalised(mc.render_scene()), "defaults", sh, res, lo, hi)
    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts()
    ctx.set_irradiance_volume(grid, (lo, hi))
    img, depth = ctx.render(_camera(native), _opts(native), want_depth=True)
    ctx.clear_irradiance_volume()
    ctx.clear_meshes()
    dd, ratio, n = mv.check_volume_frame(fr, img, depth)
    print("\ntraced 3x3x3 volume, meshes occluding: %s, largest |c| %.3g, dead probes %d, safe covered pixels %d, unsafe %.2f %%, ddepth %.2e, largest colour deviation / bound %.3f"
          % (occlude, np.abs(sh[:, :27]).max(), (sh[:, 27] == 0).sum(), n, 100 * fr["unsafe_volume"].mean(), dd, ratio))
    assert dd <= mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][0] and ratio <= 1.0, (dd, ratio)
    if n < 100:
        pytest.skip("the traced volume leaves %d safe covered pixels (fewer than 100): the cap on the unsafe share is not applied" % n)
    assert fr["unsafe_volume"].mean() <= mc.UNSAFE_CAP, fr["unsafe_volume"].mean()


def test_all_probes_dead_is_no_ambient(ctx, native):
    fr = mc.reference_frame("defaults")
    sh, res, lo, hi = mv.varying_volume()
    sh = sh.copy()
    sh[:, 27] = 0
    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts()
    _set(ctx, sh, res, lo, hi)
    img, depth = ctx.render(_camera(native), _opts(native), want_depth=True)
    ctx.clear_irradiance_volume()
    ctx.clear_meshes()
    dd, dc = mc.compare_frame("defaults", fr, img, depth)
    assert dd <= mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][0] and dc <= mc.GPU_FACTOR * mc.ORACLE_DEV_FRAME["defaults"][1], (dd, dc)


def _tiles(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // 8) * ((w + 7) // 8) + xs // 8, (xs % 8) + 8 * (ys % 8)


def test_tile_sharding_covers_frame(ctx, native):
    """the procedure of test_mesh_pass_tile_sharding_covers_frame in the new mode"""
    import torch

    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts()
    _set(ctx, *mv.varying_volume())
    w, h, world = 60, 36, 3
    cam = _camera(native, w=w, h=h)
    full, full_depth = ctx.render(cam, _opts(native), want_depth=True)
    assert (full[..., 3] == 1).sum() > 500
    tile, slot = _tiles(w, h)
    total, total_depth = np.zeros_like(full), np.zeros_like(full_depth)
    packed, packed_depth = np.zeros_like(full), np.zeros_like(full_depth)
    for r in range(world):
        mine = tile % world == r
        part, part_depth = ctx.render(cam, _opts(native, shard_index=r, shard_count=world), want_depth=True)
        assert not np.any(part[~mine])
        total[mine], total_depth[mine] = part[mine], part_depth[mine]
        n = native.load_library().ngp_packed_tiles(w, h, r, world) * 64
        rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
        ctx.render_device(cam, _opts(native, shard_index=r, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
        ctx.render_stats()  # synchronises the context's stream
        src = (tile // world) * 64 + slot
        packed[mine], packed_depth[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]]
    ctx.clear_irradiance_volume()
    ctx.clear_meshes()
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes()


def test_multi_device_replicas_follow_the_volume(ctx, native):
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        for c in (ctx, multi):
            _load(c, mc.render_scene())
            c.set_geometry_opts()
        cam = _camera(native)
        sh, res, lo, hi = mv.varying_volume()
        frames = []
        for records in (sh, (0.5 * sh[::-1]).astype(np.float32)):  # (other records: other probes dead, too)
            for c in (ctx, multi):
                _set(c, records, res, lo, hi)
            one, one_depth = ctx.render(cam, _opts(native), want_depth=True)
            two, two_depth = multi.render(cam, _opts(native), want_depth=True)
            assert (one[..., 3] == 1).sum() > 500
            assert one.tobytes() == two.tobytes() and one_depth.tobytes() == two_depth.tobytes()
            frames.append(one)
        assert frames[0].tobytes() != frames[1].tobytes()
        for c in (ctx, multi):
            c.clear_irradiance_volume()
            with pytest.raises(RuntimeError, match=REFUSAL):
                c.render(cam, _opts(native))
    finally:
        multi.close()
        ctx.clear_irradiance_volume()
        ctx.clear_meshes()


def test_hybrid_multi_sample_frame(ctx, hybrid, native):
    """NeRF and meshes, two samples a pixel, the sky volume: the Shade frame of the same ambient colour. Pixels no sample of the mesh pass
    covers (alpha 0 in the meshes-only frame) are the same bytes; the others differ by what test_sky_volume_is_the_shade_frame allows."""
    cam = _camera(native)
    _load(ctx, mc.render_scene())
    ctx.set_geometry_opts()
    meshes_only = ctx.render(cam, _opts(native, mode=native.RENDER_SHADE, spp=2))
    ctx.clear_meshes()
    hybrid.set_geometry_opts(ambientcolor=mv.SKY_AMBIENT, up_dir=(1.0, 0.0, 0.0))
    shade = hybrid.render(cam, _opts(native, mode=native.RENDER_SHADE, spp=2))
    hybrid.set_geometry_opts()
    _set(hybrid, *mv.sky_volume())
    vol = hybrid.render(cam, _opts(native, spp=2))
    hybrid.clear_irradiance_volume()
    covered = meshes_only[..., 3] > 0
    assert covered.sum() > 500 and (~covered).sum() > 50
    assert vol[~covered].tobytes() == shade[~covered].tobytes()
    assert np.abs(vol - meshes_only).max() > 1e-3  # (the NeRF is in the frame)
    diff = np.abs(vol[..., :3][covered].astype(np.float64) - shade[..., :3][covered]) / np.maximum(1.0, np.abs(shade[..., :3][covered]))
    print("\nhybrid, 2 spp: covered %d, largest difference %.2e (allowed %.2e)" % (covered.sum(), diff.max(), _sky_tolerance("ambient_x")))
    assert diff.max() <= _sky_tolerance("ambient_x")
    assert np.array_equal(vol[..., 3], shade[..., 3])


def test_other_modes_do_not_see_the_volume(hybrid, native):
    cam = _camera(native)
    hybrid.set_geometry_opts(ambientcolor=mv.SKY_AMBIENT)
    hybrid.compute_envmap_grid(2, 2, 16, 8)
    modes = (native.RENDER_SHADE, native.RENDER_SHADE_GRID_ENVMAP)
    _set(hybrid, *mv.varying_volume())
    with_volume = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
    hybrid.clear_irradiance_volume()
    without = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
    hybrid.set_geometry_opts()
    for (a, ad), (b, bd) in zip(with_volume, without):
        assert (a[..., 3] > 0).sum() > 500 and a.tobytes() == b.tobytes() and ad.tobytes() == bd.tobytes()
    assert with_volume[0][0].tobytes() != with_volume[1][0].tobytes()


def test_refusals_and_plain_shade(ctx, hybrid, native, scene_mod, scene_unit):
    cam = _camera(native)
    _load(ctx, mc.render_scene())
    with pytest.raises(RuntimeError, match="render_mode ShadeIrradianceVolume needs " + REFUSAL + " first"):
        ctx.render(cam, _opts(native))
    ctx.clear_meshes()
    with pytest.raises(RuntimeError, match=REFUSAL):
        hybrid.render(cam, _opts(native))
    # NeRF mode: Shade, with or without a volume
    nerf_cam = native.make_camera(scene_mod.orbit_camera(45.0), mc.WIDTH, mc.HEIGHT, scene_mod.focal_from_fov_x(mc.WIDTH, 0.6911))
    shade = hybrid.render(nerf_cam, native.make_opts())
    assert hybrid.render(nerf_cam, native.make_opts(render_mode=native.RENDER_SHADE_IRRADIANCE_VOLUME)).tobytes() == shade.tobytes() and shade[..., 3].max() > 0.5
    # Geometry mode without meshes: Shade, no volume asked for
    bare = native.Context(0)
    try:
        bare.set_model(scene_unit)
        a = bare.render(nerf_cam, _opts(native, mode=native.RENDER_SHADE))
        assert bare.render(nerf_cam, _opts(native)).tobytes() == a.tobytes() and a[..., 3].max() > 0.5
    finally:
        bare.close()
    with pytest.raises(RuntimeError, match="render modes implemented"):
        hybrid.render(nerf_cam, native.make_opts(render_mode=9))


def _write_geometry_scene(tmp_path, hybrid):
    """the render scene's meshes as .obj files, the unit NeRF as a snapshot, and the scene file that names them"""
    mi = pkg("meshio")
    entries = []
    for i, (tris, center) in enumerate(mc.render_scene()):
        mi.save_obj(str(tmp_path / ("mesh%d.obj" % i)), tris)
        entries.append({"center": [float(x) for x in center], "path": "mesh%d.obj" % i, "type": "Mesh"})
    hybrid.save_snapshot_file(str(tmp_path / "unit.ingp"))
    entries.append({"center": [0, 0, 0], "path": "unit.ingp", "type": "Nerf"})
    path = tmp_path / "geometry_scene.json"
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def _testbed(pyngp, scene):
    tb = pyngp.Testbed()
    tb.load_training_data(scene)
    assert tb.mode == pyngp.TestbedMode.Geometry
    tb.background_color = [0.0, 0.0, 0.0, 0.0]
    tb.render_mode = pyngp.RenderMode.ShadeIrradianceVolume
    return tb


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    import subprocess
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    assert int(pyngp.RenderMode.ShadeIrradianceVolume) == 13 and int(pyngp.RenderMode.ShadeGridEnvMap) == 4  # appended behind EncodingVis (12): the reference's values stay put
    scene = _write_geometry_scene(tmp_path, hybrid)
    w, h = mc.WIDTH, mc.HEIGHT
    # an explicit volume: the native frame of the records read back
    tb = _testbed(pyngp, scene)
    tb.snap_to_pixel_centers = True
    tb.sun_dir = [1.0, 1.0, 1.0]
    tb.fov_axis = 0
    tb.relative_focal_length = [mc.focal()[0] / w, mc.focal()[1] / w]  # (100 / 64: exact)
    tb.camera_matrix = mc.camera_matrix()
    vol = tb.compute_irradiance_volume([3, 3, 3], None, 8, 8, True)
    frame = tb.render(w, h, 1, True)
    again = tb.get_irradiance_volume()
    assert np.array_equal(again["sh"], vol["sh"]) and np.array_equal(np.float32(again["aabb"]), np.float32(vol["aabb"]))  # the caller's volume is not replaced
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        c.set_irradiance_volume(vol["sh"], (np.float32(vol["aabb"][0]), np.float32(vol["aabb"][1])))
        direct = c.render(_camera(native), _opts(native))
    finally:
        c.close()
    assert (frame[..., 3] > 0).sum() > 500 and frame.tobytes() == direct.tobytes()
    default = tb.compute_irradiance_volume([8, 8, 8], None, 32, 32, True)
    del tb
    # no volume: the first render computes the default one (8 x 8 x 8 over the render box, 32 x 32 rays, meshes occluding), the second keeps it
    tb = _testbed(pyngp, scene)
    first = tb.render(w, h, 1, True)
    kept = tb.get_irradiance_volume()
    assert kept["sh"].shape == (8, 8, 8, 28) and np.array_equal(kept["sh"], default["sh"]) and np.array_equal(np.float32(kept["aabb"]), np.float32(default["aabb"]))
    assert tb.render(w, h, 1, True).tobytes() == first.tobytes() and np.array_equal(tb.get_irradiance_volume()["sh"], kept["sh"])
    assert (first[..., 3] > 0).sum() > 100, "the default camera sees no mesh"
    del tb
    # the command line writes that frame: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit)
    tb = _testbed(pyngp, scene)
    tb.irradiance_volume_res = 3
    want = tb.render(w, h, 1, True)
    assert tb.get_irradiance_volume()["sh"].shape == (3, 3, 3, 28)
    del tb
    exe = pkg("build").build_main()
    out = tmp_path / "shot.png"
    r = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "ShadeIrradianceVolume", "--irradiance_volume_res", "3", "--width", str(w), "--height", str(h),
                        "--screenshot", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    png = np.asarray(Image.open(out)).astype(np.int64)
    a = np.clip(want[..., 3:4], 0, 1)
    v = np.clip(np.where(a > 0, want[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
    srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
    expect = np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)
    assert png.shape == (h, w, 4) and np.abs(png - expect).max() <= 1 and (png != expect).mean() < 0.01, (np.abs(png - expect).max(), (png != expect).mean())
    assert (png[..., 3] > 0).sum() > 100
    r = subprocess.run([exe, "--scene", scene, "--render_mode", "ShadeIrradianceVolume", "--irradiance_volume_res", "0", "--screenshot", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "irradiance_volume_res" in r.stderr
