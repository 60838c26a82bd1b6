"""The sun pass on the GPU (include/ngp_hip.h, "sun"): one pass ray by ray against the float64 reference, its records against the
projection of its own rays, equality as bytes wherever the contract promises it, the sunlit volume against the stage entries applied by
hand, the light a sunlit floor throws up, and frames, refusals, pyngp and the command line. Tolerances: irradiance_sun_reference.py's
docstring and test_irradiance_volume.py's projection bound; none comes from the code under test."""
import ctypes
import json

import numpy as np
import pytest

from conftest import pkg

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import irradiance_sun_reference as sr
import irradiance_visibility_reference as vr
import mesh_cases as mc
import mesh_reference as mref
import mesh_volume_cases as mv
from irradiance_volume_cases import GEN_POINTS, gen_meshes
from test_irradiance_visibility_gpu import NO_VISIBILITY, _load, _many_probes, _opts, _set_volume, _small_scene, _testbed

pytestmark = pytest.mark.gpu

STAGE = (sr.STAGE_SUN, sr.STAGE_RADIANCE, sr.STAGE_BIAS)
E2E_SUN = ((1.0, 1.0, 1.0), sr.STAGE_RADIANCE, sr.STAGE_BIAS)  # the frames' default sun
# the frames: irradiance_bounce_reference.e2e_scene (a floor under the NeRF's unit cube, which the default sun lights from above, and a torus
# that reaches into the cube) seen from straight above the cube
SUN_CAMERA = mc.look_at((0.5, 1.9, 0.5), (0.5, -0.1, 0.5))


@pytest.fixture(scope="module")
def ctx(gpu_ctx, native):
    """meshes only, a context of this module's own"""
    c = native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF and, per test, meshes"""
    c = native.Context(0)
    c.set_model(scene_unit)
    yield c
    c.close()


def _volume(c):
    return c.get_irradiance_volume()[1].reshape(-1, 28)


# ----------------------------------------------------------------------------------------------------------- one pass
def test_rays_and_records_of_one_sun_pass(ctx):
    """1. on safe rays: a ray the reference shadows carries exactly 0, a ray it lights carries light wherever alpha < 1, |dB| within 256 ULP of
    the largest albedo x radiance / pi + GPU_FACTOR x the float32 form's deviation, |dt| within TIE_EPS; 2. the records against the float64
    projection of the pass's own rays, within the bound of test_irradiance_volume.py::test_projection_of_the_traced_rays.
    The measured figures are in DESIGN 3.13."""
    _load(ctx, gen_meshes())
    try:
        for nu, nv in br.RAY_SHAPES:
            K, case = nu * nv, sr.stage_case(nu, nv)
            info, safe = case["info"], case["safe"]
            sh, rays = ctx.irradiance_sh_sun(GEN_POINTS, STAGE, br.STAGE_ALBEDO, nu, nv, alpha=case["alpha"], return_rays=True)
            assert sh.shape == (5, 28) and rays.shape == (5, K, 4) and np.isfinite(sh).all() and not np.isnan(rays).any()
            want_t, t, B = case["hit"]["t"], rays[..., 3].astype(np.float64), rays[..., :3]
            assert (info["unsafe"] & info["hit"]).sum() <= 0.02 * info["hit"].sum()
            assert np.array_equal(np.isinf(t)[safe], np.isinf(want_t)[safe])
            both = safe & np.isfinite(want_t)
            dt = np.abs(t[both] - want_t[both]).max() if both.any() else 0.0
            err = np.abs(B.astype(np.float64) - case["B"])[safe].max()
            print("\n%2d x %2d: safe rays %4d, with a hit %3d, shadowed %3d, lit %3d, |dt| %.2e, |dB| %.2e (allowed %.2e, of it the float32 form x %g: %.2e), largest B %.3f"
                  % (nu, nv, safe.sum(), both.sum(), (info["shadowed"] & safe).sum(), (info["lit"] & safe).sum(), dt, err, case["allow"], mc.GPU_FACTOR,
                     mc.GPU_FACTOR * case["dev"], case["B"].max()))
            assert np.all(B[safe & info["shadowed"]] == 0) and np.all(B[safe & ~info["lit"]] == 0)
            assert np.all(B[safe & info["lit"] & (case["alpha"] < 1)] != 0)
            assert dt < mref.TIE_EPS, dt
            assert err <= case["allow"], (err, case["allow"])
            assert np.all(B[np.isinf(t)] == 0)
            # 2. the records of these rays
            want = sh_ref.project(B, sh_ref.sphere_dirs(nu, nv)).reshape(5, 27)
            bound = 1e-5 * (4 * np.pi / K) * np.abs(B.astype(np.float64)).sum(1)  # (5, 3): per channel
            dc = np.abs(sh[:, :27].astype(np.float64) - want).reshape(5, 9, 3)
            print("        records: max |dc| = %.3e, max |dc| / bound = %.3f, max |c| = %.3f" % (dc.max(), (dc / np.maximum(bound[:, None, :], 1e-30)).max(), np.abs(want).max()))
            assert np.all(dc <= bound[:, None, :])
            assert np.array_equal(sh[:, 27], np.isinf(t).mean(1).astype(np.float32))
        assert np.abs(sh[:, :27]).max() > 1e-2
        assert ctx.irradiance_sun_ms() > 0
    finally:
        ctx.clear_meshes()


def test_a_sun_pass_is_deterministic_and_independent_of_the_split(ctx):
    """run to run, and 5 probes in one call against 2 + 3 (five probes: two workgroups of the projection, the second with one live wave;
    5 x 81 rays: no multiple of a workgroup of the ray kernel)"""
    _load(ctx, gen_meshes())
    try:
        for nu, nv in ((9, 9), (16, 16)):
            alpha = br.stage_alpha(5, nu * nv)
            one = ctx.irradiance_sh_sun(GEN_POINTS, STAGE, br.STAGE_ALBEDO, nu, nv, alpha=alpha, return_rays=True)
            two = ctx.irradiance_sh_sun(GEN_POINTS, STAGE, br.STAGE_ALBEDO, nu, nv, alpha=alpha, return_rays=True)
            a = ctx.irradiance_sh_sun(GEN_POINTS[:2], STAGE, br.STAGE_ALBEDO, nu, nv, alpha=alpha[:2], return_rays=True)
            b = ctx.irradiance_sh_sun(GEN_POINTS[2:], STAGE, br.STAGE_ALBEDO, nu, nv, alpha=alpha[2:], return_rays=True)
            for k in (0, 1):
                assert np.array_equal(one[k], two[k]) and np.array_equal(one[k], np.concatenate([a[k], b[k]]))
            assert np.abs(one[0][:, :27]).max() > 1e-2
            # no alpha is alpha 0, and occlusion off is no sun light
            assert np.array_equal(ctx.irradiance_sh_sun(GEN_POINTS, STAGE, br.STAGE_ALBEDO, nu, nv), ctx.irradiance_sh_sun(GEN_POINTS, STAGE, br.STAGE_ALBEDO, nu, nv, alpha=np.zeros_like(alpha)))
            off, off_rays = ctx.irradiance_sh_sun(GEN_POINTS, STAGE, br.STAGE_ALBEDO, nu, nv, alpha=alpha, occlude_by_meshes=False, return_rays=True)
            assert np.all(off[:, :27] == 0) and np.all(off[:, 27] == 1) and np.all(off_rays[..., :3] == 0) and np.all(np.isinf(off_rays[..., 3]))
    finally:
        ctx.clear_meshes()


def test_a_sun_pass_over_two_host_chunks(ctx):
    """600 probes x 64 x 64 rays (a host chunk of 512 whole probes and a tail of 88, see _many_probes), each ray with an alpha of its own:
    every probe's record and every ray from the one call equals the same probe asked for in calls of 100 probes (one chunk each). A probe's
    result does not depend on which probes share its launch, so the small calls are the reference."""
    _load(ctx, _small_scene())
    try:
        probes, alpha = _many_probes(), br.stage_alpha(600, 64 * 64)
        sh, rays = ctx.irradiance_sh_sun(probes, STAGE, br.STAGE_ALBEDO, 64, 64, alpha=alpha, return_rays=True)
        assert sh.shape == (600, 28) and rays.shape == (600, 4096, 4) and np.isfinite(sh).all() and not np.isnan(rays).any()
        for i in range(0, 600, 100):
            s = slice(i, i + 100)
            part_sh, part_rays = ctx.irradiance_sh_sun(probes[s], STAGE, br.STAGE_ALBEDO, 64, 64, alpha=alpha[s], return_rays=True)
            assert np.array_equal(sh[s], part_sh) and np.array_equal(rays[s], part_rays), i
        for chunk in (slice(0, 512), slice(512, 600)):  # (sun light in both chunks, and hits without any: in shadow or turned away)
            hit = np.isfinite(rays[chunk, :, 3])
            lit = rays[chunk, :, 0] > 0
            assert np.abs(sh[chunk, :27]).max() > 1e-2 and lit.any() and (hit & ~lit).any() and (~hit).any()
    finally:
        ctx.clear_meshes()


# ------------------------------------------------------------------------------------------------------ the sunlit volume
def test_no_source_is_the_bounced_volume(hybrid):
    """no sun, a sun without radiance, a black albedo, no meshes and occlusion off each give ngp_compute_irradiance_volume_bounced's records
    as bytes"""
    res, lo, hi, nu, nv = br.E2E_CASE
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=1, albedo=br.E2E_ALBEDO)
        v1 = _volume(hybrid)
        d = hybrid._volume_desc(res, (lo, hi), hybrid._sh_desc(nu, nv, True, 0.01))  # sun = NULL reaches the entry through the C ABI alone
        hybrid._check(hybrid.L.ngp_compute_irradiance_volume_sunlit(hybrid.h, ctypes.byref(d), ctypes.byref(hybrid._bounce_desc(1, br.E2E_ALBEDO)), None, None))
        assert _volume(hybrid).tobytes() == v1.tobytes()
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=1, albedo=br.E2E_ALBEDO, sun=(E2E_SUN[0], 0.0, 1e-3))
        assert _volume(hybrid).tobytes() == v1.tobytes()
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=1, albedo=br.E2E_ALBEDO, sun=E2E_SUN)
        assert _volume(hybrid).tobytes() != v1.tobytes()  # (and a sun with radiance is in the numbers)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        v0 = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=2, albedo=0.0, sun=E2E_SUN)
        assert _volume(hybrid).tobytes() == v0.tobytes()
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, occlude_by_meshes=False)
        free = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=1, albedo=br.E2E_ALBEDO, occlude_by_meshes=False, sun=E2E_SUN)
        assert _volume(hybrid).tobytes() == free.tobytes()
        hybrid.clear_meshes()
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        bare = _volume(hybrid)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=1, albedo=br.E2E_ALBEDO, sun=E2E_SUN)
        assert _volume(hybrid).tobytes() == bare.tobytes() and bare.tobytes() != v0.tobytes()
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


def _add(v0, r):
    """V_0 + R on the 27 coefficients in float32; float 27 V_0's"""
    out = v0.copy()
    out[:, :27] = v0[:, :27] + r[:, :27]
    assert np.array_equal(r[:, 27], v0[:, 27])  # (the same rays against the same meshes)
    return out


def test_sunlit_volume_is_the_stages_applied_by_hand(hybrid):
    """N = 0 holds S = V_0 + the stage sun pass with the trace's own alpha; N = 2 continues from that S with two stage bounce passes, S in
    V_0's place; as bytes, plain and through a visibility descriptor, whose maps are ngp_compute_irradiance_volume_visibility's and stay"""
    res, lo, hi, nu, nv = br.E2E_CASE
    positions = vr.probe_positions(res, lo, hi)
    vis = dict(n_u=8, n_v=8, sharpness_log2=4, max_distance=0.0, normal_bias=0.01)
    _load(hybrid, br.e2e_scene())
    try:
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        v0 = _volume(hybrid)
        hybrid.compute_irradiance_volume_visibility(**vis)
        d0, maps = hybrid.get_irradiance_volume_visibility()
        _, traced = hybrid.irradiance_sh_traced(positions, nu, nv, return_rays=True)
        alpha = traced[..., 3]
        assert (alpha > 0.05).any() and (alpha < 0.95).any()  # the NeRF is in front of some hits
        S = _add(v0, hybrid.irradiance_sh_sun(positions, E2E_SUN, br.E2E_ALBEDO, nu, nv, alpha=alpha))
        assert np.abs(S[:, :27] - v0[:, :27]).max() > 1e-3
        for visibility in (None, vis):
            visible = visibility is not None

            def hold(records):
                _set_volume(hybrid, records, res, lo, hi)
                if visible:
                    hybrid.set_irradiance_volume_visibility(maps, d0.max_distance, d0.sharpness_log2, d0.normal_bias)

            hold(S)
            v1 = _add(S, hybrid.irradiance_sh_bounce(positions, br.E2E_ALBEDO, nu, nv, alpha=alpha, visible=visible))
            hold(v1)
            v2 = _add(S, hybrid.irradiance_sh_bounce(positions, br.E2E_ALBEDO, nu, nv, alpha=alpha, visible=visible))
            assert np.abs(v2[:, :27] - v1[:, :27]).max() > 1e-5
            for n, want in ((0, S), (2, v2)):
                for _ in range(2):  # (and run to run)
                    hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, bounces=n, albedo=br.E2E_ALBEDO, visibility=visibility, sun=E2E_SUN)
                    got = _volume(hybrid)
                    assert got.tobytes() == want.tobytes(), (n, visible, np.abs(got - want).max())
                if visible:
                    d, held = hybrid.get_irradiance_volume_visibility()
                    assert held.tobytes() == maps.tobytes()
                    assert (d.n_u, d.n_v, d.sharpness_log2, d.max_distance, d.normal_bias) == (d0.n_u, d0.n_v, d0.sharpness_log2, d0.max_distance, d0.normal_bias)
                else:
                    with pytest.raises(RuntimeError, match=NO_VISIBILITY):  # (the sunlit compute drops what was held, like the plain one)
                        hybrid.get_irradiance_volume_visibility()
        assert hybrid.irradiance_sun_ms() > 0
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


def test_a_sunlit_floor_lights_what_is_above_it(hybrid):
    """under a point 5 cm above the unit cube's bottom, over the floor, E for the down-facing normal rises with the sun, by no more than
    test_irradiance_sun_cpu.py::test_an_open_floor_throws_sun_light_up allows (the NeRF in front of the floor only takes away)"""
    albedo, res, lo, hi, nu, nv = br.FLOOR_CASE
    _load(hybrid, br.floor_scene())
    try:
        p, down = np.float32([[0.5, 0.05, 0.5], [0.3, 0.1, 0.6]]), np.float32([[0, -1, 0], [0, -1, 0]])
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv)
        before = hybrid.irradiance_volume_at(p, down)
        hybrid.compute_irradiance_volume(res, (lo, hi), nu, nv, albedo=albedo, sun=E2E_SUN)
        after = hybrid.irradiance_volume_at(p, down)
        gain = (after - before)[:, :3].astype(np.float64)
        bound = np.float32(albedo).astype(np.float64) * sr.STAGE_RADIANCE.astype(np.float64) * float(sr.unit_sun(E2E_SUN[0])[1]) * sr.OVERSHOOT
        print("\nE(down) %s -> %s with the sun; bound on the gain %s" % (before[0, :3], after[0, :3], bound))
        assert np.all(gain > 0) and np.all(gain <= bound), (gain, bound)
        assert np.array_equal(after[:, 3], before[:, 3])
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


# --------------------------------------------------------------------------------------------- frames, refusals, bindings
def test_frames_devices_and_other_modes(hybrid, native, scene_unit):
    """a sunlit volume reaches the replicas of a multi-device context in one step: the ShadeIrradianceVolume frame is the same bytes on two
    devices and on one, and differs from the frame without the sun; Shade and ShadeGridEnvMap frames do not see it"""
    res, box, nu, nv = (2, 2, 2), (np.float32([0, 0, 0]), np.float32([1, 1, 1])), 16, 16
    cam = native.make_camera(SUN_CAMERA, mc.WIDTH, mc.HEIGHT, (100.0, 100.0))
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        frames = {}
        for c in (hybrid, multi):
            _load(c, br.e2e_scene())
            c.set_geometry_opts()
        hybrid.set_geometry_opts(ambientcolor=mv.SKY_AMBIENT)
        hybrid.compute_envmap_grid(2, 2, 16, 8)
        modes = (native.RENDER_SHADE, native.RENDER_SHADE_GRID_ENVMAP)
        hybrid.compute_irradiance_volume(res, box, nu, nv)
        others = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
        hybrid.set_geometry_opts()
        for key, kw in (("plain", {}), ("sunlit", dict(albedo=0.64, sun=E2E_SUN)), ("sunlit_bounced_visible", dict(bounces=1, albedo=0.64, visibility=dict(n_u=8, n_v=8), sun=E2E_SUN))):
            for c in (hybrid, multi):
                c.compute_irradiance_volume(res, box, nu, nv, **kw)
            one, one_depth = hybrid.render(cam, _opts(native), want_depth=True)
            two, two_depth = multi.render(cam, _opts(native), want_depth=True)
            assert (one[..., 3] > 0).sum() > 500
            assert one.tobytes() == two.tobytes() and one_depth.tobytes() == two_depth.tobytes(), key
            frames[key] = one
        assert len({f.tobytes() for f in frames.values()}) == 3
        changed = np.abs(frames["sunlit"] - frames["plain"]).max(-1) > 0
        print("\nthe sun's first bounce changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(frames["sunlit"] - frames["plain"]).max()))
        assert changed.sum() > 100
        hybrid.set_geometry_opts(ambientcolor=mv.SKY_AMBIENT)
        held = [hybrid.render(cam, _opts(native, mode=m), want_depth=True) for m in modes]
        for (a, ad), (b, bd) in zip(held, others):
            assert (a[..., 3] > 0).sum() > 500 and a.tobytes() == b.tobytes() and ad.tobytes() == bd.tobytes()
    finally:
        multi.close()
        hybrid.set_geometry_opts()
        hybrid.clear_irradiance_volume()
        hybrid.clear_meshes()


def test_refusals(hybrid, native):
    res, lo, hi, nu, nv = br.E2E_CASE
    one = np.float32([[0.5, 0.5, 0.5]])
    up = dict(direction=(0, 1, 0))
    nan, inf = float("nan"), float("inf")
    bad_suns = [(dict(direction=(0, 0, 0)), "direction must be finite and not zero"), (dict(direction=(0, nan, 1)), "direction"), (dict(direction=(0, 1, 0), radiance=(1, 1, -1)), "radiance"),
                (dict(direction=(0, 1, 0), radiance=inf), "radiance"), (dict(direction=(0, 1, 0), shadow_bias=-0.5), "shadow_bias"), (dict(direction=(0, 1, 0), shadow_bias=nan), "shadow_bias")]
    c = native.Context(0)
    try:
        with pytest.raises(RuntimeError, match="No network"):
            c.compute_irradiance_volume(res, (lo, hi), nu, nv, sun=up)
        # the stage entry needs neither a model nor a volume nor meshes: without meshes nothing is hit
        sh, rays = c.irradiance_sh_sun(one, up, 0.5, 4, 4, return_rays=True)
        assert np.all(sh[:, :27] == 0) and np.all(sh[:, 27] == 1) and np.all(np.isinf(rays[..., 3]))
        assert c.irradiance_sh_sun(np.zeros((0, 3), np.float32), up, 0.5, 4, 4).shape == (0, 28)
        for kw, message in ((dict(n_u=0), "n_u and n_v"), (dict(n_u=2048, n_v=2048), "too large")):
            with pytest.raises(RuntimeError, match=message):
                c.irradiance_sh_sun(one, up, 0.5, **kw)
        with pytest.raises(RuntimeError, match="position 0 is not finite"):
            c.irradiance_sh_sun(np.float32([[0.5, nan, 0.5]]), up, 0.5, 4, 4)
        for bad in (nan, inf):
            alpha = np.zeros((1, 16), np.float32)
            alpha[0, 7] = bad
            with pytest.raises(RuntimeError, match="alpha 7 is not finite"):
                c.irradiance_sh_sun(one, up, 0.5, 4, 4, alpha=alpha)
        for bad in (1.5, -0.1, nan):
            with pytest.raises(RuntimeError, match="albedo must be finite and in"):
                c.irradiance_sh_sun(one, up, bad, 4, 4)
        for sun, message in bad_suns:
            with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: " + message):
                c.irradiance_sh_sun(one, sun, 0.5, 4, 4)
    finally:
        c.close()
    try:
        hybrid.clear_meshes()
        hybrid.compute_irradiance_volume(res, (lo, hi), 4, 4)
        held = _volume(hybrid)
        bad = [(dict(bounces=17, albedo=0.5), "n_bounces must be at most 16"), (dict(albedo=1.5), "albedo"), (dict(bounces=1, albedo=(0.1, nan, 0.1)), "albedo"),
               (dict(albedo=0.5, n_u=0), "n_u and n_v"), (dict(albedo=0.5, visibility=dict(sharpness_log2=7)), "sharpness_log2"),
               (dict(bounces=1, albedo=0.5, visibility=dict(normal_bias=-1.0)), "normal_bias"), (dict(albedo=0.5, visibility=dict(n_u=0)), "n_u and n_v")]
        for kw, message in bad:
            with pytest.raises(RuntimeError, match=message):
                hybrid.compute_irradiance_volume(res, (lo, hi), **dict(dict(n_u=4, n_v=4, sun=up), **kw))
        for sun, message in bad_suns:
            with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: " + message):
                hybrid.compute_irradiance_volume(res, (lo, hi), 4, 4, bounces=1, albedo=0.5, sun=sun)
        with pytest.raises(RuntimeError, match="resolution"):
            hybrid.compute_irradiance_volume((2, 0, 2), (lo, hi), 4, 4, sun=up)
        d = hybrid._volume_desc(res, (lo, hi), hybrid._sh_desc(4, 4, True, 0.01))
        with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: the bounce descriptor"):
            hybrid._check(hybrid.L.ngp_compute_irradiance_volume_sunlit(hybrid.h, ctypes.byref(d), None, None, ctypes.byref(hybrid._sun_desc(up))))
        assert _volume(hybrid).tobytes() == held.tobytes()  # the failed calls left the held volume alone
    finally:
        hybrid.clear_irradiance_volume()


def _write_scene(tmp_path, hybrid):
    """e2e_scene's meshes as .obj files, the unit NeRF as a snapshot, and the scene file that names them"""
    mi = pkg("meshio")
    entries = []
    for i, (tris, center) in enumerate(br.e2e_scene()):
        mi.save_obj(str(tmp_path / ("sun%d.obj" % i)), tris)
        entries.append({"center": [float(x) for x in center], "path": "sun%d.obj" % i, "type": "Mesh"})
    hybrid.save_snapshot_file(str(tmp_path / "unit.ingp"))
    entries.append({"center": [0, 0, 0], "path": "unit.ingp", "type": "Nerf"})
    path = tmp_path / "sun_geometry_scene.json"  # (the Testbed takes a scene file for a Geometry scene by the word in its name)
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def _sun_testbed(pyngp, scene, **kw):
    tb = _testbed(pyngp, scene, **kw)
    if kw.get("camera", True):
        tb.camera_matrix = SUN_CAMERA
    return tb


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    """the Testbed's keyword (its sun is the frame's: sun_dir, irradiance_volume_sun_radiance, bias 1e-3; its albedo the base colour squared
    even without bounces), irradiance_volume_sun for the default volume of a ShadeIrradianceVolume render, and --irradiance_volume_sun"""
    import subprocess
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    hybrid.clear_meshes()
    scene = _write_scene(tmp_path, hybrid)
    w, h = mc.WIDTH, mc.HEIGHT
    cam = native.make_camera(SUN_CAMERA, w, h, (100.0, 100.0))
    tb = _sun_testbed(pyngp, scene)
    assert tb.irradiance_volume_sun is False and np.allclose(tb.irradiance_volume_sun_radiance, sr.STAGE_RADIANCE, rtol=1e-6, atol=0)
    off = tb.render(w, h, 1, True)
    v0 = tb.get_irradiance_volume()
    box = (np.float32(v0["aabb"][0]), np.float32(v0["aabb"][1]))
    vol = tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, sun=True)
    tb.irradiance_volume_sun_radiance = [1.0, 2.0, 3.0]
    own = tb.compute_irradiance_volume([2, 2, 2], None, 32, 32, True, bounces=1, albedo=[0.9, 0.5, 0.1], sun=True)
    del tb
    sun = ((1.0, 1.0, 1.0), native.SUN_RADIANCE, 1e-3)  # _testbed's sun_dir
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, sun=sun)
        assert c.get_irradiance_volume()[1].tobytes() == vol["sh"].tobytes() and vol["sh"].tobytes() != v0["sh"].tobytes()
        direct = c.render(cam, _opts(native))
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, bounces=1, albedo=(0.9, 0.5, 0.1), sun=(sun[0], (1.0, 2.0, 3.0), 1e-3))
        assert c.get_irradiance_volume()[1].tobytes() == own["sh"].tobytes() and own["sh"].tobytes() != vol["sh"].tobytes()
        c.compute_irradiance_volume((2, 2, 2), box, 32, 32, bounces=1, visibility={}, sun=sun)
        direct_visible = c.render(cam, _opts(native))
    finally:
        c.close()
    tb = _sun_testbed(pyngp, scene)
    tb.irradiance_volume_sun = True
    on = tb.render(w, h, 1, True)
    assert tb.render(w, h, 1, True).tobytes() == on.tobytes()
    assert tb.get_irradiance_volume()["sh"].tobytes() == vol["sh"].tobytes()  # the render holds compute_irradiance_volume(sun=True)'s records
    del tb
    tb = _sun_testbed(pyngp, scene, visibility=True)
    tb.irradiance_volume_sun, tb.irradiance_volume_bounces = True, 1
    on_visible = tb.render(w, h, 1, True)
    del tb
    changed = np.abs(on - off).max(-1) > 0
    print("\npyngp: irradiance_volume_sun changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(on - off).max()))
    assert (off[..., 3] > 0).sum() > 500 and changed.sum() > 100
    assert on.tobytes() == direct.tobytes() and on_visible.tobytes() == direct_visible.tobytes() and on_visible.tobytes() != on.tobytes()
    # the command line writes that frame: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit)
    tb = _sun_testbed(pyngp, scene, camera=False)
    dark = tb.render(w, h, 1, True)
    del tb
    tb = _sun_testbed(pyngp, scene, camera=False)
    tb.irradiance_volume_sun = True
    want = tb.render(w, h, 1, True)
    del tb
    assert (np.abs(want - dark).max(-1) > 0).sum() > 20  # (the default sun is in the default camera's frame)
    exe = pkg("build").build_main()
    out = tmp_path / "shot.png"
    r = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "ShadeIrradianceVolume", "--irradiance_volume_res", "2", "--irradiance_volume_sun", "--width", str(w),
                        "--height", str(h), "--screenshot", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    png = np.asarray(Image.open(out)).astype(np.int64)
    a = np.clip(want[..., 3:4], 0, 1)
    v = np.clip(np.where(a > 0, want[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
    srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
    expect = np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)
    assert png.shape == (h, w, 4) and np.abs(png - expect).max() <= 1 and (png != expect).mean() < 0.01, (np.abs(png - expect).max(), (png != expect).mean())
    assert (png[..., 3] > 0).sum() > 100
