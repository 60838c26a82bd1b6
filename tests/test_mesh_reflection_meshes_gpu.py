"""The meshes in the mesh reflection on the GPU (include/ngp_hip.h, "mesh reflection, the meshes in it"): the identities the contract promises
as bytes, the hit record against the float64 reference, the colour against the reference rendered with the recorded radiance and the recorded
hit colour, the direction of the change, every ambient source, and the structure around it: the sun shadow beside it, determinism, samples,
shards, devices, streams and bindings.
Tolerances: mesh_cases.position_tolerance on the float32 form's own deviation for p2 (test_mesh_reflection_gpu.py's rule for t_hit),
mesh_sun_nerf_shadow_cases' colour rule for C2 and the frame, plus GPU_FACTOR x the float32 form's own deviation of the added term; none comes
from the code under test. The measured figures are in DESIGN 3.20."""
import json
import subprocess

import numpy as np
import pytest

from conftest import pkg

import mesh_cases as mc
import mesh_reflection_meshes_cases as hc
import mesh_volume_cases as mv

pytestmark = pytest.mark.gpu

W, H = hc.WIDTH, hc.HEIGHT
ON = dict(strength=1.0, min_transmittance=0.01, t_min=0.0)
SUN_NERF = (0.01, 0.0)
VOLUME_BOX = (np.float32([-0.1, -0.2, -0.1]), np.float32([1.6, 1.5, 1.1]))
RICH = dict(ambientcolor=mv.SKY_AMBIENT, up_dir=(1.0, 0.0, 0.0), metallic=0.3, clearcoat=0.5, sheen=0.5)  # every term of the BRDF and the sky at work


def _load(c, scene):
    c.clear_meshes()
    for tris, center in scene:
        c.add_mesh(tris, center)


def _opts(native, mode=None, **kw):
    return native.make_opts(**dict(dict(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0), render_mode=native.RENDER_SHADE if mode is None else mode), **kw))


def _cam(native, w=W, h=H, **kw):
    return native.make_camera(hc.CAMERA, w, h, hc.FOCAL, **kw)


def _render(c, native, reflection, meshes, cam=None, sun=None, **kw):
    """a frame (colour, depth) with the reflection, the sub-option and the sun shadow as given; all three are off again afterwards"""
    c.set_mesh_reflection(reflection)
    c.set_mesh_reflection_meshes(meshes)
    c.set_sun_nerf_shadow(sun)
    try:
        return c.render(cam or _cam(native), _opts(native, **kw), want_depth=True)
    finally:
        c.set_mesh_reflection(None)
        c.set_mesh_reflection_meshes(False)
        c.set_sun_nerf_shadow(None)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _hits(c, n=W * H):
    return c.frame_mesh_reflection_hits(n)


def _context(native, scene_unit, case, model=True):
    c = native.Context(0)
    if model:
        c.set_model(scene_unit)
    _load(c, hc.scene(case))
    c.set_geometry_opts(sun_dir=hc.SUN[case])
    return c


@pytest.fixture(scope="module")
def contexts(gpu_ctx, native, scene_unit):
    """per case: the unit NeRF over the case's meshes under the case's sun; and case C's meshes alone"""
    cs = {case: _context(native, scene_unit, case) for case in ("A", "B", "C")}
    cs["bare"] = _context(native, scene_unit, "C", model=False)
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def shots(contexts, native):
    """per case: the frames most tests compare. plain: every option off; off: the reflection alone, with its 12-float record; on: the
    sub-option too, with both records; bare (case C): the meshes alone"""
    out = {}
    for case in ("A", "B", "C"):
        c = contexts[case]
        s = dict(plain=_render(c, native, None, False))
        c.set_mesh_reflection(ON)
        try:
            s["off"] = c.render(_cam(native), _opts(native), want_depth=True)
            s["off_record"] = c.frame_mesh_reflection(W * H).reshape(H, W, 12)
            s["off_stats"] = c.render_stats()
            c.set_mesh_reflection_meshes(True)
            s["on"] = c.render(_cam(native), _opts(native), want_depth=True)
            s["on_record"] = c.frame_mesh_reflection(W * H).reshape(H, W, 12)
            s["hits"] = _hits(c).reshape(H, W, 8)
            s["on_stats"], s["hits_ms"], s["trace_ms"] = c.render_stats(), c.frame_mesh_reflection_hits_ms(), c.frame_mesh_reflection_ms()
        finally:
            c.set_mesh_reflection(None)
            c.set_mesh_reflection_meshes(False)
        out[case] = s
    out["C"]["bare"] = _render(contexts["bare"], native, None, False)
    return out


# ------------------------------------------------------------------------------------------------------- identities as bytes
def test_identities_as_bytes(contexts, shots, native):
    """case C. The sub-option off after on; on with the reflection off; on at strength 0; on in NeRF mode; on without meshes; on with the
    meshes alone: each is the frame of the same options without the sub-option, colour and depth, and none of them shades a hit"""
    c, s = contexts["C"], shots["C"]
    assert not _same(s["on"], s["off"]) and not _same(s["off"], s["plain"])
    assert _same(_render(c, native, ON, False), s["off"])                                  # off after on
    assert c.frame_mesh_reflection_hits_ms() == 0
    with pytest.raises(RuntimeError, match="shaded no reflection hits"):
        _hits(c)
    assert _same(_render(c, native, None, True), s["plain"])                               # the reflection off
    assert _same(_render(c, native, dict(strength=0.0), True), s["plain"])                 # strength 0: no trace is run
    with pytest.raises(RuntimeError, match="shaded no reflection hits"):
        _hits(c)
    nerf_mode = dict(testbed_mode=native.MODE_NERF)
    assert _same(_render(c, native, ON, True, **nerf_mode), _render(c, native, None, False, **nerf_mode))
    assert _same(_render(contexts["bare"], native, ON, True), s["bare"])                   # no model
    with pytest.raises(RuntimeError, match="shaded no reflection hits"):
        _hits(contexts["bare"])
    c.clear_meshes()
    try:
        assert _same(_render(c, native, ON, True), _render(c, native, None, False))        # Geometry mode without meshes
    finally:
        _load(c, hc.scene("C"))
    assert _same(_render(c, native, ON, True), s["on"]) and c.mesh_reflection_meshes() is False


def test_a_scene_without_cut_rays_is_the_reflection_only_frame(shots):
    """case A: no mirror ray is cut, and the frame with the sub-option on is the reflection-only frame as bytes, its 12-float record too; the
    hit record is all zeros. Case C: the 12-float record and depth are those of the sub-option-off frame as bytes, and so are the statistics"""
    a = shots["A"]
    assert _same(a["on"], a["off"]) and a["on_record"].tobytes() == a["off_record"].tobytes() and not a["hits"].any()
    assert (a["off_record"][..., 11] > 0.9).sum() > 20
    s = shots["C"]
    assert s["on_record"].tobytes() == s["off_record"].tobytes() and s["on"][1].tobytes() == s["off"][1].tobytes() and s["on"][0].tobytes() != s["off"][0].tobytes()
    for k in ("n_rays", "n_rays_alive_after_init", "n_rays_hit", "n_samples"):
        assert s["on_stats"][k] == s["off_stats"][k], k
    print("\nhit-shade kernel %.3f ms inside a reflection prep + trace of %.3f ms" % (s["hits_ms"], s["trace_ms"]))
    assert 0 < s["hits_ms"] <= s["trace_ms"]


# ---------------------------------------------------------------------------------------------------------------- the record
@pytest.mark.parametrize("case", ["B", "C"])
def test_hit_record_matches_the_reference(case, shots):
    """(a) a pixel owns a hit exactly where the reference's mirror ray is cut (safe rays), and the record is zero elsewhere, its last float 1 on
    owners; (b) |p2 - p2_64| <= mesh_cases.position_tolerance(the float32 form's own deviation, t_hit); (c) shadow2 is the reference's on safe
    hits (case B has both values, case C is lit); (d) |C2 - C2_64| <= frame_bound(C2_64)"""
    fr = hc.frame(case)
    rec = shots[case]["hits"]
    owns = rec[..., 7] != 0
    safe = ~fr["unsafe"] & ~fr["t_unsafe"] & ~fr["hit_unsafe"]
    assert not np.isnan(rec).any() and not np.any(rec[~owns]) and np.all(rec[..., 7][owns] == 1)
    assert np.array_equal(owns[safe], fr["cut"][safe])                                                       # (a)
    assert np.array_equal(owns, np.isfinite(shots[case]["on_record"][..., 3]) & np.any(shots[case]["on_record"][..., 4:7] != 0, -1))
    m = safe & fr["cut"]
    dp = np.abs(rec[..., 0:3].astype(np.float64) - fr["p2"])[m].max(-1)
    tol = mc.position_tolerance(fr["p2_dev"], fr["t_hit"][m])
    dc = np.abs(rec[..., 4:7].astype(np.float64) - fr["C2"])[m]
    bound = hc.frame_bound(fr["C2"])[m]
    lit = m & fr["faces_sun"] & (fr["shadow2"] == 1)
    print("\ncase %s: %d hits (safe %d; shadow2 = 1: %d, = 0: %d; lit and facing the sun %d); |dp2| / tolerance %.3f (largest %.2e, the float32 form deviates by %.2e); "
          "|dC2| / bound %.3f (largest C2 %.3f)" % (case, owns.sum(), m.sum(), (rec[..., 3][m] == 1).sum(), (rec[..., 3][m] == 0).sum(), lit.sum(), (dp / tol).max(), dp.max(),
                                                    fr["p2_dev"], (dc / bound).max(), fr["C2"][m].max()))
    assert m.sum() >= 100 and (fr["hit_unsafe"] & fr["cut"]).sum() <= mc.UNSAFE_CAP * fr["cut"].sum()
    assert np.all(dp <= tol), (dp / tol).max()                                                               # (b)
    assert np.array_equal(rec[..., 3][m], fr["shadow2"][m].astype(np.float32))                               # (c)
    if case == "B":
        assert (rec[..., 3][m] == 0).sum() >= hc.MIN_SHADOWED and (rec[..., 3][m] == 1).sum() > 0
    else:
        assert lit.sum() >= hc.MIN_LIT_OPEN
    assert np.all(dc <= bound), (dc / bound).max()                                                           # (d)
    assert fr["C2"][lit].max() > 0.1


# ---------------------------------------------------------------------------------------------------------------- the colour
@pytest.mark.parametrize("case", ["B", "C"])
def test_colour_is_the_reference_with_the_recorded_radiance_and_hit_colour(case, contexts, shots, native, scene_unit):
    """Clear pixels: the plain hybrid frame equals the frame of the meshes alone as bytes, so the NeRF pass added nothing there. On clear, safe,
    covered pixels the frame is the float64 reference rendered with the recorded (rgb_r, alpha_r) and the recorded C2, within frame_bound plus
    GPU_FACTOR x the float32 form's own deviation of the added term where that is not zero. Pixels without a hit are the sub-option-off
    frame's as bytes."""
    s = shots[case]
    if case == "C":
        bare = s["bare"]
    else:
        b = _context(native, scene_unit, case, model=False)
        try:
            bare = _render(b, native, None, False)
        finally:
            b.close()
    plain, on, off = s["plain"], s["on"], s["off"]
    clear = np.all(plain[0].view(np.uint32) == bare[0].view(np.uint32), axis=-1) & (plain[1].view(np.uint32) == bare[1].view(np.uint32))
    rgba_r, hit = s["on_record"][..., 8:12], s["hits"][..., 7] != 0
    fr = hc.frame(case, rgba_r, hit_colour=s["hits"][..., 4:7])
    want = fr["rgba"][..., :3]
    dev32 = np.abs(fr["added32"].astype(np.float64) - fr["added"])
    base, extra = hc.frame_bound(want), mc.GPU_FACTOR * dev32
    m = clear & ~fr["unsafe"] & ~fr["t_unsafe"] & ~fr["hit_unsafe"] & fr["covered"]
    err = np.abs(on[0][..., :3].astype(np.float64) - want)
    ratio = (err / (base + extra))[m]
    share = extra[m & hit].max() / (base + extra)[m & hit].min() if (m & hit).any() else 0.0
    print("\ncase %s: clear pixels %d (safe and covered %d, of them with a hit %d); largest colour deviation / bound %.3f (%.2e absolute; without the float32 allowance %.3f); "
          "the float32 form of the term deviates by at most %.2e, at most %.3f of a bound" % (case, clear.sum(), m.sum(), (m & hit).sum(), ratio.max(), err[m].max(),
                                                                                            (err / base)[m].max(), dev32[m].max(), share))
    assert (m & hit).sum() >= 50
    assert np.array_equal(on[0][..., 3][m], fr["rgba"][..., 3][m])
    assert ratio.max() <= 1.0, ratio.max()
    assert on[0][~hit].tobytes() == off[0][~hit].tobytes() and on[1].tobytes() == off[1].tobytes()


def test_direction_of_the_change(shots):
    """case C: every safe lit hit whose ray sees nothing of the NeRF (alpha_r = 0) is strictly brighter than in the sub-option-off frame, in
    every channel, on the clear pixels (where the NeRF pass, which composites over the mesh pass, added nothing: an opaque NeRF pixel in front
    hides its mesh pixel whole); no pixel is darker; a hit the object hides (alpha_r > 0.9) gains at most (1 - alpha_r) strength |F (.) C2_ref|
    plus the colour bound"""
    s = shots["C"]
    fr = hc.frame("C")
    on, off = s["on"][0][..., :3].astype(np.float64), s["off"][0][..., :3].astype(np.float64)
    a = s["on_record"][..., 11]
    safe = ~fr["unsafe"] & ~fr["t_unsafe"] & ~fr["hit_unsafe"]
    lit = safe & fr["cut"] & fr["faces_sun"] & (fr["shadow2"] == 1)
    clear = np.all(s["plain"][0].view(np.uint32) == s["bare"][0].view(np.uint32), axis=-1)
    open_, hidden = lit & (a == 0), lit & (a > 0.9)
    gain = on - off
    cap = (np.maximum(1.0 - a.astype(np.float64), 0.0)[..., None] * fr["F"] * fr["C2"]) + hc.frame_bound(on)
    print("\ncase C: lit hits at alpha_r = 0: %d (on clear pixels %d, smallest gain %.3g), at alpha_r > 0.9: %d (largest gain %.3g, largest gain / cap %.3f); largest loss %.3g"
          % (open_.sum(), (open_ & clear).sum(), gain[open_ & clear].min(), hidden.sum(), gain[hidden].max(), (gain / cap)[hidden].max(), (off - on).max()))
    assert open_.sum() >= hc.MIN_LIT_OPEN and hidden.sum() >= hc.MIN_LIT_HIDDEN
    assert (open_ & clear).sum() >= 50 and np.all(gain[open_ & clear] > 0)
    assert np.all(on >= off)
    assert np.all(gain[hidden] <= cap[hidden])


# ------------------------------------------------------------------------------------------------------------ ambient sources
@pytest.mark.parametrize("mode", ["Shade", "ShadeEnvMap", "ShadeGridEnvMap", "ShadeIrradianceVolume", "ShadeIrradianceVolumeVisible"])
def test_every_ambient_source_reaches_the_hit(mode, contexts, native):
    """case C with geometry options that put every term of the BRDF to work, per source of ambient light: C2 is the float64 shade at the
    reference's hit with that source's ambient light there -- the sky term in float64, or E / pi of the context's own lookup at the recorded
    p2 and the reference's n2 (ngp_irradiance_at, ngp_irradiance_volume_at, with visibility where the frame uses it) -- within
    frame_bound(C2_ref); the frame is not the sub-option-off frame and its depth is"""
    c = contexts["C"]
    c.set_geometry_opts(sun_dir=hc.SUN["C"], **RICH)
    try:
        if mode == "ShadeEnvMap":
            c.compute_envmap(n_theta=16, n_phi=8)
        elif mode == "ShadeGridEnvMap":
            c.compute_envmap_grid(2, 2, 16, 8)
        elif mode.startswith("ShadeIrradianceVolume"):
            c.compute_irradiance_volume((3, 2, 3), VOLUME_BOX, 8, 8, occlude_by_meshes=False)
            if mode.endswith("Visible"):
                c.compute_irradiance_volume_visibility(n_u=8, n_v=8, sharpness_log2=4, max_distance=0.0, normal_bias=0.01)
        kw = dict(mode={"Shade": native.RENDER_SHADE, "ShadeEnvMap": native.RENDER_SHADE_ENVMAP, "ShadeGridEnvMap": native.RENDER_SHADE_GRID_ENVMAP}.get(mode, native.RENDER_SHADE_IRRADIANCE_VOLUME))
        off = _render(c, native, ON, False, **kw)
        c.set_mesh_reflection(ON)
        c.set_mesh_reflection_meshes(True)
        try:
            on = c.render(_cam(native), _opts(native, **kw), want_depth=True)
            rec = _hits(c).reshape(H, W, 8)
        finally:
            c.set_mesh_reflection(None)
            c.set_mesh_reflection_meshes(False)
        geo = hc.frame("C")
        m = geo["cut"] & ~geo["unsafe"] & ~geo["t_unsafe"] & ~geo["hit_unsafe"] & (rec[..., 7] != 0)
        p2, n2 = np.ascontiguousarray(rec[..., 0:3][m]), np.ascontiguousarray(geo["n2"][m], np.float32)
        if mode == "Shade":
            ambient = mv.sky_ambient_fn(RICH["ambientcolor"], RICH["up_dir"])
        else:
            if mode.startswith("ShadeIrradianceVolume"):
                E = np.maximum(c.irradiance_volume_at(p2, n2, visible=mode.endswith("Visible"))[:, :3].astype(np.float64), 0.0)
            else:
                E = c.irradiance_at(p2, n2).astype(np.float64)
            at_hits = np.zeros((H, W, 3))
            at_hits[m] = E / np.pi
            at_hits = at_hits[geo["cut"]]

            hit_points = geo["p2"][geo["cut"]]

            def ambient(pos, N):  # (the lookup's value at the reference's hit points, which are compared; none at the primary pixels, which are not)
                return at_hits if pos.shape == hit_points.shape and np.array_equal(pos, hit_points) else np.zeros_like(pos)
        brdf = {k: v for k, v in RICH.items() if k not in ("ambientcolor", "up_dir")}
        fr = hc.frame("C", ambient_fn=ambient, **brdf)
        dc = np.abs(rec[..., 4:7].astype(np.float64) - fr["C2"])[m]
        bound = hc.frame_bound(fr["C2"])[m]
        dark = m & (fr["shadow2"] == 0) | (m & ~fr["faces_sun"])
        print("\n%s: %d safe hits; |dC2| / bound %.3f; C2 %.3g .. %.3g; the ambient term alone at %d hits (largest %.3g); the sub-option changes %d pixels"
              % (mode, m.sum(), (dc / bound).max(), fr["C2"][m].min(), fr["C2"][m].max(), dark.sum(), fr["C2"][dark].max() if dark.any() else 0, (np.abs(on[0] - off[0]).max(-1) > 0).sum()))
        assert m.sum() >= 100 and np.unique(rec[..., 4][m]).size > 20
        assert np.all(dc <= bound), (dc / bound).max()
        assert not _same(on, off) and on[1].tobytes() == off[1].tobytes() and np.all(on[0] >= off[0])
    finally:
        c.clear_irradiance_volume()
        c.set_geometry_opts(sun_dir=hc.SUN["C"])


# ----------------------------------------------------------------------------------------------------------------- structure
def test_with_the_sun_shadow_on_each_record_is_its_single_option_frames(contexts, shots, native):
    """case C with ngp_set_sun_nerf_shadow on too: the sun-shadow record is that of the frame with the sun shadow alone, the 12-float record
    and the hit record those of the frame without the sun shadow, and depth that of every frame, as bytes; the NeRF's shadow does not reach
    the hit. A second run gives the same bytes."""
    c, s = contexts["C"], shots["C"]
    c.set_sun_nerf_shadow(SUN_NERF)
    try:
        c.render(_cam(native), _opts(native))
        sun_rec = c.frame_sun_shadow(W * H)
        c.set_mesh_reflection(ON)
        refl_sun = c.render(_cam(native), _opts(native), want_depth=True)
        assert c.frame_sun_shadow(W * H).tobytes() == sun_rec.tobytes()
        c.set_mesh_reflection_meshes(True)
        both = c.render(_cam(native), _opts(native), want_depth=True)
        assert c.frame_sun_shadow(W * H).tobytes() == sun_rec.tobytes() and (sun_rec[:, 3] > 0).sum() > 20
        assert c.frame_mesh_reflection(W * H).tobytes() == s["on_record"].tobytes() and _hits(c).tobytes() == s["hits"].tobytes()
        assert both[1].tobytes() == s["on"][1].tobytes() and not _same(both, refl_sun) and not _same(both, s["on"])
        hit = s["hits"][..., 7] != 0
        assert both[0][~hit].tobytes() == refl_sun[0][~hit].tobytes()
        again = c.render(_cam(native), _opts(native), want_depth=True)
        assert _same(again, both) and _hits(c).tobytes() == s["hits"].tobytes()
        with pytest.raises(RuntimeError, match="n_pixels"):
            _hits(c, W * H - 1)
    finally:
        c.set_mesh_reflection(None)
        c.set_mesh_reflection_meshes(False)
        c.set_sun_nerf_shadow(None)
    assert _same(_render(c, native, ON, True), s["on"])  # two runs, the sun shadow off again


def test_two_samples_per_pixel(contexts, native):
    """case C, 2 spp with jittered samples: the hit record is the last sample's, which is that of the one-sample frame of that sample index; no
    pixel is darker than without the sub-option and depth is the same"""
    c = contexts["C"]
    cam = _cam(native, snap=False)
    off = _render(c, native, ON, False, cam=cam, spp=2)
    c.set_mesh_reflection(ON)
    c.set_mesh_reflection_meshes(True)
    try:
        on = c.render(cam, _opts(native, spp=2), want_depth=True)
        rec2 = _hits(c)
        c.render(_cam(native, snap=False, spp_index=1), _opts(native))
        rec_last = _hits(c)
        c.render(cam, _opts(native))
        rec_first = _hits(c)
    finally:
        c.set_mesh_reflection(None)
        c.set_mesh_reflection_meshes(False)
    assert rec2.tobytes() == rec_last.tobytes() and rec2.tobytes() != rec_first.tobytes() and (rec2[:, 7] != 0).sum() >= 100
    assert not _same(on, off) and on[1].tobytes() == off[1].tobytes() and np.all(on[0] >= off[0])


def _tiles(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // 8) * ((w + 7) // 8) + xs // 8, (xs % 8) + 8 * (ys % 8)


def test_shards_and_packed_shards_cover_the_frame(contexts, native):
    """case C, three shards in image layout and tile-packed (60 x 44: partial tiles on both axes) against the whole frame: colour, depth and
    the hit record, as bytes"""
    import torch

    c = contexts["C"]
    w, h, world = 60, 44, 3
    cam = _cam(native, w=w, h=h)
    tile, slot = _tiles(w, h)
    c.set_mesh_reflection(ON)
    c.set_mesh_reflection_meshes(True)
    try:
        full, full_depth = c.render(cam, _opts(native), want_depth=True)
        full_rec = _hits(c, w * h).reshape(h, w, 8)
        assert (full_rec[..., 7] != 0).sum() > 100 and (full[..., 3] == 1).sum() > 500
        total, total_depth, total_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        packed, packed_depth, packed_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        for rank in range(world):
            mine = tile % world == rank
            part, part_depth = c.render(cam, _opts(native, shard_index=rank, shard_count=world), want_depth=True)
            rec = _hits(c, w * h).reshape(h, w, 8)
            assert not np.any(part[~mine]) and not np.any(rec[~mine])
            total[mine], total_depth[mine], total_rec[mine] = part[mine], part_depth[mine], rec[mine]
            n = native.load_library().ngp_packed_tiles(w, h, rank, world) * 64
            rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
            c.render_device(cam, _opts(native, shard_index=rank, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
            rec = _hits(c, n)  # (synchronises the context's stream)
            src = (tile // world) * 64 + slot
            packed[mine], packed_depth[mine], packed_rec[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]], rec[src[mine]]
    finally:
        c.set_mesh_reflection(None)
        c.set_mesh_reflection_meshes(False)
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes() and total_rec.tobytes() == full_rec.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes() and packed_rec.tobytes() == full_rec.tobytes()


def test_two_devices_render_the_one_device_frame(shots, native, scene_unit):
    """a context of two devices (the same ordinal twice): the flag reaches the replica with the geometry, each device shades the hits of its
    share, the frame is the one-device frame as bytes; the hit record is the primary's tile-packed share"""
    s = shots["C"]
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        _load(multi, hc.scene("C"))
        multi.set_geometry_opts(sun_dir=hc.SUN["C"])
        assert _same(_render(multi, native, ON, False), s["off"])
        multi.set_mesh_reflection(ON)
        multi.set_mesh_reflection_meshes(True)
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), s["on"])
        n = native.load_library().ngp_packed_tiles(W, H, 0, 2) * 64
        rec = _hits(multi, n)
        tile, slot = _tiles(W, H)
        mine = tile % 2 == 0
        assert rec[((tile // 2) * 64 + slot)[mine]].tobytes() == s["hits"][mine].tobytes()
        multi.set_mesh_reflection_meshes(False)
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), s["off"])  # and off reaches it too
    finally:
        multi.close()


def test_frame_on_a_callers_stream(contexts, shots, native):
    """ngp_render_device on a caller's stream, then the caller's own synchronise: the same bytes"""
    import torch

    c, s = contexts["C"], shots["C"]
    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    c.set_mesh_reflection(ON)
    c.set_mesh_reflection_meshes(True)
    try:
        c.render_device(_cam(native), _opts(native), rgba.data_ptr(), dep.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert rgba.cpu().numpy().tobytes() == s["on"][0].tobytes() and dep.cpu().numpy().tobytes() == s["on"][1].tobytes()
        assert _hits(c).tobytes() == s["hits"].tobytes()
    finally:
        c.set_mesh_reflection(None)
        c.set_mesh_reflection_meshes(False)
    assert _same(_render(c, native, ON, False), s["off"])  # (back on the context's own stream)


# ------------------------------------------------------------------------------------------------------------------ bindings
# for the command line's level default camera at z = 2: the floor raised to just under the object's base plate (test_mesh_reflection_gpu.py's),
# and a wall across the far side of the floor that faces the camera and the default sun: the floor's mirror rays climb away from the camera into it
LEVEL_SCENE = [(hc.scene("A")[0][0], (0.0, -0.405, 0.0)), ((mc.cube().astype(np.float64) * np.array([1.0, 1.0, 0.04])).astype(np.float32), (0.0, 0.1, -0.95))]


def _write_scene(tmp_path, c, meshes, name):
    """the meshes as .obj files, the unit NeRF as a snapshot, and the scene file that names them"""
    mi = pkg("meshio")
    entries = []
    for i, (tris, center) in enumerate(meshes):
        mi.save_obj(str(tmp_path / ("%s%d.obj" % (name, i))), tris)
        entries.append({"center": [float(x) for x in center], "path": "%s%d.obj" % (name, i), "type": "Mesh"})
    c.save_snapshot_file(str(tmp_path / "unit.ingp"))
    entries.append({"center": [0, 0, 0], "path": "unit.ingp", "type": "Nerf"})
    path = tmp_path / ("%s_geometry_scene.json" % name)  # (the Testbed takes a scene file for a Geometry scene by the word in its name)
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def test_pyngp_and_command_line(tmp_path, contexts, shots, native):
    """testbed.mesh_reflection_meshes (default False) gives the native frames as bytes, and --mesh_reflection_meshes writes the frame the
    property gives, to the 8 bits of the file"""
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    scene = _write_scene(tmp_path, contexts["C"], hc.scene("C"), "wall")

    def testbed(camera):
        tb = pyngp.Testbed()
        tb.load_training_data(scene if camera else level)
        assert tb.mode == pyngp.TestbedMode.Geometry
        tb.background_color = [0.0, 0.0, 0.0, 0.0]
        tb.render_mode = pyngp.RenderMode.Shade
        if camera:  # (else the default camera and sun, the command line's)
            tb.snap_to_pixel_centers = True
            tb.sun_dir = [float(x) for x in hc.SUN["C"]]
            tb.fov_axis = 0
            tb.relative_focal_length = [hc.FOCAL[0] / W, hc.FOCAL[1] / W]
            tb.camera_matrix = hc.CAMERA
        return tb

    tb = testbed(True)
    assert tb.mesh_reflection_meshes is False
    tb.mesh_reflection_meshes = True
    assert tb.render(W, H, 1, True).tobytes() == shots["C"]["plain"][0].tobytes()  # (the reflection is off: the sub-option alone does nothing)
    tb.mesh_reflection = True
    assert tb.render(W, H, 1, True).tobytes() == shots["C"]["on"][0].tobytes()
    tb.mesh_reflection_meshes = False
    assert tb.render(W, H, 1, True).tobytes() == shots["C"]["off"][0].tobytes()
    del tb
    # the command line writes the frame of the default camera: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round
    # the last bit)
    level = _write_scene(tmp_path, contexts["C"], LEVEL_SCENE, "level")
    shots_ = {}
    for meshes in (False, True):
        tb = testbed(False)
        tb.mesh_reflection, tb.mesh_reflection_strength, tb.mesh_reflection_meshes = True, 4.0, meshes
        shots_[meshes] = tb.render(W, H, 1, True)
        del tb

    def as_png(frame):
        a = np.clip(frame[..., 3:4], 0, 1)
        v = np.clip(np.where(a > 0, frame[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
        srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
        return np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)

    expect = {k: as_png(v) for k, v in shots_.items()}
    print("\ncommand line: the flag changes %d of %d pixels of the file" % ((expect[True] != expect[False]).any(-1).sum(), W * H))
    assert (expect[True] != expect[False]).any(-1).sum() > 20
    exe = pkg("build").build_main()
    for meshes in (True, False):
        out = tmp_path / ("shot%d.png" % meshes)
        flags = ["--mesh_reflection", "--mesh_reflection_strength", "4.0"] + (["--mesh_reflection_meshes"] if meshes else [])
        res = subprocess.run([exe, "--no-gui", "--scene", level, "--render_mode", "Shade", "--width", str(W), "--height", str(H), "--screenshot", str(out)] + flags,
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr
        png = np.asarray(Image.open(out)).astype(np.int64)
        assert png.shape == (H, W, 4) and np.abs(png - expect[meshes]).max() <= 1 and (png != expect[meshes]).mean() < 0.01, (meshes, np.abs(png - expect[meshes]).max())
