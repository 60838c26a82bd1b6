"""The meshes in front of the sun on the NeRF on the GPU (include/ngp_hip.h, "sun: the meshes in front of the sun on the NeRF"): the
identities the contract promises as bytes (strength 0 pins the new composite to the NeRF pass's own on every pixel), the per-pixel record
against the float64 reference, the colour against the restated composite, the effect, and the structure around it: determinism, samples,
shards, devices, streams, statistics, the other shadow option at the same time, and the bindings. Tolerances: TIE_EPS and the float32
form's own deviation for p (test_irradiance_sun_shadow_gpu.py's rule), mesh_sun_nerf_shadow_cases.frame_bound for colour; none comes from
the code under test. The measured figures are in DESIGN 3.16.

n, the NeRF's own premultiplied pixel, is read from a second context: the same model without meshes, its render box set to the box the
meshes give the first one, rendered in Geometry mode. Its NeRF pass marches the rays the hybrid frame's does."""
import json
import subprocess

import numpy as np
import pytest

from conftest import pkg

import mesh_cases as mc
import mesh_reference as mref
import mesh_sun_nerf_shadow_cases as sc
import mesh_volume_cases as mv
import nerf_mesh_shadow_cases as nc

pytestmark = pytest.mark.gpu

W, H = nc.WIDTH, nc.HEIGHT
ON = dict(strength=nc.STRENGTH, bias=nc.BIAS)
NONE = dict(strength=0.0, bias=nc.BIAS)
FULL = dict(strength=1.0, bias=nc.BIAS)
VOLUME_BOX = (np.float32([-0.1, -0.2, -0.1]), np.float32([1.1, 0.7, 1.1]))
RICH = dict(ambientcolor=mv.SKY_AMBIENT, up_dir=(1.0, 0.0, 0.0), metallic=0.3, clearcoat=0.5, sheen=0.5)  # every term of the BRDF and the sky at work


def _load(c, scene):
    c.clear_meshes()
    for tris, center in scene:
        c.add_mesh(tris, center)


def _opts(native, mode=None, **kw):
    return native.make_opts(**dict(dict(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0), render_mode=native.RENDER_SHADE if mode is None else mode), **kw))


def _cam(native, w=W, h=H, **kw):
    return native.make_camera(nc.CAMERA, w, h, nc.FOCAL, **kw)


def _render(c, native, shadow, cam=None, **kw):
    c.set_mesh_shadow_on_nerf(shadow)
    try:
        return c.render(cam or _cam(native), _opts(native, **kw), want_depth=True)
    finally:
        c.set_mesh_shadow_on_nerf(None)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF over the floor and under the plate, the default geometry options (sun (1, 1, 1))"""
    c = native.Context(0)
    c.set_model(scene_unit)
    _load(c, nc.scene())
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare(gpu_ctx, native):
    """the meshes alone"""
    c = native.Context(0)
    _load(c, nc.scene())
    c.set_geometry_opts()
    yield c
    c.close()


def _frames(hybrid, bare, native, scene_unit, matrix):
    """the frames of one view: option off, on with its record, statistics and time, on with strength 1, the meshes alone (m), the model
    alone inside the meshes' box (n, with what the depth test culls taken out)"""
    cam = native.make_camera(matrix, W, H, nc.FOCAL)
    off = _render(hybrid, native, None, cam=cam)
    off_stats = hybrid.render_stats()
    hybrid.set_mesh_shadow_on_nerf(ON)
    on = hybrid.render(cam, _opts(native), want_depth=True)
    record = hybrid.frame_mesh_shadow(W * H).reshape(H, W, 4)
    on_stats, shadow_ms = hybrid.render_stats(), hybrid.frame_mesh_shadow_ms()
    hybrid.set_mesh_shadow_on_nerf(None)
    lo, hi = hybrid.mesh_info()["aabb"]
    alone = native.Context(0)
    try:
        alone.set_model(dict(scene_unit, render_aabb=(tuple(float(x) for x in lo), tuple(float(x) for x in hi))))
        nerf = alone.render(cam, _opts(native), want_depth=True)
    finally:
        alone.close()
    m, m_depth = _render(bare, native, None, cam=cam)
    # (a ray that enters no mesh's box leaves an opaque black pixel at no depth, which the NeRF pass reads as MAX_DEPTH: nothing lies behind it)
    behind = m_depth >= np.float32(0.01)
    n = np.where((behind & (nerf[1] > m_depth))[..., None], np.float32(0), nerf[0])  # what the depth test culls never reaches the frame
    # (a pixel of alpha <= 0.2 leaves no depth behind: over a mesh, whether the test culled it cannot be read from these frames)
    unknown = (nerf[0][..., 3] > 0) & (nerf[0][..., 3] <= np.float32(nc.OWNER_ALPHA)) & behind
    return dict(unknown=unknown, behind=behind, off=off, on=on, record=record, off_stats=off_stats, on_stats=on_stats, shadow_ms=shadow_ms, full=_render(hybrid, native, FULL, cam=cam), m=m,
                m_depth=m_depth, n=n)


@pytest.fixture(scope="module")
def frames(hybrid, bare, native, scene_unit):
    """the case's view"""
    return _frames(hybrid, bare, native, scene_unit, nc.CAMERA)


# ------------------------------------------------------------------------------------------------------- identities as bytes
def test_identities_as_bytes(hybrid, bare, frames, native, scene_unit):
    """off after on, strength 0, NeRF mode, the G-buffer render modes, a context of meshes alone, Geometry mode without meshes and a model
    without density: each is the option-off frame, colour and depth. Strength 0.5 is not, and its depth is."""
    off, on = frames["off"], frames["on"]
    assert (off[0][..., 3] > 0).sum() > 500 and on[0].tobytes() != off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
    assert frames["full"][1].tobytes() == off[1].tobytes()
    assert _same(_render(hybrid, native, None), off)                      # off after on
    assert hybrid.mesh_shadow_on_nerf() is None
    assert _same(_render(hybrid, native, NONE), off)                      # strength 0
    for mode in (native.RENDER_SHADE, native.RENDER_AO, native.RENDER_POSITIONS, native.RENDER_DEPTH, native.RENDER_COST, native.RENDER_NORMALS):
        kw = dict(testbed_mode=native.MODE_NERF, mode=mode)
        a, b = _render(hybrid, native, ON, **kw), _render(hybrid, native, None, **kw)
        assert _same(a, b) and (a[0][..., 3] > 0).sum() > 300, mode
        with pytest.raises(RuntimeError, match="ran no mesh shadow pass"):
            hybrid.frame_mesh_shadow(W * H)
        assert hybrid.frame_mesh_shadow_ms() == 0
    assert _same(_render(bare, native, ON), (frames["m"], frames["m_depth"]))  # no model
    with pytest.raises(RuntimeError, match="ran no mesh shadow pass"):
        bare.frame_mesh_shadow(W * H)
    hybrid.clear_meshes()
    try:
        assert _same(_render(hybrid, native, ON), _render(hybrid, native, None))  # Geometry mode without meshes
    finally:
        _load(hybrid, nc.scene())
    empty = native.Context(0)
    try:
        empty.set_model(dict(scene_unit, density_grid=np.zeros_like(scene_unit["density_grid"])))
        _load(empty, nc.scene())
        empty.set_geometry_opts()
        a, b = _render(empty, native, ON), _render(empty, native, None)
        assert _same(a, b) and (a[0][..., 3] > 0).sum() > 500
    finally:
        empty.close()


@pytest.mark.parametrize("mode", ["Shade", "ShadeEnvMap", "ShadeGridEnvMap", "ShadeIrradianceVolume", "ShadeIrradianceVolumeVisible"])
def test_strength_zero_is_the_option_off_frame(mode, hybrid, native):
    """f = 1 on every pixel: the composite of the new kernel is the NeRF pass's own, as bytes, in each shade mode, with geometry options
    that put every term of the BRDF to work; strength 0.5 changes the frame and not its depth"""
    hybrid.set_geometry_opts(**RICH)
    try:
        if mode == "ShadeEnvMap":
            hybrid.compute_envmap(n_theta=16, n_phi=8)
        elif mode == "ShadeGridEnvMap":
            hybrid.compute_envmap_grid(2, 2, 16, 8)
        elif mode.startswith("ShadeIrradianceVolume"):
            hybrid.compute_irradiance_volume((3, 2, 3), VOLUME_BOX, 8, 8, occlude_by_meshes=False)
            if mode.endswith("Visible"):
                hybrid.compute_irradiance_volume_visibility(n_u=8, n_v=8, sharpness_log2=4, max_distance=0.0, normal_bias=0.01)
        kw = dict(mode={"Shade": native.RENDER_SHADE, "ShadeEnvMap": native.RENDER_SHADE_ENVMAP, "ShadeGridEnvMap": native.RENDER_SHADE_GRID_ENVMAP}.get(mode, native.RENDER_SHADE_IRRADIANCE_VOLUME))
        off, none, on = _render(hybrid, native, None, **kw), _render(hybrid, native, NONE, **kw), _render(hybrid, native, ON, **kw)
        print("\n%s: %d pixels with colour; the shadow changes %d" % (mode, (off[0][..., :3].max(-1) > 1e-3).sum(), (np.abs(on[0] - off[0]).max(-1) > 0).sum()))
        assert (off[0][..., 3] > 0).sum() > 500 and np.unique(off[0][..., 0]).size > 100
        assert _same(none, off)
        assert on[0].tobytes() != off[0].tobytes() and on[1].tobytes() == off[1].tobytes() and np.all(on[0] <= off[0])
    finally:
        hybrid.clear_irradiance_volume()
        hybrid.set_geometry_opts()


# ---------------------------------------------------------------------------------------------------------------- the record
def test_record_matches_the_reference(frames):
    """(a) the pixels with a record are those where the NeRF's own alpha, in front of the mesh depth, exceeds 0.2; every other entry is
    zero; (b) |p - p64| <= TIE_EPS + GPU_FACTOR x the float32 form's deviation, p64 the float64 point at the frame's own depth output;
    (c) blocked equals mesh_reference.global_nearest from the recorded p itself on every ray the float64 tracer calls safe; (d) the case's
    conditions hold on the GPU's own record"""
    rec, depth = frames["record"], frames["on"][1]
    owner = rec[..., 3] != 0
    assert np.isfinite(rec).all() and set(np.unique(rec[..., 3])) <= {0.0, 1.0, 2.0} and np.all(rec[~owner] == 0)
    assert np.array_equal(owner, frames["n"][..., 3] > np.float32(nc.OWNER_ALPHA))                       # (a)
    sh = nc.shadow(np.where(owner, 1.0, 0.0), depth, nc.meshes())
    dp = np.abs(rec[..., :3].astype(np.float64) - sh["p"])[owner].max()
    allow = mref.TIE_EPS + mc.GPU_FACTOR * sh["p_dev"]
    blocked64, unsafe = nc.blocked_from(rec[..., :3][owner], nc.meshes())
    blocked = rec[..., 3][owner] == 2
    print("\n%d owners, blocked %d, open %d, unsafe %d; |dp| %.2e (allowed %.2e, of it the float32 form x %g: %.2e); blocked differs on %d safe rays"
          % (owner.sum(), blocked.sum(), (~blocked).sum(), unsafe.sum(), dp, allow, mc.GPU_FACTOR, mc.GPU_FACTOR * sh["p_dev"], (blocked != blocked64)[~unsafe].sum()))
    assert dp <= allow, (dp, allow)                                                                       # (b)
    assert np.array_equal(blocked[~unsafe], blocked64[~unsafe])                                           # (c)
    assert owner.sum() >= nc.MIN_OWNERS and blocked.sum() >= nc.BLOCKED_SHARE * owner.sum() and (~blocked).sum() >= nc.OPEN_SHARE * owner.sum()  # (d)
    assert unsafe.sum() <= mc.UNSAFE_CAP * owner.sum()


# ---------------------------------------------------------------------------------------------------------------- the colour
def test_colour_is_the_restated_composite(frames):
    """f from the record. Where no mesh lies behind the pixel the on frame's rgb is fl(off rgb x f) and its alpha the off frame's, as
    bytes. Where the floor lies behind it the on frame is fl(n f) + m (1 - a), n from the frame of the model alone and m from the frame of
    the meshes alone, within mesh_sun_nerf_shadow_cases.frame_bound. Pixels whose record says open or nothing are the off frame's bytes."""
    (off, off_depth), (on, on_depth) = frames["off"], frames["on"]
    rec, n, m = frames["record"], frames["n"], frames["m"]
    f = np.where(rec[..., 3] == 2, np.float32(1) - np.float32(nc.STRENGTH), np.float32(1)).astype(np.float32)
    assert on_depth.tobytes() == off_depth.tobytes()
    nothing_behind = ~frames["behind"]
    assert np.all(m[..., :3][nothing_behind] == 0)
    want = np.concatenate([(off[..., :3] * f[..., None]).astype(np.float32), off[..., 3:]], -1)
    assert (nothing_behind & (rec[..., 3] == 2)).sum() > 20 and on[nothing_behind].tobytes() == want[nothing_behind].tobytes()
    floor = ~nothing_behind & ~frames["unknown"]
    want = nc.composite(n, m, f)
    bound = sc.frame_bound(want[..., :3].astype(np.float64))
    ratio = np.abs(on[..., :3].astype(np.float64) - want[..., :3])[floor] / bound[floor]
    over_floor = floor & (n[..., 3] > 0)
    exact = on.view(np.uint32) == want.view(np.uint32)
    print("\npixels with nothing behind %d (blocked %d), over the floor %d (the NeRF on %d of them, blocked %d); largest colour deviation / bound %.3g; equal as bytes on %d of %d pixels (%d left out: alpha <= 0.2 over the floor)"
          % (nothing_behind.sum(), (nothing_behind & (rec[..., 3] == 2)).sum(), floor.sum(), over_floor.sum(), (over_floor & (rec[..., 3] == 2)).sum(), ratio.max(), exact.all(-1)[~frames["unknown"]].sum(), (~frames["unknown"]).sum(), frames["unknown"].sum()))
    assert over_floor.sum() >= 50
    assert ratio.max() <= 1.0, ratio.max()
    assert np.array_equal(on[..., 3][floor], want[..., 3][floor])
    known = ~frames["unknown"]
    assert on[known].tobytes() == want[known].tobytes()  # measured on the MI355X: the comparison holds as bytes, so bytes are asserted
    same = rec[..., 3] != 2
    assert on[same].tobytes() == off[same].tobytes()
    assert nc.composite(n, m, np.ones_like(f))[known].tobytes() == off[known].tobytes()  # and the off frame is the same composite with f = 1


def test_second_view_shadows_the_nerf_over_the_floor(hybrid, bare, native, scene_unit):
    """in the case's view every blocked pixel has nothing behind it. From higher up the floor lies behind part of the shadowed NeRF (measured:
    47 of 256 blocked pixels, the NeRF opaque on all 47): the on frame is fl(n f) + m (1 - a) as bytes, f from the record, and blocked is
    the float64 tracer's from the recorded p on safe rays"""
    fr = _frames(hybrid, bare, native, scene_unit, nc.CAMERA_ABOVE)
    on, off, rec, n, m = fr["on"][0], fr["off"][0], fr["record"], fr["n"], fr["m"]
    blocked, known = rec[..., 3] == 2, ~fr["unknown"]
    f = np.where(blocked, np.float32(1) - np.float32(nc.STRENGTH), np.float32(1)).astype(np.float32)
    mixed = blocked & fr["behind"] & (n[..., 3] < 1) & (m[..., :3].sum(-1) > 0)
    print("\nsecond view: owners %d, blocked %d, of them over the floor %d, with the floor showing through %d" % ((rec[..., 3] != 0).sum(), blocked.sum(), (blocked & fr["behind"]).sum(), mixed.sum()))
    assert (blocked & fr["behind"]).sum() >= 10
    assert on[known].tobytes() == nc.composite(n, m, f)[known].tobytes() and fr["on"][1].tobytes() == fr["off"][1].tobytes()
    assert on[~blocked].tobytes() == off[~blocked].tobytes() and np.all(on <= off) and on.tobytes() != off.tobytes()
    owner = rec[..., 3] != 0
    blocked64, unsafe = nc.blocked_from(rec[..., :3][owner], nc.meshes())
    assert np.array_equal(blocked[owner][~unsafe], blocked64[~unsafe]) and unsafe.sum() <= mc.UNSAFE_CAP * owner.sum()


def test_blocked_pixels_lose_the_share(frames):
    """the test that fails without the option. On blocked pixels the NeRF's part of the pixel (the pixel less m (1 - a), which is the whole
    pixel where no mesh lies behind it) sums to (1 - strength) of the off frame's, within frame_bound a channel; with strength 1 the blocked
    pixels with nothing behind them are black; no pixel is brighter than off"""
    off, on, full = frames["off"][0], frames["on"][0], frames["full"][0]
    rec, n, m = frames["record"], frames["n"], frames["m"]
    blocked = rec[..., 3] == 2
    behind = (m.astype(np.float64) * (1.0 - n[..., 3:4].astype(np.float64)))[..., :3]
    part_on, part_off = on[..., :3].astype(np.float64) - behind, off[..., :3].astype(np.float64) - behind
    bound = 3 * sc.frame_bound(off[..., :3].astype(np.float64)).max(-1)
    err = np.abs(part_on.sum(-1) - (1.0 - nc.STRENGTH) * part_off.sum(-1))
    lit = blocked & (part_off.sum(-1) > 0.05)
    print("\nblocked %d (with colour %d); largest |sum on - (1 - strength) sum off| / bound %.3g; mean rgb sum on blocked pixels off %.4f, on %.4f, strength 1 %.4f"
          % (blocked.sum(), lit.sum(), (err / bound)[blocked].max(), off[..., :3].sum(-1)[blocked].mean(), on[..., :3].sum(-1)[blocked].mean(), full[..., :3].sum(-1)[blocked].mean()))
    assert lit.sum() >= 50
    assert np.all(err[blocked] <= bound[blocked])
    assert np.all(on[..., :3].sum(-1)[lit] < 0.75 * off[..., :3].sum(-1)[lit] + behind.sum(-1)[lit])
    alone = blocked & ~frames["behind"]
    assert alone.sum() > 20 and np.all(full[..., :3][alone] == 0) and np.all(off[..., :3][alone].sum(-1) > 0)
    assert full[..., 3].tobytes() == off[..., 3].tobytes() and np.all(on <= off) and np.all(full <= on)


# ----------------------------------------------------------------------------------------------------------------- structure
def test_two_runs_statistics_and_time(hybrid, frames, native):
    """a second run is the first as bytes, record included; the frame's statistics are the off frame's; the pass's time is positive and
    finite, and 0 after a frame without it"""
    hybrid.set_mesh_shadow_on_nerf(ON)
    try:
        again = hybrid.render(_cam(native), _opts(native), want_depth=True)
        assert _same(again, frames["on"]) and hybrid.frame_mesh_shadow(W * H).tobytes() == frames["record"].tobytes()
        with pytest.raises(RuntimeError, match="n_pixels"):
            hybrid.frame_mesh_shadow(W * H - 1)
    finally:
        hybrid.set_mesh_shadow_on_nerf(None)
    on, off = frames["on_stats"], frames["off_stats"]
    print("\nstatistics on %s\n           off %s\nmesh shadow kernel %.4f ms" % (on, off, frames["shadow_ms"]))
    for k in ("n_rays", "n_rays_alive_after_init", "n_rays_hit", "n_samples"):
        assert on[k] == off[k], k
    assert off["n_samples"] > 0
    assert np.isfinite(frames["shadow_ms"]) and frames["shadow_ms"] > 0
    _render(hybrid, native, None)
    assert hybrid.frame_mesh_shadow_ms() == 0
    with pytest.raises(RuntimeError, match="ran no mesh shadow pass"):
        hybrid.frame_mesh_shadow(W * H)


def test_two_samples_per_pixel(hybrid, native):
    """2 spp with jittered samples: every sample is shadowed on its own ray and the record is the last sample's, which is the record of the
    one-sample frame of that sample index; with strength 0 the frame is the option-off frame as bytes"""
    cam = _cam(native, snap=False)
    off = _render(hybrid, native, None, cam=cam, spp=2)
    assert _same(_render(hybrid, native, NONE, cam=cam, spp=2), off)
    hybrid.set_mesh_shadow_on_nerf(ON)
    try:
        on = hybrid.render(cam, _opts(native, spp=2), want_depth=True)
        rec2 = hybrid.frame_mesh_shadow(W * H)
        last = hybrid.render(_cam(native, snap=False, spp_index=1), _opts(native), want_depth=True)
        rec_last = hybrid.frame_mesh_shadow(W * H)
        hybrid.render(cam, _opts(native))
        rec_first = hybrid.frame_mesh_shadow(W * H)
    finally:
        hybrid.set_mesh_shadow_on_nerf(None)
    assert rec2.tobytes() == rec_last.tobytes() and rec2.tobytes() != rec_first.tobytes()
    assert on[0].tobytes() != off[0].tobytes() and on[1].tobytes() == off[1].tobytes() and np.all(on[0] <= off[0])
    owner = rec2[:, 3] != 0
    sh = nc.shadow(np.where(owner, 1.0, 0.0).reshape(H, W), last[1], nc.meshes(), pixel_offset=tuple(float(x) for x in _pixel_offset(native, 1)))
    assert owner.sum() >= nc.MIN_OWNERS and np.abs(rec2[:, :3].astype(np.float64) - sh["p"].reshape(-1, 3))[owner].max() <= mref.TIE_EPS + mc.GPU_FACTOR * sh["p_dev"]


def _pixel_offset(native, spp_index):
    """the sample's offset inside its pixel, as the oracle forms it"""
    import oracle as orc

    return orc.Oracle().pixel_offset(spp_index)


def _tiles(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // 8) * ((w + 7) // 8) + xs // 8, (xs % 8) + 8 * (ys % 8)


def test_shards_and_packed_shards_cover_the_frame(hybrid, native):
    """three shards in image layout and tile-packed (60 x 44: partial tiles on both axes) against the whole frame: colour, depth and the
    record, as bytes"""
    import torch

    w, h, world = 60, 44, 3
    cam = _cam(native, w=w, h=h)
    tile, slot = _tiles(w, h)
    hybrid.set_mesh_shadow_on_nerf(ON)
    try:
        full, full_depth = hybrid.render(cam, _opts(native), want_depth=True)
        full_rec = hybrid.frame_mesh_shadow(w * h).reshape(h, w, 4)
        assert (full_rec[..., 3] == 2).sum() > 20 and (full_rec[..., 3] == 1).sum() > 20 and (full[..., 3] > 0).sum() > 500
        total, total_depth, total_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        packed, packed_depth, packed_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        for r in range(world):
            mine = tile % world == r
            part, part_depth = hybrid.render(cam, _opts(native, shard_index=r, shard_count=world), want_depth=True)
            rec = hybrid.frame_mesh_shadow(w * h).reshape(h, w, 4)
            assert not np.any(part[~mine]) and not np.any(rec[~mine])
            total[mine], total_depth[mine], total_rec[mine] = part[mine], part_depth[mine], rec[mine]
            n = native.load_library().ngp_packed_tiles(w, h, r, world) * 64
            rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
            hybrid.render_device(cam, _opts(native, shard_index=r, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
            rec = hybrid.frame_mesh_shadow(n)  # (synchronises the context's stream)
            src = (tile // world) * 64 + slot
            packed[mine], packed_depth[mine], packed_rec[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]], rec[src[mine]]
    finally:
        hybrid.set_mesh_shadow_on_nerf(None)
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes() and total_rec.tobytes() == full_rec.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes() and packed_rec.tobytes() == full_rec.tobytes()


def test_two_devices_render_the_one_device_frame(frames, native, scene_unit):
    """a context of two devices (the same ordinal twice): the option reaches the replica with the geometry, each device shadows its share,
    the frame is the one-device frame as bytes; the record is the primary's tile-packed share"""
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        _load(multi, nc.scene())
        multi.set_geometry_opts()
        assert _same(_render(multi, native, None), frames["off"])
        multi.set_mesh_shadow_on_nerf(ON)
        two = multi.render(_cam(native), _opts(native), want_depth=True)
        assert _same(two, frames["on"])
        n = native.load_library().ngp_packed_tiles(W, H, 0, 2) * 64
        rec = multi.frame_mesh_shadow(n)
        tile, slot = _tiles(W, H)
        mine = tile % 2 == 0
        assert rec[((tile // 2) * 64 + slot)[mine]].tobytes() == frames["record"][mine].tobytes()
        st = multi.render_stats()
        for k in ("n_rays", "n_rays_hit", "n_samples"):
            assert st[k] == frames["off_stats"][k], k
        multi.set_mesh_shadow_on_nerf(None)
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), frames["off"])  # and off reaches it too
    finally:
        multi.close()


def test_frame_on_a_callers_stream(hybrid, frames, native):
    """ngp_render_device on a caller's stream, then the caller's own synchronise: the same bytes"""
    import torch

    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    hybrid.set_mesh_shadow_on_nerf(ON)
    try:
        hybrid.render_device(_cam(native), _opts(native), rgba.data_ptr(), dep.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert rgba.cpu().numpy().tobytes() == frames["on"][0].tobytes() and dep.cpu().numpy().tobytes() == frames["on"][1].tobytes()
        assert hybrid.frame_mesh_shadow(W * H).tobytes() == frames["record"].tobytes()
    finally:
        hybrid.set_mesh_shadow_on_nerf(None)
    assert _same(_render(hybrid, native, None), frames["off"])  # (back on the context's own stream)


def test_both_shadow_options_at_once(hybrid, frames, native):
    """ngp_set_sun_nerf_shadow on at the same time: the mesh pass is the split one, the NeRF pass and so the record are untouched, and the
    frame is neither single-option frame"""
    hybrid.set_sun_nerf_shadow(True)
    try:
        sun_only = hybrid.render(_cam(native), _opts(native), want_depth=True)
        both = _render(hybrid, native, ON)
        hybrid.set_mesh_shadow_on_nerf(ON)
        hybrid.render(_cam(native), _opts(native))
        rec = hybrid.frame_mesh_shadow(W * H)
        assert hybrid.frame_sun_shadow(W * H).shape == (W * H, 4) and hybrid.frame_mesh_shadow_ms() > 0
    finally:
        hybrid.set_sun_nerf_shadow(None)
        hybrid.set_mesh_shadow_on_nerf(None)
    assert rec.tobytes() == frames["record"].tobytes()
    assert both[1].tobytes() == frames["on"][1].tobytes()
    assert both[0].tobytes() != frames["on"][0].tobytes() and both[0].tobytes() != sun_only[0].tobytes() and sun_only[0].tobytes() != frames["off"][0].tobytes()
    assert np.all(both[0] <= frames["on"][0]) and np.all(both[0] <= sun_only[0])


# ------------------------------------------------------------------------------------------------------------------ bindings
def _write_scene(tmp_path, hybrid, name="plate", plate_center=nc.PLATE_CENTER):
    """the meshes as .obj files, the unit NeRF as a snapshot, and the scene file that names them"""
    mi = pkg("meshio")
    entries = []
    for i, (tris, center) in enumerate(nc.scene()):
        mi.save_obj(str(tmp_path / ("mesh%d.obj" % i)), tris)
        entries.append({"center": [float(x) for x in (center if i == 0 else plate_center)], "path": "mesh%d.obj" % i, "type": "Mesh"})
    hybrid.save_snapshot_file(str(tmp_path / "unit.ingp"))
    entries.append({"center": [0, 0, 0], "path": "unit.ingp", "type": "Nerf"})
    path = tmp_path / (name + "_geometry_scene.json")  # (the Testbed takes a scene file for a Geometry scene by the word in its name)
    path.write_text(json.dumps({"geometry": entries}))
    return str(path)


def _testbed(pyngp, scene, camera=True):
    tb = pyngp.Testbed()
    tb.load_training_data(scene)
    assert tb.mode == pyngp.TestbedMode.Geometry
    tb.background_color = [0.0, 0.0, 0.0, 0.0]
    tb.render_mode = pyngp.RenderMode.Shade
    if camera:  # (else the default camera, the command line's)
        tb.snap_to_pixel_centers = True
        tb.sun_dir = [1.0, 1.0, 1.0]
        tb.fov_axis = 0
        tb.relative_focal_length = [nc.FOCAL[0] / W, nc.FOCAL[1] / W]
        tb.camera_matrix = nc.CAMERA
    return tb


def test_pyngp_and_command_line(tmp_path, hybrid, native):
    """testbed.mesh_shadow_on_nerf (with its two parameters) gives the native frame as bytes, and --mesh_shadow_on_nerf writes the frame
    the property gives, to the 8 bits of the file"""
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    scene = _write_scene(tmp_path, hybrid)
    cam = _cam(native)
    tb = _testbed(pyngp, scene)
    assert tb.mesh_shadow_on_nerf is False and tb.mesh_shadow_on_nerf_strength == 0.5 and tb.mesh_shadow_on_nerf_bias == np.float32(1e-2)
    off = tb.render(W, H, 1, True)
    tb.mesh_shadow_on_nerf = True
    on = tb.render(W, H, 1, True)
    tb.mesh_shadow_on_nerf_strength, tb.mesh_shadow_on_nerf_bias = 0.75, 0.05
    own = tb.render(W, H, 1, True)
    tb.mesh_shadow_on_nerf = False
    assert tb.render(W, H, 1, True).tobytes() == off.tobytes()
    del tb
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        assert c.render(cam, _opts(native)).tobytes() == off.tobytes()
        c.set_mesh_shadow_on_nerf(True)
        assert c.render(cam, _opts(native)).tobytes() == on.tobytes()
        c.set_mesh_shadow_on_nerf(dict(strength=0.75, bias=0.05))
        assert c.render(cam, _opts(native)).tobytes() == own.tobytes()
    finally:
        c.close()
    changed = np.abs(on - off).max(-1) > 0
    print("\npyngp: mesh_shadow_on_nerf changes %d of %d pixels, by at most %.3g" % (changed.sum(), changed.size, np.abs(on - off).max()))
    assert (on[..., 3] > 0).sum() > 500 and changed.sum() > 100 and on.tobytes() != own.tobytes()
    # the command line writes the frame of the default camera: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit).
    # That camera looks at the cube from +z, the side the case's plate leaves in the sun: the plate moves over it (centre (0.5, 0.7, 0.5)).
    scene = _write_scene(tmp_path, hybrid, "plate_in_front", (0.5, 0.7, 0.5))
    shots = {}
    for shadow in (False, True):
        tb = _testbed(pyngp, scene, camera=False)
        tb.mesh_shadow_on_nerf = shadow
        tb.mesh_shadow_on_nerf_strength = 1.0
        shots[shadow] = tb.render(W, H, 1, True)
        del tb

    def as_png(frame):
        a = np.clip(frame[..., 3:4], 0, 1)
        v = np.clip(np.where(a > 0, frame[..., :3] / np.maximum(a, np.float32(1e-30)), 0), 0, 1).astype(np.float32)
        srgb = np.where(v < np.float32(0.0031308), np.float32(12.92) * v, np.float32(1.055) * np.power(v, np.float32(0.41666)) - np.float32(0.055))
        return np.concatenate([np.rint(np.clip(srgb, 0, 1) * 255), np.rint(a * 255)], -1).astype(np.int64)

    expect = {k: as_png(v) for k, v in shots.items()}
    print("command line: the flag changes %d of %d pixels of the file" % ((expect[True] != expect[False]).any(-1).sum(), W * H))
    assert (expect[True] != expect[False]).any(-1).sum() > 20
    exe = pkg("build").build_main()
    for shadow in (True, False):
        out = tmp_path / ("shot%d.png" % shadow)
        r = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "Shade", "--width", str(W), "--height", str(H), "--screenshot", str(out)]
                           + (["--mesh_shadow_on_nerf", "--mesh_shadow_on_nerf_strength", "1"] if shadow else []), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        png = np.asarray(Image.open(out)).astype(np.int64)
        assert png.shape == (H, W, 4) and np.abs(png - expect[shadow]).max() <= 1 and (png != expect[shadow]).mean() < 0.01, (shadow, np.abs(png - expect[shadow]).max(), (png != expect[shadow]).mean())
        assert (png[..., 3] > 0).sum() > 100
