"""The sun's disk on the GPU (include/ngp_hip.h, "sun: the sun's disk"): the identities the contract promises as bytes, the mesh pixels'
record against the float64 tracer, their colour against the restated shading, the NeRF pixels' record and their composite as bytes, and
the structure around it: samples, shards, devices, streams, the pass's time, refusals, both kernel layouts and the bindings.

Tolerances: TIE_EPS and the float32 form's own deviation for q and p (test_mesh_sun_nerf_shadow_gpu.py's and test_nerf_mesh_shadow_gpu.py's
rule), mesh_sun_nerf_shadow_cases.frame_bound for colour; a count is compared as an integer, on every owner pixel none of whose rays the
float64 tracer flags, traced from the recorded origin along the library's own table. None comes from the code under test."""
import json
import subprocess

import numpy as np
import pytest

from conftest import pkg

import mesh_cases as mc
import mesh_reference as mref
import mesh_sun_nerf_shadow_cases as sc
import nerf_mesh_shadow_cases as nc
import sun_disk_cases as sd

pytestmark = pytest.mark.gpu

W, H = sd.WIDTH, sd.HEIGHT
DISK = dict(angular_radius=sd.RADIUS, n_rays=sd.K)
SHADOW = dict(strength=nc.STRENGTH, bias=nc.BIAS)


def _load(c, scene):
    c.clear_meshes()
    for tris, center in scene:
        c.add_mesh(tris, center)


def _opts(native, **kw):
    return native.make_opts(**dict(dict(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0), render_mode=native.RENDER_SHADE), **kw))


def _cam(native, matrix=sd.CAMERA, w=W, h=H, **kw):
    return native.make_camera(matrix, w, h, sd.FOCAL, **kw)


def _render(c, native, disk, cam=None, shadow=None, sun_nerf=None, **kw):
    c.set_sun_disk(disk)
    c.set_mesh_shadow_on_nerf(shadow)
    c.set_sun_nerf_shadow(sun_nerf)
    try:
        return c.render(cam or _cam(native), _opts(native, **kw), want_depth=True)
    finally:
        c.set_sun_disk(None)
        c.set_mesh_shadow_on_nerf(None)
        c.set_sun_nerf_shadow(None)


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _count(rec_w):
    """the integer count of a disk record's w = 1 + count on owners (0 elsewhere)"""
    return np.where(rec_w != 0, rec_w - 1, 0).astype(np.int64)


def _table(c, s=0, sun=sd.SUN):
    c.set_sun_disk(DISK)
    try:
        return c.sun_disk_directions(sun, s)
    finally:
        c.set_sun_disk(None)


@pytest.fixture(scope="module")
def bare(gpu_ctx, native):
    """the mesh side's meshes alone: the floor and the low plate"""
    c = native.Context(0)
    _load(c, sd.mesh_scene())
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def hybrid(gpu_ctx, native, scene_unit):
    """the unit NeRF over the mesh side's meshes"""
    c = native.Context(0)
    c.set_model(scene_unit)
    _load(c, sd.mesh_scene())
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def nerf_side(gpu_ctx, native, scene_unit):
    """the NeRF side: the unit NeRF over the floor and under nerf_mesh_shadow_cases' plate"""
    c = native.Context(0)
    c.set_model(scene_unit)
    _load(c, nc.scene())
    c.set_geometry_opts()
    yield c
    c.close()


@pytest.fixture(scope="module")
def nerf_bare(gpu_ctx, native):
    c = native.Context(0)
    _load(c, nc.scene())
    c.set_geometry_opts()
    yield c
    c.close()


def _disk_frame(c, native, cam=None, **kw):
    """(frame, depth), the disk record (h, w, 4) and the pass's time of a frame with the disk on"""
    c.set_sun_disk(DISK)
    for name, value in kw.items():
        getattr(c, "set_" + name)(value)
    try:
        fr = c.render(cam or _cam(native), _opts(native), want_depth=True)
        rec = c.frame_sun_disk(W * H).reshape(H, W, 4)
        out = dict(frame=fr, record=rec, ms=c.frame_sun_disk_ms())
        if kw.get("sun_nerf_shadow") is not None:
            out["sun_shadow"] = c.frame_sun_shadow(W * H).reshape(H, W, 4)
        if kw.get("mesh_shadow_on_nerf") is not None:
            out["mesh_shadow"] = c.frame_mesh_shadow(W * H).reshape(H, W, 4)
        return out
    finally:
        c.set_sun_disk(None)
        for name in kw:
            getattr(c, "set_" + name)(None)


@pytest.fixture(scope="module")
def mesh_frames(bare, hybrid, native):
    """the mesh side: the meshes alone off and on, the hybrid frame with ngp_set_sun_nerf_shadow off and on, each with the disk off and on"""
    return dict(bare_off=_render(bare, native, None), bare_on=_disk_frame(bare, native), hybrid_off=_render(hybrid, native, None),
                hybrid_sun_off=_render(hybrid, native, None, sun_nerf=True), hybrid_on=_disk_frame(hybrid, native, sun_nerf_shadow=True))


# ------------------------------------------------------------------------------------------------------- identities as bytes
def test_identities_as_bytes(bare, hybrid, nerf_side, mesh_frames, native):
    """off after on is the parent's frame, depth and records; a disk without meshes and NeRF mode change nothing; strength 0 with the disk on
    gives the frame of ngp_set_mesh_shadow_on_nerf off; the disk on changes the frame and not its depth"""
    off, on = mesh_frames["bare_off"], mesh_frames["bare_on"]["frame"]
    assert (off[0][..., 3] > 0).sum() > 500 and on[0].tobytes() != off[0].tobytes() and on[1].tobytes() == off[1].tobytes()
    assert _same(_render(bare, native, None), off) and bare.sun_disk() is None                    # off after on
    assert _same(_render(hybrid, native, None), mesh_frames["hybrid_off"])
    # ... and every record: both shadow options on the NeRF side, before and after a frame with the disk
    def records():
        nerf_side.set_sun_nerf_shadow(True)
        nerf_side.set_mesh_shadow_on_nerf(SHADOW)
        try:
            fr = nerf_side.render(_cam(native, nc.CAMERA), _opts(native), want_depth=True)
            return fr, nerf_side.frame_sun_shadow(W * H), nerf_side.frame_mesh_shadow(W * H)
        finally:
            nerf_side.set_sun_nerf_shadow(None)
            nerf_side.set_mesh_shadow_on_nerf(None)
    before = records()
    with pytest.raises(RuntimeError, match="ran no sun disk pass"):
        nerf_side.frame_sun_disk(W * H)
    with pytest.raises(RuntimeError, match="ran no sun disk pass"):
        nerf_side.frame_sun_disk_ms()
    with_disk = _render(nerf_side, native, DISK, cam=_cam(native, nc.CAMERA), shadow=SHADOW, sun_nerf=True)
    after = records()
    assert not _same(with_disk, before[0]) and with_disk[1].tobytes() == before[0][1].tobytes()
    assert _same(after[0], before[0]) and after[1].tobytes() == before[1].tobytes() and after[2].tobytes() == before[2].tobytes()
    # NeRF mode
    nerf_mode = dict(testbed_mode=native.MODE_NERF)
    a, b = _render(hybrid, native, DISK, **nerf_mode), _render(hybrid, native, None, **nerf_mode)
    assert _same(a, b) and (a[0][..., 3] > 0).sum() > 300
    with pytest.raises(RuntimeError, match="ran no sun disk pass"):
        hybrid.frame_sun_disk(W * H)
    # no meshes
    hybrid.clear_meshes()
    try:
        assert _same(_render(hybrid, native, DISK, shadow=SHADOW), _render(hybrid, native, None))
    finally:
        _load(hybrid, sd.mesh_scene())
    # strength 0 with the disk on: f = 1 on every NeRF pixel
    cam = _cam(native, nc.CAMERA)
    zero = _render(nerf_side, native, DISK, cam=cam, shadow=dict(strength=0.0, bias=nc.BIAS))
    none = _render(nerf_side, native, DISK, cam=cam)
    some = _render(nerf_side, native, DISK, cam=cam, shadow=SHADOW)
    assert _same(zero, none) and some[0].tobytes() != none[0].tobytes() and some[1].tobytes() == none[1].tobytes() and np.all(some[0] <= none[0])


def test_two_runs_time_and_refusals(bare, mesh_frames, native):
    """a second run is the first as bytes, frame_sun_disk included; the pass's time is positive; after a frame without the pass both
    getters refuse"""
    again = _disk_frame(bare, native)
    first = mesh_frames["bare_on"]
    assert _same(again["frame"], first["frame"]) and again["record"].tobytes() == first["record"].tobytes()
    print("\nmesh_sun_disk_kernel %.4f ms, %.4f ms" % (first["ms"], again["ms"]))
    assert np.isfinite(first["ms"]) and first["ms"] > 0 and again["ms"] > 0
    bare.set_sun_disk(DISK)
    try:
        bare.render(_cam(native), _opts(native))
        with pytest.raises(RuntimeError, match="n_pixels"):
            bare.frame_sun_disk(W * H - 1)
    finally:
        bare.set_sun_disk(None)
    _render(bare, native, None)
    with pytest.raises(RuntimeError, match="ran no sun disk pass"):
        bare.frame_sun_disk(W * H)
    with pytest.raises(RuntimeError, match="ran no sun disk pass"):
        bare.frame_sun_disk_ms()


# ---------------------------------------------------------------------------------------------------------------- mesh record
def _check_mesh_record(name, rec, table, g):
    """(a) the owner set is the float64 reference's; (b) |q - q64| <= TIE_EPS + GPU_FACTOR x the float32 form's deviation; (c) count is the
    float64 tracer's from the recorded q along the library's table on every owner none of whose rays it flags; the rest is under the cap"""
    owner = rec[..., 3] != 0
    ref_owner = g["owner"].reshape(H, W)
    assert np.isfinite(rec).all() and np.all(rec[~owner] == 0) and not g["primary_unsafe"].any()
    assert np.array_equal(owner, ref_owner)                                                            # (a)
    q32 = sc._q32(g["meshes"], g["M"], g["d"], g["entry"], g["start"], g["owner"])
    q_dev = float(np.abs(q32.astype(np.float64) - g["q"])[g["owner"]].max())
    dq = np.abs(rec[..., :3].astype(np.float64) - g["q"].reshape(H, W, 3))[owner].max()
    allow = mref.TIE_EPS + mc.GPU_FACTOR * q_dev
    count = _count(rec[..., 3])
    assert np.array_equal(rec[..., 3][owner], 1.0 + count[owner]) and count.min() >= 0 and count.max() <= sd.K
    count64, flagged = sd.counts(g["meshes"], rec[..., :3][owner], table)
    differ = int((count[owner] != count64)[~flagged].sum())
    o, p, f = sd.classes(count, owner)
    print("\n%s: %d owners; open %d, partial %d, full %d; |dq| %.2e (allowed %.2e); owners with a flagged ray %d (%.2f %%); count differs on %d of the others, on %d of the flagged"
          % (name, owner.sum(), o, p, f, dq, allow, flagged.sum(), 100.0 * flagged.sum() / owner.sum(), differ, (count[owner] != count64)[flagged].sum()))
    assert dq <= allow, (dq, allow)                                                                    # (b)
    assert differ == 0 and flagged.sum() <= sd.UNSAFE_CAP * owner.sum()                                # (c)
    assert min(o, p, f) >= sd.CLASS_SHARE * owner.sum()
    return owner, count


def test_mesh_record_matches_the_reference(bare, hybrid, mesh_frames, native):
    """on the meshes alone, and in the hybrid frame with ngp_set_sun_nerf_shadow on, where the shadow-list entry is live (the sun shadow's
    record holds q) exactly where V > 0 and carries the disk's q as bits"""
    g = sd.mesh_geometry()
    table = _table(bare)
    assert table.tobytes() == sd.directions(sd.SUN, sd.RADIUS, sd.K, 0).tobytes()
    owner, count = _check_mesh_record("meshes alone", mesh_frames["bare_on"]["record"], table, g)
    hy = mesh_frames["hybrid_on"]
    assert hy["record"].tobytes() == mesh_frames["bare_on"]["record"].tobytes()  # the same G-buffer, the same table
    _check_mesh_record("hybrid, sun_nerf_shadow on", hy["record"], table, g)
    ss = hy["sun_shadow"]
    live = np.any(ss[..., :3] != 0, axis=-1)
    V = sd.visibility(count, sd.K)
    assert np.array_equal(live[owner], (V > 0)[owner]) and (owner & live).sum() > 100 and (owner & ~live).sum() > 100
    assert ss[..., :3][owner & live].tobytes() == hy["record"][..., :3][owner & live].tobytes() and np.all(ss[owner & ~live] == 0)


# ---------------------------------------------------------------------------------------------------------------- mesh colour
def test_mesh_colour_is_the_restated_shading(mesh_frames):
    """the meshes alone: the frame is the float64 shading with light = SUN_COLOUR V on owners, V from the record, within frame_bound on safe
    pixels; depth is the off frame's; pixels the disk leaves open keep the off frame's bytes; partial pixels lie strictly between their
    V = 0 and V = 1 colours in the channel sum, which is what fails without the option"""
    g = sd.mesh_geometry()
    (off, off_depth), (on, on_depth) = mesh_frames["bare_off"], mesh_frames["bare_on"]["frame"]
    rec = mesh_frames["bare_on"]["record"]
    owner, count = rec[..., 3] != 0, _count(rec[..., 3])
    V = sd.visibility(count, sd.K)
    want, unsafe = sd.mesh_colour(g, V)
    bound = sc.frame_bound(want[..., :3])
    m = ~unsafe & g["covered"].reshape(H, W)
    ratio = np.abs(on[..., :3].astype(np.float64) - want[..., :3])[m] / bound[m]
    dark, lit = sd.mesh_colour(g, 0.0)[0][..., :3].sum(-1), sd.mesh_colour(g, 1.0)[0][..., :3].sum(-1)
    partial = owner & (count > 0) & (count < sd.K) & m & (lit - dark > 0.1)
    got = on[..., :3].astype(np.float64).sum(-1)
    share = (got - dark)[partial] / (lit - dark)[partial]
    print("\ncovered and safe %d of %d; largest colour deviation / bound %.3g; partial pixels with sun %d: (sum - dark) / (lit - dark) in [%.3f, %.3f]"
          % (m.sum(), g["covered"].sum(), ratio.max(), partial.sum(), share.min(), share.max()))
    assert on_depth.tobytes() == off_depth.tobytes() and np.array_equal(on[..., 3][m], want[..., 3][m])
    assert ratio.max() <= 1.0, ratio.max()
    assert partial.sum() >= 50 and np.all(got[partial] > dark[partial]) and np.all(got[partial] < lit[partial])
    same = ~owner | ((count == 0) & ~g["shadowed"].reshape(H, W) & ~g["shadow_unsafe"].reshape(H, W))
    assert on[same].tobytes() == off[same].tobytes()
    full = owner & (count == sd.K) & m & (lit - dark > 0.1)
    assert full.sum() >= 50 and np.all(np.abs(got - dark)[full] <= 3 * bound.max(-1)[full])


def test_hybrid_colour_carries_v_times_t_s(mesh_frames):
    """ngp_set_sun_nerf_shadow on as well: on pixels the NeRF pass leaves alone, light = SUN_COLOUR V T_s with T_s = max(1 - alpha_s, 0)
    from the sun shadow's record, within frame_bound"""
    g = sd.mesh_geometry()
    hy = mesh_frames["hybrid_on"]
    on = hy["frame"][0]
    (off, off_depth), (bare, bare_depth) = mesh_frames["hybrid_off"], mesh_frames["bare_off"]
    clear = np.all(off.view(np.uint32) == bare.view(np.uint32), axis=-1) & (off_depth.view(np.uint32) == bare_depth.view(np.uint32))
    V = sd.visibility(_count(hy["record"][..., 3]), sd.K)
    T_s = sc.factor_of(hy["sun_shadow"][..., 3])
    want, unsafe = sd.mesh_colour(g, V, T_s)
    bound = sc.frame_bound(want[..., :3])
    m = clear & ~unsafe & g["covered"].reshape(H, W)
    ratio = np.abs(on[..., :3].astype(np.float64) - want[..., :3])[m] / bound[m]
    both = m & (V > 0) & (V < 1) & (T_s < 1)
    print("\nclear, covered and safe %d; largest colour deviation / bound %.3g; pixels with 0 < V < 1 and T_s < 1: %d" % (m.sum(), ratio.max(), both.sum()))
    assert m.sum() >= sc.MIN_RAYS and both.sum() >= 10 and ratio.max() <= 1.0, ratio.max()
    assert hy["frame"][1].tobytes() == off_depth.tobytes() and on.tobytes() != mesh_frames["hybrid_sun_off"][0].tobytes()


# ---------------------------------------------------------------------------------------------------- NeRF record and colour
def _nerf_frames(nerf_side, nerf_bare, native, scene_unit, matrix):
    """the NeRF side of one view with the disk on: the hybrid frame with and without the meshes' shadow, its records, the meshes alone (m)
    and the model alone inside the meshes' box (n, with what the depth test culls taken out), as test_nerf_mesh_shadow_gpu.py forms them"""
    cam = _cam(native, matrix)
    on = _disk_frame(nerf_side, native, cam=cam, mesh_shadow_on_nerf=SHADOW)
    none = _render(nerf_side, native, DISK, cam=cam)
    lo, hi = nerf_side.mesh_info()["aabb"]
    alone = native.Context(0)
    try:
        alone.set_model(dict(scene_unit, render_aabb=(tuple(float(x) for x in lo), tuple(float(x) for x in hi))))
        nerf = alone.render(cam, _opts(native), want_depth=True)
    finally:
        alone.close()
    m, m_depth = _render(nerf_bare, native, DISK, cam=cam)
    behind = m_depth >= np.float32(0.01)
    n = np.where((behind & (nerf[1] > m_depth))[..., None], np.float32(0), nerf[0])
    unknown = (nerf[0][..., 3] > 0) & (nerf[0][..., 3] <= np.float32(nc.OWNER_ALPHA)) & behind
    return dict(on=on["frame"], record=on["mesh_shadow"], disk_record=on["record"], none=none, m=m, m_depth=m_depth, n=n, unknown=unknown, behind=behind)


@pytest.mark.parametrize("view", ["CAMERA", "CAMERA_ABOVE"])
def test_nerf_record_and_composite(view, nerf_side, nerf_bare, native, scene_unit):
    """(a) the owners are the pixels where the NeRF's own alpha exceeds 0.2, w = 1 + count / K, zeros elsewhere; (b) p as
    test_nerf_mesh_shadow_gpu.py checks it; (c) count is the float64 tracer's from the recorded p along the library's table on every owner
    without a flagged ray; (d) the frame is nerf_mesh_shadow_cases.composite(n, m, f) as bytes, f from the recorded count, on the pixels
    that file's test compares (alpha <= 0.2 over a mesh left out); open pixels are the frame's without the meshes' shadow, as bytes"""
    matrix = getattr(nc, view)
    fr = _nerf_frames(nerf_side, nerf_bare, native, scene_unit, matrix)
    rec, (on, depth) = fr["record"], fr["on"]
    owner = rec[..., 3] != 0
    blocked = np.where(owner, rec[..., 3] - 1, 0)
    count = np.rint(blocked * sd.K).astype(np.int64)
    assert np.isfinite(rec).all() and np.all(rec[~owner] == 0) and np.array_equal(blocked, count / sd.K) and count.min() >= 0 and count.max() <= sd.K
    assert np.array_equal(owner, fr["n"][..., 3] > np.float32(nc.OWNER_ALPHA))                                # (a)
    sh = nc.shadow(np.where(owner, 1.0, 0.0), depth, nc.meshes(), matrix_3x4=matrix)
    dp = np.abs(rec[..., :3].astype(np.float64) - sh["p"])[owner].max()
    allow = mref.TIE_EPS + mc.GPU_FACTOR * sh["p_dev"]
    table = _table(nerf_side, sun=nc.SUN)
    count64, flagged = sd.counts_from_p(rec[..., :3][owner], table)
    differ = int((count[owner] != count64)[~flagged].sum())
    o, p, f_ = sd.classes(count, owner)
    print("\n%s: %d owners; open %d, partial %d, full %d; |dp| %.2e (allowed %.2e); owners with a flagged ray %d (%.2f %%); count differs on %d of the others"
          % (view, owner.sum(), o, p, f_, dp, allow, flagged.sum(), 100.0 * flagged.sum() / owner.sum(), differ))
    assert dp <= allow, (dp, allow)                                                                            # (b)
    assert differ == 0 and flagged.sum() <= sd.UNSAFE_CAP * owner.sum()                                        # (c)
    assert min(o, p, f_) >= sd.CLASS_SHARE * owner.sum()
    f = np.where(owner, sd.factor(count, sd.K, nc.STRENGTH), np.float32(1)).astype(np.float32)
    known = ~fr["unknown"]
    want = nc.composite(fr["n"], fr["m"], f)
    assert depth.tobytes() == fr["none"][1].tobytes()
    assert on[known].tobytes() == want[known].tobytes()                                                        # (d)
    assert nc.composite(fr["n"], fr["m"], np.ones_like(f))[known].tobytes() == fr["none"][0][known].tobytes()
    assert on[count == 0].tobytes() == fr["none"][0][count == 0].tobytes() and np.all(on <= fr["none"][0])
    part = owner & (count > 0) & (count < sd.K) & (fr["n"][..., :3].sum(-1) > 0.05) & ~fr["behind"]
    hard = np.float32(1) - np.float32(nc.STRENGTH)
    assert part.sum() >= 20 and np.all(on[..., :3][part].sum(-1) < fr["none"][0][..., :3][part].sum(-1)) and np.all(f[part] > hard)
    # the mesh pixels of this frame own disks too, and the meshes alone give the same record
    assert (fr["disk_record"][..., 3] != 0).sum() > 100


# ----------------------------------------------------------------------------------------------------------------- structure
def _pixel_offset(spp_index):
    import oracle as orc

    return orc.Oracle().pixel_offset(spp_index)


def test_two_samples_use_the_rotated_table(bare, native):
    """2 spp with jittered samples: the record is the last sample's, the record of the one-sample frame of spp index 1, and its counts are
    the float64 tracer's along the restated table with s = 1, which is the library's; the table with s = 0 gives other counts"""
    cam = _cam(native, snap=False)
    bare.set_sun_disk(DISK)
    try:
        two = bare.render(cam, _opts(native, spp=2), want_depth=True)
        rec2 = bare.frame_sun_disk(W * H)
        bare.render(_cam(native, snap=False, spp_index=1), _opts(native))
        rec_last = bare.frame_sun_disk(W * H)
        bare.render(cam, _opts(native))
        rec_first = bare.frame_sun_disk(W * H)
        lib = bare.sun_disk_directions(sd.SUN, 1)
    finally:
        bare.set_sun_disk(None)
    off = _render(bare, native, None, cam=cam, spp=2)
    assert rec2.tobytes() == rec_last.tobytes() and rec2.tobytes() != rec_first.tobytes()
    assert two[0].tobytes() != off[0].tobytes() and two[1].tobytes() == off[1].tobytes()
    t1, t0 = sd.directions(sd.SUN, sd.RADIUS, sd.K, 1), sd.directions(sd.SUN, sd.RADIUS, sd.K, 0)
    assert lib.tobytes() == t1.tobytes() and t1.tobytes() != t0.tobytes()
    owner = rec2[:, 3] != 0
    g = sd.mesh_geometry(pixel_offset=tuple(float(x) for x in _pixel_offset(1)))
    assert np.array_equal(owner[~g["primary_unsafe"]], g["owner"][~g["primary_unsafe"]]) and g["primary_unsafe"].sum() <= mc.UNSAFE_CAP * owner.size
    count = _count(rec2[:, 3])[owner]
    c1, flagged1 = sd.counts(g["meshes"], rec2[:, :3][owner], t1)
    c0, flagged0 = sd.counts(g["meshes"], rec2[:, :3][owner], t0)
    safe = ~flagged1 & ~flagged0
    print("\n2 spp: %d owners, flagged under either table %d; counts differ from s = 1 on %d safe owners, from s = 0 on %d" % (owner.sum(), (~safe).sum(), (count != c1)[safe].sum(), (count != c0)[safe].sum()))
    assert np.array_equal(count[safe], c1[safe]) and (count != c0)[safe].sum() >= 10 and flagged1.sum() <= sd.UNSAFE_CAP * owner.sum()


def _tiles(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return (ys // 8) * ((w + 7) // 8) + xs // 8, (xs % 8) + 8 * (ys % 8)


def _both_on(c):
    c.set_sun_disk(DISK)
    c.set_mesh_shadow_on_nerf(SHADOW)


def _both_off(c):
    c.set_sun_disk(None)
    c.set_mesh_shadow_on_nerf(None)


@pytest.mark.parametrize("side", ["mesh", "nerf"])
def test_shards_and_packed_shards_cover_the_frame(side, hybrid, nerf_side, native):
    """three shards in image layout and tile-packed (60 x 44: partial tiles on both axes) against the whole frame, both kernels at work, in
    the view whose mesh pixels and in the view whose NeRF pixels lie in a penumbra: colour, depth and both records, as bytes"""
    import torch

    w, h, world = 60, 44, 3
    nerf_side, matrix = (hybrid, sd.CAMERA) if side == "mesh" else (nerf_side, nc.CAMERA)
    cam = _cam(native, matrix, w=w, h=h)
    tile, slot = _tiles(w, h)
    _both_on(nerf_side)
    try:
        full, full_depth = nerf_side.render(cam, _opts(native), want_depth=True)
        full_rec = np.concatenate([nerf_side.frame_sun_disk(w * h), nerf_side.frame_mesh_shadow(w * h)], 1).reshape(h, w, 8)
        part_disk, part_nerf = _count(full_rec[..., 3]), full_rec[..., 7]
        assert (((part_disk > 0) & (part_disk < sd.K)).sum() > 10 if side == "mesh" else ((part_nerf > 1) & (part_nerf < 2)).sum() > 20) and (full[..., 3] > 0).sum() > 500
        assert (full_rec[..., 3] != 0).sum() > 100 and (part_nerf != 0).sum() > 100
        total, total_depth, total_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        packed, packed_depth, packed_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        for r in range(world):
            mine = tile % world == r
            part, part_depth = nerf_side.render(cam, _opts(native, shard_index=r, shard_count=world), want_depth=True)
            rec = np.concatenate([nerf_side.frame_sun_disk(w * h), nerf_side.frame_mesh_shadow(w * h)], 1).reshape(h, w, 8)
            assert not np.any(part[~mine]) and not np.any(rec[~mine])
            total[mine], total_depth[mine], total_rec[mine] = part[mine], part_depth[mine], rec[mine]
            n = native.load_library().ngp_packed_tiles(w, h, r, world) * 64
            rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
            nerf_side.render_device(cam, _opts(native, shard_index=r, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
            rec = np.concatenate([nerf_side.frame_sun_disk(n), nerf_side.frame_mesh_shadow(n)], 1)  # (synchronises the context's stream)
            src = (tile // world) * 64 + slot
            packed[mine], packed_depth[mine], packed_rec[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]], rec[src[mine]]
    finally:
        _both_off(nerf_side)
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes() and total_rec.tobytes() == full_rec.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes() and packed_rec.tobytes() == full_rec.tobytes()


@pytest.fixture(scope="module")
def nerf_on(nerf_side, native):
    """the NeRF side's frame and records with the disk and the meshes' shadow on"""
    return _disk_frame(nerf_side, native, cam=_cam(native, nc.CAMERA), mesh_shadow_on_nerf=SHADOW)


def test_two_devices_render_the_one_device_frame(nerf_on, native, scene_unit):
    """a context of two devices (the same ordinal twice): the option reaches the replica with the geometry, each device spreads the rays of
    its share, the frame is the one-device frame as bytes; the records are the primary's tile-packed share"""
    multi = native.Context(devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        multi.set_model(scene_unit)
        _load(multi, nc.scene())
        multi.set_geometry_opts()
        cam = _cam(native, nc.CAMERA)
        off = multi.render(cam, _opts(native), want_depth=True)
        _both_on(multi)
        assert _same(multi.render(cam, _opts(native), want_depth=True), nerf_on["frame"])
        n = native.load_library().ngp_packed_tiles(W, H, 0, 2) * 64
        tile, slot = _tiles(W, H)
        mine = tile % 2 == 0
        src = ((tile // 2) * 64 + slot)[mine]
        assert multi.frame_sun_disk(n)[src].tobytes() == nerf_on["record"][mine].tobytes()
        assert multi.frame_mesh_shadow(n)[src].tobytes() == nerf_on["mesh_shadow"][mine].tobytes()
        _both_off(multi)
        assert _same(multi.render(cam, _opts(native), want_depth=True), off) and not _same(off, nerf_on["frame"])  # and off reaches it too
    finally:
        multi.close()


def test_frame_on_a_callers_stream(nerf_side, nerf_on, native):
    """ngp_render_device on a caller's stream, then the caller's own synchronise: the same bytes"""
    import torch

    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    _both_on(nerf_side)
    try:
        nerf_side.render_device(_cam(native, nc.CAMERA), _opts(native), rgba.data_ptr(), dep.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert rgba.cpu().numpy().tobytes() == nerf_on["frame"][0].tobytes() and dep.cpu().numpy().tobytes() == nerf_on["frame"][1].tobytes()
        assert nerf_side.frame_sun_disk(W * H).tobytes() == nerf_on["record"].tobytes() and nerf_side.frame_sun_disk_ms() > 0
    finally:
        _both_off(nerf_side)


def test_both_kernel_layouts_give_equal_records(bare, nerf_side, mesh_frames, nerf_on, native, monkeypatch):
    """NGP_SUN_DISK_LAYOUT=thread, one thread a pixel looping over its rays in place of the wave dealing them over its lanes: frames and
    records are the same bytes, on both kernels and for every allowed K"""
    monkeypatch.setenv("NGP_SUN_DISK_LAYOUT", "thread")
    loop = _disk_frame(bare, native)
    assert _same(loop["frame"], mesh_frames["bare_on"]["frame"]) and loop["record"].tobytes() == mesh_frames["bare_on"]["record"].tobytes()
    loop = _disk_frame(nerf_side, native, cam=_cam(native, nc.CAMERA), mesh_shadow_on_nerf=SHADOW)
    assert _same(loop["frame"], nerf_on["frame"]) and loop["record"].tobytes() == nerf_on["record"].tobytes() and loop["mesh_shadow"].tobytes() == nerf_on["mesh_shadow"].tobytes()
    for k in sd.ALLOWED_RAYS:
        out = {}
        for layout in ("thread", "wave"):
            monkeypatch.setenv("NGP_SUN_DISK_LAYOUT", layout)
            nerf_side.set_sun_disk(dict(angular_radius=sd.RADIUS, n_rays=k))
            nerf_side.set_mesh_shadow_on_nerf(SHADOW)
            try:
                fr = nerf_side.render(_cam(native, nc.CAMERA), _opts(native), want_depth=True)
                out[layout] = (fr, nerf_side.frame_sun_disk(W * H), nerf_side.frame_mesh_shadow(W * H))
            finally:
                _both_off(nerf_side)
        a, b = out["thread"], out["wave"]
        assert _same(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), k
        assert set(np.unique(_count(b[1][:, 3]))) <= set(range(k + 1)) and (b[2][:, 3] > 1).sum() > 50, k


# ------------------------------------------------------------------------------------------------------------------ bindings
def _write_scene(tmp_path, nerf_side, name="plate", plate_center=nc.PLATE_CENTER):
    """the meshes as .obj files, the unit NeRF as a snapshot, and the scene file that names them"""
    mi = pkg("meshio")
    entries = []
    for i, (tris, center) in enumerate(nc.scene()):
        mi.save_obj(str(tmp_path / ("mesh%d.obj" % i)), tris)
        entries.append({"center": [float(x) for x in (center if i == 0 else plate_center)], "path": "mesh%d.obj" % i, "type": "Mesh"})
    nerf_side.save_snapshot_file(str(tmp_path / "unit.ingp"))
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


def test_pyngp_and_command_line(tmp_path, nerf_side, native):
    """testbed.sun_disk (with its two parameters) gives the native frame as bytes, and --sun_disk writes the frame the property gives, to
    the 8 bits of the file"""
    from PIL import Image

    pyngp = pkg("build").import_pyngp()
    scene = _write_scene(tmp_path, nerf_side)
    cam = _cam(native, nc.CAMERA)
    tb = _testbed(pyngp, scene)
    assert tb.sun_disk is False and tb.sun_disk_angular_radius == np.float32(sd.REAL_SUN) and tb.sun_disk_rays == 16
    off = tb.render(W, H, 1, True)
    tb.sun_disk = True
    real = tb.render(W, H, 1, True)
    tb.sun_disk_angular_radius, tb.sun_disk_rays, tb.mesh_shadow_on_nerf = sd.RADIUS, 8, True
    own = tb.render(W, H, 1, True)
    tb.sun_disk, tb.mesh_shadow_on_nerf = False, False
    assert tb.render(W, H, 1, True).tobytes() == off.tobytes()
    del tb
    c = native.Context(0)
    try:
        c.load_scene(scene)
        c.set_geometry_opts()
        assert c.render(cam, _opts(native)).tobytes() == off.tobytes()
        c.set_sun_disk(True)
        assert c.render(cam, _opts(native)).tobytes() == real.tobytes()
        c.set_sun_disk(dict(angular_radius=sd.RADIUS, n_rays=8))
        c.set_mesh_shadow_on_nerf(True)
        assert c.render(cam, _opts(native)).tobytes() == own.tobytes()
    finally:
        c.close()
    print("\npyngp: sun_disk changes %d of %d pixels, with 5 degrees and the meshes' shadow %d" % ((np.abs(real - off).max(-1) > 0).sum(), W * H, (np.abs(own - off).max(-1) > 0).sum()))
    assert (off[..., 3] > 0).sum() > 500 and (np.abs(own - off).max(-1) > 0).sum() > 100 and own.tobytes() != real.tobytes()
    # the command line writes the frame of the default camera: un-premultiplied, sRGB-encoded, 8 bits (csrc/ngp_main.cpp write_png; pow may round the last bit).
    # That camera looks at the cube from +z, the side the case's plate leaves in the sun: the plate moves over it (centre (0.5, 0.7, 0.5)).
    scene = _write_scene(tmp_path, nerf_side, "plate_in_front", (0.5, 0.7, 0.5))
    shots = {}
    for disk in (False, True):
        tb = _testbed(pyngp, scene, camera=False)
        tb.mesh_shadow_on_nerf, tb.mesh_shadow_on_nerf_strength = True, 1.0
        tb.sun_disk, tb.sun_disk_angular_radius, tb.sun_disk_rays = disk, sd.RADIUS, 8
        shots[disk] = tb.render(W, H, 1, True)
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
    for disk in (True, False):
        out = tmp_path / ("shot%d.png" % disk)
        r = subprocess.run([exe, "--no-gui", "--scene", scene, "--render_mode", "Shade", "--width", str(W), "--height", str(H), "--screenshot", str(out), "--mesh_shadow_on_nerf",
                            "--mesh_shadow_on_nerf_strength", "1"] + (["--sun_disk", "--sun_disk_angular_radius", repr(sd.RADIUS), "--sun_disk_rays", "8"] if disk else []),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        png = np.asarray(Image.open(out)).astype(np.int64)
        assert png.shape == (H, W, 4) and np.abs(png - expect[disk]).max() <= 1 and (png != expect[disk]).mean() < 0.01, (disk, np.abs(png - expect[disk]).max(), (png != expect[disk]).mean())
        assert (png[..., 3] > 0).sum() > 100
