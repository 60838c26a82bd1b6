"""All the frame options at once on the GPU (include/ngp_hip.h, the six blocks from "sun: the NeRF in front of the frames' sun" to "mesh
reflection, the meshes in it"): frame_options_cases' one case rendered under each of the 48 option sets on one context. What the contract
promises across options as bytes -- depth never changes, each pass's record depends on its own options alone, the NeRF-side options leave a
pixel without NeRF alone and the mesh-side options a pixel without a mesh, no state survives a frame, a pass that did not run refuses its
record -- and the frames with every option on, and the three-option sets no pair reaches, against the composed float64 reference.

Which options a record depends on, read from the header: the reflection's 12 floats on the reflection alone ("each record is that of the
frame with only that option on"; the sub-option "does not change [it] by a bit"); the hit record on the reflection and its sub-option
(shadow2 is the central ray, "ngp_set_sun_nerf_shadow does not reach the hit", the disk "stays hard-edged" there); the ambient record on
the ambient change alone (its owners and p are the NeRF pass's); the disk record on the disk alone (q is the G-buffer's, the count the
meshes'); the sun-shadow record on the sun shadow and on whether the disk is on (the disk rewrites the list: live where V > 0); the
mesh-shadow record on the meshes' shadow and on whether the disk is on (w = 1 + count / K).

Tolerances are the single-option tests' own, summed per pixel over the terms present (frame_options_cases.mesh_layer and frame); what only
the network supplies is measured by ngp_trace_nerf_rays at the records' own rays and by a context without meshes, never read from the
frame under test. The ambient ratio g goes into the reference as the record holds it once the record has met
ambient_change_cases.ratio's allowance, as test_ambient_change_gpu.py's colour test takes it: a float64 ratio rounded to float32 is not
the float32 program's own rounding, and the composite is compared as bytes."""
import numpy as np
import pytest

import ambient_change_cases as ac
import frame_options_cases as fo
import mesh_cases as mc
import mesh_reference as mref
import mesh_sun_nerf_shadow_cases as sc
import mesh_volume_cases as mv
import nerf_mesh_shadow_cases as nc
import sun_disk_cases as sd
from test_sun_disk_gpu import _count, _load, _opts, _same, _tiles

pytestmark = pytest.mark.gpu

W, H = fo.WIDTH, fo.HEIGHT
INF = np.float32(np.inf)
# the record getters: (name, the option that runs the pass, floats a pixel, the refusal after a frame without the pass)
GETTERS = (("frame_sun_shadow", "sun", 4, "traced no sun shadow rays"), ("frame_sun_disk", "disk", 4, "ran no sun disk pass"),
           ("frame_mesh_reflection", "refl", 12, "traced no reflection rays"), ("frame_mesh_reflection_hits", "hits", 8, "shaded no reflection hits"),
           ("frame_mesh_shadow", "shadow", 4, "ran no mesh shadow pass"), ("frame_ambient_change", "ambient", 12, "ran no ambient change pass"))
# what each record depends on, beside its own option
DEPENDS = dict(frame_sun_shadow=("sun", "disk"), frame_sun_disk=("disk",), frame_mesh_reflection=("refl",), frame_mesh_reflection_hits=("refl", "hits"),
               frame_mesh_shadow=("shadow", "disk"), frame_ambient_change=("ambient",))
VISIBILITY = dict(n_u=8, n_v=8, sharpness_log2=4, max_distance=0.0, normal_bias=0.01)


def _cam(native, w=W, h=H, **kw):
    return native.make_camera(fo.CAMERA, w, h, fo.FOCAL, **kw)


def _apply(c, options):
    c.set_sun_nerf_shadow(fo.SUN_NERF if "sun" in options else None)
    c.set_sun_disk(fo.DISK if "disk" in options else None)
    c.set_mesh_reflection(fo.REFLECTION if "refl" in options else None)
    c.set_mesh_reflection_meshes("hits" in options)
    c.set_mesh_shadow_on_nerf(fo.SHADOW if "shadow" in options else None)
    c.set_ambient_change_on_nerf(True if "ambient" in options else None)


def _records(c, n):
    """per getter: the record (n, floats), or the message it refuses with"""
    out = {}
    for name, _, _, _ in GETTERS:
        try:
            out[name] = getattr(c, name)(n)
        except RuntimeError as e:
            out[name] = str(e)
    return out


def _shot(c, native, options, w=W, h=H, **kw):
    """the frame (colour, depth) and every record of one option set; the options stay as set"""
    _apply(c, options)
    frame = c.render(_cam(native, w, h), _opts(native, **kw), want_depth=True)
    return dict(frame=frame, records=_records(c, w * h))


def _equal(a, b):
    """two shots: colour, depth and every record as bytes, a refusal equal to a refusal"""
    if not _same(a["frame"], b["frame"]):
        return False
    for name, x in a["records"].items():
        y = b["records"][name]
        if isinstance(x, str) != isinstance(y, str) or (x != y if isinstance(x, str) else x.tobytes() != y.tobytes()):
            return False
    return True


def _context(native, scene_unit, devices=None):
    c = native.Context(0) if devices is None else native.Context(devices=devices)
    c.set_model(scene_unit)
    _load(c, fo.scene())
    c.set_geometry_opts()
    after, before, _ = ac.volumes()
    c.set_irradiance_volume(mv.as_grid(after, ac.RES), (ac.LO, ac.HI), ac.N_U, ac.N_V)
    c.set_reference_irradiance_volume(mv.as_grid(before, ac.RES), (ac.LO, ac.HI), ac.N_U, ac.N_V)
    return c


@pytest.fixture(scope="module")
def ctx(gpu_ctx, native, scene_unit):
    """the unit NeRF over the case's four meshes, the default geometry options, ambient_change_cases' two volumes"""
    c = _context(native, scene_unit)
    yield c
    c.close()


@pytest.fixture(scope="module")
def first(ctx, native):
    """every one of the 48 sets rendered once on the one context, in Gray-code order: set -> shot"""
    out = {s: _shot(ctx, native, s) for s in fo.gray_order()}
    _apply(ctx, frozenset())
    return out


@pytest.fixture(scope="module")
def alone(ctx, native, scene_unit):
    """what the frames under test are not asked for: the meshes alone (m, its depth), the model alone inside the meshes' box (n, with what the
    depth test culls taken out, and its depth), the pixels whose cull cannot be read from these (unknown), as test_ambient_change_gpu.py's
    frames fixture forms them"""
    lo, hi = ctx.mesh_info()["aabb"]
    cam = _cam(native)
    model = native.Context(0)
    bare = native.Context(0)
    try:
        model.set_model(dict(scene_unit, render_aabb=(tuple(float(x) for x in lo), tuple(float(x) for x in hi))))
        nerf = model.render(cam, _opts(native), want_depth=True)
        _load(bare, fo.scene())
        bare.set_geometry_opts()
        m, m_depth = bare.render(cam, _opts(native), want_depth=True)
    finally:
        model.close()
        bare.close()
    behind = m_depth >= np.float32(0.01)
    n = np.where((behind & (nerf[1] > m_depth))[..., None], np.float32(0), nerf[0])
    unknown = (nerf[0][..., 3] > 0) & (nerf[0][..., 3] <= np.float32(nc.OWNER_ALPHA)) & behind
    return dict(n=n, n_depth=nerf[1], m=m, m_depth=m_depth, unknown=unknown, behind=behind)


# ------------------------------------------------------------------------------------------------------- identities as bytes
def test_depth_never_changes_and_unrun_passes_refuse(first):
    """the depth image of every set is the all-off depth as bytes; a set's frame has a record for exactly the passes it turns on, and every
    other getter refuses with its own message; every set changes the colour of the set without any one of its options"""
    none = first[frozenset()]
    assert (none["frame"][0][..., 3] > 0).sum() > 500
    for s, shot in first.items():
        assert shot["frame"][1].tobytes() == none["frame"][1].tobytes(), fo.name(s)
        for name, option, floats, refusal in GETTERS:
            rec = shot["records"][name]
            if option in s:
                assert not isinstance(rec, str) and rec.shape == (W * H, floats) and not np.isnan(rec).any(), (fo.name(s), name)
            else:
                assert isinstance(rec, str) and refusal in rec, (fo.name(s), name, rec)
        for o in s:
            less = s - {o} - ({"hits"} if o == "refl" else set())
            assert shot["frame"][0].tobytes() != first[less]["frame"][0].tobytes(), (fo.name(s), o)


def test_records_are_separable(first):
    """each pass's record in every set that runs it equals, as bytes, the record in the smallest set that determines it (DEPENDS)"""
    for s, shot in first.items():
        for name, option, _, _ in GETTERS:
            if option in s:
                least = frozenset(o for o in DEPENDS[name] if o in s)
                assert shot["records"][name].tobytes() == first[least]["records"][name].tobytes(), (fo.name(s), name, fo.name(least))
    # and the dependence that is there is there: the disk changes both shadow records
    for name, a, b in (("frame_sun_shadow", ("sun",), ("sun", "disk")), ("frame_mesh_shadow", ("shadow",), ("shadow", "disk"))):
        assert first[frozenset(a)]["records"][name].tobytes() != first[frozenset(b)]["records"][name].tobytes()


def test_colour_is_separable_by_pixel_class(first, alone):
    """where the NeRF's scratch is empty (its own alpha 0) a set's colour is that of the same set without the meshes' shadow and the ambient
    change; where no mesh covers the pixel (it owns no disk: the primary ray found no triangle) it is that of the same set without the sun
    shadow, the reflection and its sub-option; the disk stays as it is in both. As bytes, in all 48 sets."""
    empty = (alone["n"][..., 3] == 0) & ~alone["unknown"]
    no_mesh = first[frozenset(("disk",))]["records"]["frame_sun_disk"].reshape(H, W, 4)[..., 3] == 0
    print("\npixels with an empty NeRF scratch %d, without a mesh %d, of %d" % (empty.sum(), no_mesh.sum(), W * H))
    assert empty.sum() >= fo.SHARES["mesh_alone"] * W * H and (no_mesh & (alone["n"][..., 3] > np.float32(nc.OWNER_ALPHA))).sum() >= fo.SHARES["nerf_alone"] * W * H
    assert np.all(alone["m"][..., :3][no_mesh] == 0) and np.all(alone["m"][..., 3][no_mesh] == 1)
    for s, shot in first.items():
        colour = shot["frame"][0]
        assert colour[empty].tobytes() == first[s - {"shadow", "ambient"}]["frame"][0][empty].tobytes(), fo.name(s)
        assert colour[no_mesh].tobytes() == first[s - {"sun", "refl", "hits"}]["frame"][0][no_mesh].tobytes(), fo.name(s)


def test_no_state_survives_a_frame(ctx, first, native, scene_unit):
    """the 48 sets a second time on the same context in a shuffled order, with a 52 x 36 or a 120 x 88 frame of the set rendered ahead of two
    of every three (the larger one grows every buffer the set's passes own, under whatever the sets before left behind): colour, depth and
    every record of every set equal the first visit's as bytes, refusals included; the frames of the other sizes repeat too; and the all-on
    frame of a fresh context equals them"""
    order = fo.option_sets()
    np.random.default_rng(48).shuffle(order)
    assert order != fo.gray_order()
    other = {}
    try:
        for i, s in enumerate(order):
            if i % 3:
                w, h = fo.WALK_SIZES[i % 3 - 1]
                other[(s, w, h)] = _shot(ctx, native, s, w, h)
            assert _equal(_shot(ctx, native, s), first[s]), (i, fo.name(s))
        for (s, w, h), shot in list(other.items())[::7]:  # (now that every buffer has its final size)
            assert _equal(_shot(ctx, native, s, w, h), shot), (fo.name(s), w, h)
    finally:
        _apply(ctx, frozenset())
    fresh = _context(native, scene_unit)
    try:
        big = _shot(fresh, native, fo.ALL, *fo.WALK_SIZES[1])
        assert _equal(_shot(fresh, native, fo.ALL), first[fo.ALL])
        known = [shot for (s, w, h), shot in other.items() if s == fo.ALL and (w, h) == fo.WALK_SIZES[1]]
        assert all(_equal(big, shot) for shot in known)
    finally:
        fresh.close()


IDS_REFUSAL = "ran without mesh materials"
# the passes' time getters, by the option that runs the pass; after a frame without the pass the disk's refuses like its record, the others give 0
MS_GETTERS = (("frame_sun_shadow_ms", "sun"), ("frame_sun_disk_ms", "disk"), ("frame_mesh_reflection_ms", "refl"), ("frame_mesh_reflection_hits_ms", "hits"),
              ("frame_mesh_shadow_ms", "shadow"), ("frame_ambient_change_ms", "ambient"))


def test_buffers_grow_whichever_pass_comes_first(first, native, scene_unit):
    """a fresh context whose first frames each need a shared buffer through the pass that never allocated it first elsewhere: the sun's disk
    alone (the G-buffer and the shadow list with no sun-shadow record), the ambient change alone (the NeRF scratch with no mesh-shadow
    record), materials alone (the id plane; every mesh owns a copy of the context's material, which changes no byte), then everything on at
    120 x 88 and at 60 x 44. After each of the first three frames exactly the getters of the passes that did not run refuse, each with its
    own text; the last frame's colour, depth and six records are the long-lived context's all-on frame as bytes, and its id plane is the
    third frame's and has a mesh wherever a pixel owns a disk."""
    c = _context(native, scene_unit)

    def materials(on):
        for i in range(c.n_meshes()):
            c.set_mesh_material(i, {} if on else None)

    def check_refusals(ran, ids):
        for (name, option, floats, refusal), rec in zip(GETTERS, _records(c, W * H).values()):
            if option in ran:
                assert not isinstance(rec, str) and rec.shape == (W * H, floats), (ran, name)
            else:
                assert isinstance(rec, str) and refusal in rec, (ran, name, rec)
        for name, option in MS_GETTERS:
            if option in ran:
                assert getattr(c, name)() >= 0.0, (ran, name)
            elif option == "disk":
                with pytest.raises(RuntimeError, match="ran no sun disk pass"):
                    getattr(c, name)()
            else:
                assert getattr(c, name)() == 0.0, (ran, name)
        if ids:
            return c.frame_mesh_ids(W * H)
        with pytest.raises(RuntimeError, match=IDS_REFUSAL):
            c.frame_mesh_ids(W * H)

    try:
        for ran in (frozenset(("disk",)), frozenset(("ambient",))):
            assert _equal(_shot(c, native, ran), first[ran]), fo.name(ran)
            check_refusals(ran, False)
        materials(True)
        assert _equal(_shot(c, native, frozenset()), first[frozenset()])
        ids = check_refusals(frozenset(), True)
        _shot(c, native, fo.ALL, *fo.WALK_SIZES[1])
        assert c.frame_mesh_ids(fo.WALK_SIZES[1][0] * fo.WALK_SIZES[1][1]).shape == (fo.WALK_SIZES[1][0] * fo.WALK_SIZES[1][1],)
        assert _equal(_shot(c, native, fo.ALL), first[fo.ALL])
        assert c.frame_mesh_ids(W * H).tobytes() == ids.tobytes()
        owns_disk = first[fo.ALL]["records"]["frame_sun_disk"][:, 3] != 0
        assert owns_disk.sum() > 500 and np.all(ids[owns_disk] >= 0) and np.all(ids >= -1) and np.all(ids < c.n_meshes())
    finally:
        c.close()


# ------------------------------------------------------------------------------------------- against the composed reference
def _trace(c, o, d, t, min_transmittance):
    return c.trace_nerf_rays(np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), np.ascontiguousarray(t, np.float32), min_transmittance)[0]


def _check_against_reference(options, ctx, shot, alone, geo, ambient_fn=sc.no_ambient, s=0, **shading):
    """the records of one shot, each under its own module's rule, then the colour against frame_options_cases.frame fed with what
    ngp_trace_nerf_rays and the context without meshes measure. Returns the figures of the comparison."""
    colour, depth = shot["frame"]
    rec = {k: (v if isinstance(v, str) else v.reshape(H, W, -1)) for k, v in shot["records"].items()}
    tie = geo["primary_unsafe"].reshape(H, W)  # (a primary ray the float64 tracer flags: which triangle, if any, the pixel sees is a float32 tracer's to decide)
    own = geo["owner"].reshape(H, W) & ~tie
    mirror = geo["mirror"]
    measured = dict(n=alone["n"], n_depth=alone["n_depth"])
    out = {}
    assert tie.sum() <= mc.UNSAFE_CAP * W * H
    table = sd.directions(fo.SUN, fo.RADIUS, fo.K, s)
    q_allow = mref.TIE_EPS + mc.GPU_FACTOR * float(np.abs(sc._q32(geo["meshes"], geo["M"], geo["d"], geo["entry"], geo["start"], geo["owner"]).astype(np.float64) - geo["q"])[own.reshape(-1)].max())
    count = None
    if "disk" in options:  # test_sun_disk_gpu.py's _check_mesh_record
        r = rec["frame_sun_disk"]
        assert np.array_equal((r[..., 3] != 0)[~tie], own[~tie]) and np.all(r[r[..., 3] == 0] == 0)
        assert np.abs(r[..., :3].astype(np.float64) - geo["q"].reshape(H, W, 3))[own].max() <= q_allow
        count = _count(r[..., 3])
        count64, flagged = sd.counts(geo["meshes"], r[..., :3][own], table)
        assert np.array_equal(count[own][~flagged], count64[~flagged]) and flagged.sum() <= fo.UNSAFE_CAP * own.sum()
        out["disk_flagged"] = flagged.sum() / float(W * H)
        assert (own & (count > 0) & (count < fo.K)).sum() >= fo.SHARES["disk_partial"] * W * H and (own & (count == fo.K)).sum() >= fo.SHARES["disk_full"] * W * H
    if "sun" in options:  # test_mesh_sun_nerf_shadow_gpu.py: alpha_s is the tracer's at the record's own ray, as bytes; test_sun_disk_gpu.py: live where V > 0
        r = rec["frame_sun_shadow"]
        live = np.any(r[..., :3] != 0, -1)
        assert np.all(r[..., 3][~live] == 0)
        traced = _trace(ctx, r[..., :3][live], np.tile(sc.s_hat(fo.SUN), (int(live.sum()), 1)), np.tile(np.float32([fo.SUN_NERF[1], INF]), (int(live.sum()), 1)), fo.SUN_NERF[0])
        assert r[..., 3][live].tobytes() == traced[:, 3].tobytes() and (r[..., 3] > 0.9).any() and (live & own & (r[..., 3] == 0)).any()
        safe = own & ~(geo["flagged"] if "disk" in options else geo["shadow_unsafe"]).reshape(H, W)
        want_live = (sd.visibility(count, fo.K) > 0) if "disk" in options else ~geo["shadowed"].reshape(H, W)
        assert np.array_equal(live[safe], want_live[safe]) and ("disk" not in options or (own & ~live).sum() > 50)
        assert np.abs(r[..., :3].astype(np.float64) - geo["q"].reshape(H, W, 3))[own & live].max() <= q_allow
        if "disk" in options:
            assert r[..., :3][own & live].tobytes() == rec["frame_sun_disk"][..., :3][own & live].tobytes()
        measured["alpha_s"] = np.zeros((H, W), np.float32)
        measured["alpha_s"][live] = traced[:, 3]
    if "refl" in options:  # test_mesh_reflection_gpu.py's record rule
        r = rec["frame_mesh_reflection"]
        q, t_hit, d, owns = r[..., 0:3], r[..., 3], r[..., 4:7], np.any(r[..., 4:7] != 0, -1)
        assert not np.any(r[~owns]) and np.array_equal(owns[~tie], mirror["owns"][~tie]) and np.all(r[..., 7] == 0)
        traced = _trace(ctx, q[owns], d[owns], np.stack([np.full(int(owns.sum()), fo.REFLECTION["t_min"], np.float32), t_hit[owns]], 1), fo.REFLECTION["min_transmittance"])
        assert r[..., 8:12][owns].tobytes() == traced.tobytes() and (r[..., 11] > 0.9).any() and (owns & (r[..., 11] == 0)).any()
        m = owns & mirror["owns"] & ~mirror["unsafe"] & ~mirror["t_unsafe"]
        assert np.abs(q.astype(np.float64) - mirror["rq"])[m].max() <= mref.TIE_EPS + mc.GPU_FACTOR * mirror["rq_dev"]
        assert np.abs(d.astype(np.float64) - mirror["r"])[m].max() <= mref.TIE_EPS + mc.GPU_FACTOR * mirror["r_dev"]
        assert np.array_equal(np.isfinite(t_hit)[m], mirror["cut"][m])
        mcut = m & mirror["cut"]
        assert mcut.sum() >= fo.SHARES["mirror_cut"] * W * H and (m & ~mirror["cut"]).sum() >= fo.SHARES["mirror_open"] * W * H
        assert np.all(np.abs(t_hit[mcut].astype(np.float64) - mirror["t_hit"][mcut]) <= mc.position_tolerance(mirror["t_dev"], mirror["t_hit"][mcut]))
        measured["reflected"] = np.zeros((H, W, 4), np.float32)
        measured["reflected"][owns] = traced
    if "ambient" in options:  # test_ambient_change_gpu.py's record rules; g then enters the reference as the record holds it
        r = rec["frame_ambient_change"]
        owner = r[..., 3] != 0
        assert np.array_equal(owner, alone["n"][..., 3] > np.float32(nc.OWNER_ALPHA)) and np.all(r[~owner] == 0)
        ratio = ac.case_ratio(r[..., :3][owner], r[..., 4:7][owner])
        keep = ~ratio["tie"]
        err = np.abs(r[..., 8:11][owner].astype(np.float64) - ratio["g"])
        assert ratio["tie"].mean() <= ac.TIE_CAP and np.array_equal(r[..., 3][owner][keep], ratio["state"][keep]) and np.all(err[keep] <= ratio["allow"][keep])
        out["ambient_changed"] = ((r[..., 3] == 2) & np.any(r[..., 8:11] != 1, -1)).sum() / float(W * H)
        assert out["ambient_changed"] >= fo.SHARES["ambient_changed"]
        measured["g"] = np.where((r[..., 3] == 2)[..., None], r[..., 8:11], np.float32(1)).astype(np.float32)
        measured["p"] = r[..., :3]
    if "shadow" in options:
        measured["p"] = rec["frame_mesh_shadow"][..., :3]
    fr = fo.frame(options, measured, ambient_fn=ambient_fn, s=s, **shading)
    if "hits" in options:  # test_mesh_reflection_meshes_gpu.py's test_hit_record_matches_the_reference
        r = rec["frame_mesh_reflection_hits"]
        mr = fr["mesh"]["mirror"]
        hit = r[..., 7] != 0
        safe = ~mr["unsafe"] & ~mr["t_unsafe"] & ~mr["hit_unsafe"]
        assert not np.any(r[~hit]) and np.all(r[..., 7][hit] == 1) and np.array_equal(hit[safe], mr["cut"][safe])
        m = safe & mr["cut"]
        assert np.all(np.abs(r[..., 0:3].astype(np.float64) - mr["p2"])[m].max(-1) <= mc.position_tolerance(mr["p2_dev"], mr["t_hit"][m]))
        assert np.array_equal(r[..., 3][m], mr["shadow2"][m].astype(np.float32))
        out["C2"] = float((np.abs(r[..., 4:7].astype(np.float64) - mr["C2"])[m] / sc.frame_bound(mr["C2"])[m]).max())
        assert out["C2"] <= 1.0 and (m & mr["faces_sun"] & (mr["shadow2"] == 1)).sum() >= 100 and (m & (mr["shadow2"] == 0)).sum() > 0
    if "shadow" in options:  # test_nerf_mesh_shadow_gpu.py's and test_sun_disk_gpu.py's record rules
        r, sh = rec["frame_mesh_shadow"], fr["shadow"]
        owner = r[..., 3] != 0
        assert np.array_equal(owner, alone["n"][..., 3] > np.float32(nc.OWNER_ALPHA)) and np.all(r[~owner] == 0)
        restated = nc.shadow(np.where(owner, 1.0, 0.0), depth, fo.meshes(), matrix_3x4=fo.CAMERA, width=W, height=H, focal=fo.FOCAL)
        assert np.abs(r[..., :3].astype(np.float64) - restated["p"])[owner].max() <= mref.TIE_EPS + mc.GPU_FACTOR * restated["p_dev"]
        keep = owner & ~sh["flagged"]
        assert np.array_equal(r[..., 3][keep], sh["w"][keep]) and sh["flagged"].sum() <= fo.UNSAFE_CAP * owner.sum()
        out["nerf_soft"] = (owner & (sh["count"] > 0)).sum() / float(W * H)
        assert out["nerf_soft"] >= fo.SHARES["nerf_soft"]
        if "ambient" in options:
            assert r[..., :3].tobytes() == rec["frame_ambient_change"][..., :3].tobytes()
    # ---- the colour
    unsafe = fr["unsafe"] | alone["unknown"]
    black = ~geo["owner"].reshape(H, W) & np.all(fr["mesh"]["rgba"][..., :3] == 0, -1)  # the mesh layer is the opaque black of no mesh (with an ambient source such a pixel carries its ambient term)
    no_mesh = black
    m = black & ~unsafe
    assert colour[m].tobytes() == fr["rgba32"][m].tobytes()  # the float32 composite of n, g and f
    m = ~black & ~unsafe
    ratio = np.abs(colour[..., :3].astype(np.float64) - fr["rgba"][..., :3]) / fr["bound"]
    worst = np.unravel_index(np.argmax(np.where(m[..., None], ratio, 0)), ratio.shape)
    out.update(left_out=unsafe.mean(), ratio=float(ratio[m].max()), error=float(np.abs(colour[..., :3].astype(np.float64) - fr["rgba"][..., :3])[worst]), bound=float(fr["bound"][worst]),
               compared=int(m.sum()), alpha_err=float(np.abs(colour[..., 3].astype(np.float64) - fr["rgba"][..., 3])[~unsafe].max()))
    print("\n%s: compared under the bound %d mesh pixels, as bytes %d pixels without a mesh; left out %.2f %% (cap %.0f %%); largest colour deviation / bound %.3f (%.3g against %.3g); %s"
          % (fo.name(options), m.sum(), (no_mesh & ~unsafe).sum(), 100 * unsafe.mean(), 100 * fo.UNSAFE_CAP, out["ratio"], out["error"], out["bound"],
             ", ".join("%s %.3g" % (k, v) for k, v in out.items() if k in ("C2", "disk_flagged", "nerf_soft", "ambient_changed"))))
    assert unsafe.mean() <= fo.UNSAFE_CAP
    assert out["ratio"] <= 1.0, out
    assert out["alpha_err"] <= 4 * 2.0 ** -24
    return out


@pytest.mark.parametrize("which", ["all", "disk+refl+hits", "disk+ambient+shadow", "refl+ambient+shadow"])
def test_frame_matches_the_composed_reference(which, ctx, first, alone):
    """every option on, and the three-option sets the pair tests cannot reach: the records first, each under its own module's rule (counts
    as integers with flagged pixels left out, positions and ratios under those modules' allowances, the traced radiance as bytes against
    ngp_trace_nerf_rays at the record's own rays), then the colour: as bytes against the float32 composite where no mesh covers the pixel,
    elsewhere within the sum of the single-option bounds of the terms present. Pixels left out stay under 3 %.
    Measured on an MI355X: all on, the largest colour deviation is 0.19 of its bound (4.6e-8 against 2.4e-7, a NeRF pixel over a mesh), C2
    0.035 of its bound, 0.61 % of the pixels left out; disk + reflection + sub-option 0.08 (2.5e-8 against 3.3e-7), 0.57 % left out; disk +
    ambient + mesh shadow 0.19, 0.57 %; reflection + ambient + mesh shadow 0.13 (3.0e-8 against 2.4e-7), 0.23 %."""
    options = fo.ALL if which == "all" else frozenset(which.split("+"))
    assert options in (fo.ALL,) + fo.TRIPLES
    _check_against_reference(options, ctx, first[options], alone, fo.geometry())


def test_all_on_with_the_visible_volume(native, scene_unit, first, alone):
    """every option on in ShadeIrradianceVolume with probe visibility held: the mesh pixels and the mirrored hits take their ambient light
    from the visible lookup (the reference shades with E / pi of the context's own ngp_irradiance_volume_at with visibility at its own
    points; with the plain lookup it misses the frame), and the ambient ratio on the NeRF still uses the plain one: its record is the
    Shade frame's as bytes"""
    c = _context(native, scene_unit)
    try:
        c.compute_irradiance_volume_visibility(**VISIBILITY)
        _apply(c, fo.ALL)
        shot = dict(frame=c.render(_cam(native), _opts(native, render_mode=native.RENDER_SHADE_IRRADIANCE_VOLUME), want_depth=True), records=_records(c, W * H))
        c.clear_irradiance_volume_visibility()
        plain = c.render(_cam(native), _opts(native, render_mode=native.RENDER_SHADE_IRRADIANCE_VOLUME), want_depth=True)

        def lookup(visible):
            def ambient(pos, N):
                E = c.irradiance_volume_at(np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(N, np.float32), visible=visible)[:, :3].astype(np.float64)
                return np.maximum(E, 0.0) / np.pi
            return ambient

        c.compute_irradiance_volume_visibility(**VISIBILITY)
        assert shot["frame"][0].tobytes() != plain[0].tobytes() and shot["frame"][1].tobytes() == first[fo.ALL]["frame"][1].tobytes()
        for name in ("frame_ambient_change", "frame_mesh_shadow", "frame_sun_disk", "frame_sun_shadow", "frame_mesh_reflection"):
            assert shot["records"][name].tobytes() == first[fo.ALL]["records"][name].tobytes(), name
        assert shot["records"]["frame_mesh_reflection_hits"].tobytes() != first[fo.ALL]["records"]["frame_mesh_reflection_hits"].tobytes()
        _check_against_reference(fo.ALL, c, shot, alone, fo.geometry(), ambient_fn=lookup(True))
        with pytest.raises(AssertionError):
            _check_against_reference(fo.ALL, c, shot, alone, fo.geometry(), ambient_fn=lookup(False))
    finally:
        c.close()


# ----------------------------------------------------------------------------------------------------------------- structure
def test_two_samples_are_the_mean_of_their_frames(ctx, native):
    """every option on, 2 spp from spp index 0 with jittered samples: the frame is accumulate_tonemap_kernel's mean of the one-sample frames
    of spp index 0 and 1, fl(fl(a + b) / 2), as bytes (background 0, exposure 0, linear: a one-sample frame is its sample); every record is
    the last sample's, the record of the one-sample frame of spp index 1"""
    _apply(ctx, fo.ALL)
    try:
        two = ctx.render(_cam(native, snap=False), _opts(native, spp=2), want_depth=True)
        rec2 = _records(ctx, W * H)
        a = ctx.render(_cam(native, snap=False, spp_index=0), _opts(native), want_depth=True)
        rec_a = _records(ctx, W * H)
        b = ctx.render(_cam(native, snap=False, spp_index=1), _opts(native), want_depth=True)
        rec_b = _records(ctx, W * H)
    finally:
        _apply(ctx, frozenset())
    want = ((a[0] + b[0]).astype(np.float32) / np.float32(2)).astype(np.float32)
    assert two[0].tobytes() == want.tobytes() and a[0].tobytes() != b[0].tobytes() and two[1].tobytes() == b[1].tobytes()
    for name, _, _, _ in GETTERS:
        assert rec2[name].tobytes() == rec_b[name].tobytes() and rec2[name].tobytes() != rec_a[name].tobytes(), name


def _all_records(c, n):
    return np.concatenate([getattr(c, name)(n) for name, _, _, _ in GETTERS], 1)


def test_shards_and_packed_shards_cover_the_frame(ctx, first, native):
    """every option on: three shards in image layout and tile-packed (60 x 44: partial tiles on both axes) make the whole frame, its depth
    and all six records, as bytes"""
    import torch

    world = 3
    cam = _cam(native)
    tile, slot = _tiles(W, H)
    full, full_depth = first[fo.ALL]["frame"]
    full_rec = np.concatenate([first[fo.ALL]["records"][name] for name, _, _, _ in GETTERS], 1).reshape(H, W, -1)
    _apply(ctx, fo.ALL)
    try:
        total, total_depth, total_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        packed, packed_depth, packed_rec = np.zeros_like(full), np.zeros_like(full_depth), np.zeros_like(full_rec)
        for r in range(world):
            mine = tile % world == r
            part, part_depth = ctx.render(cam, _opts(native, shard_index=r, shard_count=world), want_depth=True)
            rec = _all_records(ctx, W * H).reshape(H, W, -1)
            assert not np.any(part[~mine]) and not np.any(rec[~mine])
            total[mine], total_depth[mine], total_rec[mine] = part[mine], part_depth[mine], rec[mine]
            n = native.load_library().ngp_packed_tiles(W, H, r, world) * 64
            rgba = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            dep = torch.zeros((n,), dtype=torch.float32, device="cuda")
            ctx.render_device(cam, _opts(native, shard_index=r, shard_count=world, packed_output=True), rgba.data_ptr(), dep.data_ptr(), None)
            rec = _all_records(ctx, n)  # (synchronises the context's stream)
            src = (tile // world) * 64 + slot
            packed[mine], packed_depth[mine], packed_rec[mine] = rgba.cpu().numpy()[src[mine]], dep.cpu().numpy()[src[mine]], rec[src[mine]]
    finally:
        _apply(ctx, frozenset())
    assert total.tobytes() == full.tobytes() and total_depth.tobytes() == full_depth.tobytes() and total_rec.tobytes() == full_rec.tobytes()
    assert packed.tobytes() == full.tobytes() and packed_depth.tobytes() == full_depth.tobytes() and packed_rec.tobytes() == full_rec.tobytes()


def test_two_devices_render_the_one_device_frame(first, native, scene_unit):
    """every option on, on a context of two devices (the same ordinal twice): the one-device frame as bytes; every record is the primary's
    tile-packed share of the one-device record"""
    multi = _context(native, scene_unit, devices=[0, 0])
    try:
        assert multi.n_devices() == 2
        _apply(multi, fo.ALL)
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), first[fo.ALL]["frame"])
        n = native.load_library().ngp_packed_tiles(W, H, 0, 2) * 64
        tile, slot = _tiles(W, H)
        mine = (tile % 2 == 0).reshape(-1)
        src = ((tile // 2) * 64 + slot).reshape(-1)[mine]
        for name, _, _, _ in GETTERS:
            assert getattr(multi, name)(n)[src].tobytes() == first[fo.ALL]["records"][name][mine].tobytes(), name
        _apply(multi, frozenset())
        assert _same(multi.render(_cam(native), _opts(native), want_depth=True), first[frozenset()]["frame"])
    finally:
        multi.close()


def test_frame_on_a_callers_stream(ctx, first, native):
    """every option on through ngp_render_device on a caller's stream, then the caller's own synchronise: the same bytes, records included"""
    import torch

    rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    _apply(ctx, fo.ALL)
    try:
        ctx.render_device(_cam(native), _opts(native), rgba.data_ptr(), dep.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        shot = dict(frame=(rgba.cpu().numpy(), dep.cpu().numpy()), records=_records(ctx, W * H))
        assert _equal(shot, first[fo.ALL])
    finally:
        _apply(ctx, frozenset())
    assert _equal(_shot(ctx, native, frozenset()), first[frozenset()])  # (and the context's own stream after it)


def test_both_disk_layouts_give_equal_bytes(ctx, first, native, monkeypatch):
    """NGP_SUN_DISK_LAYOUT=thread, read when a frame is rendered as in test_sun_disk_gpu.py: every option on, and the disk with each
    neighbour it shares a buffer with, give the wave layout's colour, depth and records"""
    monkeypatch.setenv("NGP_SUN_DISK_LAYOUT", "thread")
    try:
        for s in (fo.ALL, frozenset(("disk", "refl", "hits")), frozenset(("disk", "sun")), frozenset(("disk", "ambient", "shadow"))):
            assert _equal(_shot(ctx, native, s), first[s]), fo.name(s)
    finally:
        _apply(ctx, frozenset())
