"""What the inserted meshes change in the ambient light on the NeRF, without a GPU (include/ngp_hip.h, "ambient"): the conditions the case has
to meet as the oracle renders it, the identities of the float64 restatement, the branches of the ratio on a volume with dead probes, the
share of tie cases among the stage tests' points, and the option, its descriptor and the reference volume's entries on a host-only
context."""
import numpy as np
import pytest

import ambient_change_cases as ac
import irradiance_volume_cases as ivc
import mesh_volume_cases as mv
import nerf_mesh_shadow_cases as nc
from test_nerf_mesh_shadow_cpu import oracle_frames

_cache = {}


def oracle_case(oracle, scene_unit):
    """the owners of the case through the oracle, once per process: owner (h, w), p (k, 3) float32, grad (k, 3), N (k, 3) and the ratio there"""
    if "case" not in _cache:
        fr = oracle_frames(oracle, scene_unit)
        owner = fr["n"][..., 3] > np.float32(nc.OWNER_ALPHA)
        p = nc.surface_points32(fr["depth"])[owner.reshape(-1)]
        model = oracle.make_model(scene_unit)
        grad = oracle.density_gradient(model, p)  # (the unit model's box is the unit cube: the warped position is p itself)
        oracle.release(model)
        N, ok = ac.normals_from_gradient(grad)
        _cache["case"] = dict(owner=owner, p=p, grad=grad, N=N, ok=ok, ratio=ac.case_ratio(p, np.where(ok[:, None], N, 1.0)))
    return _cache["case"]


def test_case_changes_the_light_on_the_owners(oracle, scene_unit):
    """conditions on the case, not tolerances; the measured values are in the test's own output and in DESIGN 3.17"""
    c = oracle_case(oracle, scene_unit)
    after, before, hit = ac.volumes()
    r, owners = c["ratio"], int(c["owner"].sum())
    g = r["g"]
    glen = np.linalg.norm(c["grad"].astype(np.float64), axis=1)
    dead = int((after[:, 27] == 0).sum() + (before[:, 27] == 0).sum())
    under = (g.min(1) < 0.9).mean()
    spread = np.median(g.max(1) - g.min(1))
    print("\n%d owners; smallest |grad| %.3g; dead probes %d; W_after == 0 on %d, W_before == 0 on %d; min E_before %.3g; g %.3f .. %.3f; a channel under 0.9 on %.1f %%; "
          "median spread between channels %.3f; unsafe hit rays %.2f %%; ties %d"
          % (owners, glen.min(), dead, (r["W_a"] == 0).sum(), (r["W_b"] == 0).sum(), r["E_b"].min(), g.min(), g.max(), 100 * under, spread, 100 * hit["unsafe"].mean(), r["tie"].sum()))
    assert owners >= 200
    assert c["ok"].all() and glen.min() > 0
    assert dead == 0
    assert np.all(r["W_a"] > 0) and np.all(r["W_b"] > 0) and np.all(r["state"] == 2)
    assert r["E_b"].min() >= 100 * ac.MIN_IRRADIANCE
    assert g.max() < ac.MAX_GAIN
    assert under >= 0.30
    assert g.max() - g.min() >= 0.2
    assert spread > 0.01
    assert hit["unsafe"].mean() <= ivc.UNSAFE_CAP


def test_equal_volumes_change_nothing(oracle, scene_unit):
    """equal records give g = 1 exactly, whatever N is, and the composite is the oracle's own hybrid frame, array for array"""
    c, fr = oracle_case(oracle, scene_unit), oracle_frames(oracle, scene_unit)
    after, before, _ = ac.volumes()
    for vol in (after, before):
        r = ac.ratio(vol, vol, ac.RES, ac.LO, ac.HI, c["p"], c["N"])
        assert np.all(r["g"] == 1.0) and np.all(r["state"] == 2)
    p, n = ac.stage_points(ac.RES, ac.LO, ac.HI)
    a, _, res, lo, hi = ac.varying_pair()
    assert np.all(ac.ratio(a, a, res, lo, hi, p, n)["g"] == 1.0)
    g = np.ones(fr["n"].shape[:2] + (3,), np.float32)
    assert np.array_equal(ac.composite(fr["n"], fr["m"], g, np.ones(g.shape[:2], np.float32)), fr["full"])


def test_a_ratio_below_one_only_takes_away(oracle, scene_unit):
    """g <= 1 never brightens a pixel; alpha is never touched (depth is not an input of the composite at all)"""
    c, fr = oracle_case(oracle, scene_unit), oracle_frames(oracle, scene_unit)
    assert c["ratio"]["g"].max() <= 1.0
    g = np.ones(fr["n"].shape[:2] + (3,), np.float32)
    g[c["owner"]] = c["ratio"]["g"].astype(np.float32)
    one = np.ones(g.shape[:2], np.float32)
    on = ac.composite(fr["n"], fr["m"], g, one)
    off = fr["full"]
    assert np.all(on <= off) and np.array_equal(on[..., 3], off[..., 3])
    assert np.array_equal(on[~c["owner"]], off[~c["owner"]])
    changed = (on != off).any(-1)
    assert changed[c["owner"]].mean() >= 0.30
    # with the meshes' sun shadow too: f scales what g left
    half = np.where(c["owner"], np.float32(0.5), np.float32(1))
    both = ac.composite(fr["n"], fr["m"], g, half)
    assert np.all(both <= on) and np.array_equal(both[..., 3], off[..., 3])


def test_branches_on_a_volume_with_dead_probes():
    """mesh_volume_cases.varying_volume: a point whose live corners carry no weight gives state 1 and g = 1; a channel with E_before <=
    min_irradiance gives g = 1; a ratio above max_gain is capped"""
    after, before, res, lo, hi = ac.varying_pair()
    pts = sh_ref_points(res, lo, hi)
    (i0, j, k), (i1, _, _) = mv.VARYING_DEAD
    edge = 0.5 * (pts[i0 + res[0] * (j + res[1] * k)] + pts[i1 + res[0] * (j + res[1] * k)])  # between the two dead probes, on their lattice line
    r = ac.ratio(after, before, res, lo, hi, edge[None], np.float64([[0.0, 0.0, 1.0]]))
    assert r["W_a"][0] == 0 and r["W_b"][0] == 0 and r["state"][0] == 1 and np.all(r["g"][0] == 1)
    only_after = before.copy()
    only_after[:, 27] = 1.0  # dead in one volume is enough
    r = ac.ratio(after, only_after, res, lo, hi, edge[None], np.float64([[0.0, 0.0, 1.0]]))
    assert r["W_a"][0] == 0 and r["W_b"][0] > 0 and r["state"][0] == 1 and np.all(r["g"][0] == 1)
    p, n = ac.stage_points(res, lo, hi)
    r = ac.ratio(after, before, res, lo, hi, p, n)
    low = (r["E_b"] <= ac.MIN_IRRADIANCE) & (r["state"] == 2)[:, None]
    capped = (np.maximum(r["E_a"], 0) > ac.MAX_GAIN * r["E_b"]) & (r["E_b"] > ac.MIN_IRRADIANCE) & (r["state"] == 2)[:, None]
    plain = (r["state"] == 2)[:, None] & ~low & ~capped
    print("\nvarying pair: state 1 on %d of %d points; E_before <= min on %d channels; capped %d; plain %d; a clamped at 0 on %d" % ((r["state"] == 1).sum(), p.shape[0], low.sum(), capped.sum(), plain.sum(), ((r["E_a"] < 0) & plain).sum()))
    assert low.sum() >= 5 and capped.sum() >= 5 and plain.sum() >= 100 and ((r["E_a"] < 0) & plain).sum() >= 1
    none = r["state"] == 1
    assert none.sum() >= 3 and np.all(r["W_b"][none] == 0) and np.all(r["W_a"][none] > 0) and np.all(r["g"][none] == 1)
    assert np.all(r["g"][low] == 1) and np.all(r["g"][capped] == ac.MAX_GAIN)
    assert np.allclose(r["g"][plain], np.maximum(r["E_a"], 0)[plain] / r["E_b"][plain], rtol=0, atol=1e-15) and np.all(r["g"] >= 0) and np.all(r["g"] <= ac.MAX_GAIN)
    big = ac.ratio(after, before, res, lo, hi, p, n, min_irradiance=1e9)
    assert np.all(big["g"] == 1) and np.array_equal(big["state"], r["state"])


def sh_ref_points(res, lo, hi):
    import irradiance_sh_reference as sh_ref

    return sh_ref.volume_points(res, np.asarray(lo, np.float32), np.asarray(hi, np.float32))


def test_stage_points_hold_few_ties():
    """the points the GPU stage test evaluates: by the float64 reference alone at most TIE_CAP of them are tie cases, in the case's volumes
    and in the varying pair; in the case's volumes, where E_before is far from 0, the tolerance is far below the effect"""
    after, before, _ = ac.volumes()
    for name, (a, b, res, lo, hi) in (("case", (after, before, ac.RES, ac.LO, ac.HI)), ("varying", ac.varying_pair())):
        p, n = ac.stage_points(res, lo, hi)
        r = ac.ratio(a, b, res, lo, hi, p, n)
        lo64, hi64 = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        inside = np.all((p >= lo64) & (p <= hi64), 1)
        print("\n%s: %d points (%d inside the box), ties %d (%.2f %%), state 1 on %d, largest allowance %.3g" % (name, p.shape[0], inside.sum(), r["tie"].sum(), 100 * r["tie"].mean(), (r["state"] == 1).sum(), r["allow"][~r["tie"]].max()))
        assert inside.sum() >= 100 and (~inside).sum() >= 100
        assert r["tie"].mean() <= ac.TIE_CAP
        assert name != "case" or r["allow"][~r["tie"]].max() < 1e-3


# ------------------------------------------------------------------------------------------------------------ the library
def test_option_round_trip_and_refusals_on_a_host_only_context(native):
    L = native.load_library()
    for name in ("ngp_set_ambient_change_on_nerf", "ngp_get_ambient_change_on_nerf", "ngp_get_frame_ambient_change", "ngp_get_frame_ambient_change_ms",
                 "ngp_compute_reference_irradiance_volume", "ngp_set_reference_irradiance_volume", "ngp_get_reference_irradiance_volume", "ngp_clear_reference_irradiance_volume",
                 "ngp_irradiance_volume_ratio"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    try:
        assert ctx.ambient_change_on_nerf() is None  # off by default
        ctx.set_ambient_change_on_nerf(True)
        assert ctx.ambient_change_on_nerf() == dict(min_irradiance=np.float32(1e-3), max_gain=4.0)
        ctx.set_ambient_change_on_nerf(dict(min_irradiance=0.25, max_gain=2.0))
        assert ctx.ambient_change_on_nerf() == dict(min_irradiance=0.25, max_gain=2.0)
        ctx.set_ambient_change_on_nerf(dict(max_gain=1.0))
        assert ctx.ambient_change_on_nerf() == dict(min_irradiance=np.float32(1e-3), max_gain=1.0)
        ctx.set_ambient_change_on_nerf(dict(min_irradiance=0.0))
        assert ctx.ambient_change_on_nerf() == dict(min_irradiance=0.0, max_gain=4.0)
        nan, inf = float("nan"), float("inf")
        ctx.set_ambient_change_on_nerf(dict(min_irradiance=0.5, max_gain=8.0))
        for change, message in ((dict(min_irradiance=nan), "min_irradiance must be finite and >= 0"), (dict(min_irradiance=-1e-3), "min_irradiance"), (dict(min_irradiance=inf), "min_irradiance"),
                                (dict(max_gain=nan), "max_gain must be finite and >= 1"), (dict(max_gain=0.999), "max_gain"), (dict(max_gain=inf), "max_gain"), (dict(max_gain=-inf), "max_gain")):
            with pytest.raises(RuntimeError, match="invalid ambient change descriptor: " + message):
                ctx.set_ambient_change_on_nerf(change)
            assert ctx.ambient_change_on_nerf() == dict(min_irradiance=0.5, max_gain=8.0)  # a refused call leaves the option alone
        with pytest.raises(ValueError, match="ambient_change_on_nerf"):
            ctx.set_ambient_change_on_nerf(dict(max_gian=2.0))
        for off in (None, False):
            ctx.set_ambient_change_on_nerf(True)
            ctx.set_ambient_change_on_nerf(off)
            assert ctx.ambient_change_on_nerf() is None
        with pytest.raises(RuntimeError, match="null argument"):
            ctx._check(L.ngp_get_ambient_change_on_nerf(ctx.h, None, None))
        # the stage entries and the reference volume need a device, as the volume's own entries do there
        sh, res, lo, hi = mv.varying_volume()
        for call in (lambda: ctx.frame_ambient_change(16), lambda: ctx.frame_ambient_change_ms(), lambda: ctx.set_reference_irradiance_volume(mv.as_grid(sh, res), (lo, hi)),
                     lambda: ctx.reference_irradiance_volume(), lambda: ctx.clear_reference_irradiance_volume(),
                     lambda: ctx.irradiance_volume_ratio(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))):
            with pytest.raises(RuntimeError, match="no HIP device"):
                call()
        for call in (lambda: ctx.set_irradiance_volume(mv.as_grid(sh, res), (lo, hi)), lambda: ctx.get_irradiance_volume(), lambda: ctx.clear_irradiance_volume()):
            with pytest.raises(RuntimeError, match="no HIP device"):  # (the existing entries: the same words)
                call()
        with pytest.raises(RuntimeError):
            ctx.compute_reference_irradiance_volume(ac.RES, (ac.LO, ac.HI), ac.N_U, ac.N_V)
    finally:
        ctx.close()
