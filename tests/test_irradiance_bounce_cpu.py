"""Bounces without a GPU: the float64 reference's own properties (a black albedo, linearity in the albedo, a constant source, the series
between two facing quads), the share of unsafe rays in every case the GPU file uses, and the library's refusals on a host-only context."""
import re

import numpy as np
import pytest

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import irradiance_visibility_reference as vr
import mesh_visibility_cases as vc
from irradiance_volume_cases import GEN_POINTS, UNSAFE_CAP


@pytest.mark.parametrize("nu,nv", br.RAY_SHAPES)
def test_unsafe_share_is_under_the_cap(nu, nv):
    """from the reference alone, for both lookups of the per-ray stage test; the float32 form's deviation is a rounding error, not a licence"""
    for visible in (False, True):
        case = br.stage_case(nu, nv, visible)
        hit = case["hit"]
        share = hit["unsafe"].mean()
        print("\n%d x %d %s: unsafe %.2f %%, rays with a hit %d of %d, float32 deviation %.2e, allowance %.2e (largest B %.3f)"
              % (nu, nv, "visible" if visible else "plain", 100 * share, case["info"]["mask"].sum(), hit["t"].size, case["dev"], case["allow"], case["B"].max()))
        assert share <= UNSAFE_CAP
        assert case["allow"] < 1e-3 * max(case["B"].max(), 1.0)
    if nu * nv >= 64:
        assert case["info"]["mask"][0].all() and case["info"]["mask"][4].mean() < 0.1  # the probe inside the ball, the probe far away
        assert (case["info"]["W"] < 0.999).any()  # dead probes took part
        assert (case["B"][case["safe"]] > 0.1).any()


def test_end_to_end_cases_are_mostly_safe():
    """the lattices the GPU file bounces on, their own probes' rays: few unsafe, every probe sees a mesh and the open, and every probe lies
    inside the NeRF's unit cube"""
    for (res, lo, hi, nu, nv), scene in ((br.E2E_CASE, br.e2e_scene()), (br.FLOOR_CASE[1:], br.floor_scene())):
        probes = vr.probe_positions(res, lo, hi)
        hit = br.hits(br.normalised(scene), probes, nu, nv)
        blocked = (hit["tri"] >= 0).mean(1)
        assert hit["unsafe"].mean() <= UNSAFE_CAP and np.all(blocked > 0) and np.all(blocked < 1), blocked
        assert np.all(probes > 0) and np.all(probes < 1)
    floor = br.normalised(br.floor_scene())[0]
    assert -0.11 < floor[..., 1].min() and floor[..., 1].max() < -0.09 and floor[..., 0].min() < 0.01 and floor[..., 0].max() > 0.99


def _stage(nu=9, nv=9, albedo=br.STAGE_ALBEDO, sh=None, alpha=True):
    v, res, lo, hi = br.stage_volume()
    hit = br.hits(br.stage_meshes(), GEN_POINTS, nu, nv)
    a = br.stage_alpha(GEN_POINTS.shape[0], nu * nv) if alpha else None
    B, _ = br.bounce_rays(hit, GEN_POINTS, nu, nv, albedo, a, br.source(v if sh is None else sh, res, lo, hi))
    return B, hit, a


def test_black_albedo_gives_nothing():
    B, hit, _ = _stage(albedo=0.0)
    assert np.all(B == 0) and np.all(br.records(B, hit["t"], 9, 9)[:, :27] == 0)


def test_linear_in_the_albedo():
    B1, hit, _ = _stage(albedo=np.float32([0.25, 0.125, 0.5]))
    B2, _, _ = _stage(albedo=np.float32([0.5, 0.25, 1.0]))
    R1, R2 = br.records(B1, hit["t"], 9, 9), br.records(B2, hit["t"], 9, 9)
    assert np.abs(R1[:, :27]).max() > 1e-2 and np.abs(R2[:, :27] - 2 * R1[:, :27]).max() < 1e-14
    assert np.array_equal(R1[:, 27], R2[:, 27])


def test_constant_source():
    """a volume of the constant record L: M = albedo L on every blocked ray, so R's first coefficient is the constant record's, weighted by
    the blocked, unattenuated share of the rays"""
    L = 0.7
    sh = np.tile(vc.constant_record(L), (12, 1))
    B, hit, alpha = _stage(sh=sh)
    mask = hit["tri"] >= 0
    want = (1.0 - alpha.astype(np.float64))[..., None] * br.STAGE_ALBEDO.astype(np.float64) * L
    assert np.abs(B[mask] - want[mask]).max() < 1e-6 and np.all(B[~mask] == 0)  # (the float32 records round the constant: 6e-8)
    R = br.records(B, hit["t"], 9, 9)
    weight = (mask * (1.0 - alpha)).mean(1)
    assert np.abs(R[:, :3] - weight[:, None] * br.STAGE_ALBEDO * vc.constant_record(L)[0]).max() < 1e-6
    assert np.array_equal(R[:, 27], (~mask).mean(1))


def test_series_between_two_facing_quads():
    """two large quads facing each other across a lattice that holds the constant radiance L: every pass adds light, and the radiance a hit
    throws back stays under L (q + q^2 + ... + q^b). q = albedo x 1.0625 x 1.02: E of nine coefficients overshoots the true irradiance of a
    non-negative radiance by at most sum_l A_l (2 l + 1) / (4 pi) = 1.0625 (a point light), the 16 x 16 quadrature by at most 1.29 %
    (include/ngp_hip.h), and the true irradiance of a radiance below X is below pi X."""
    quad = lambda z, flip: np.float32([[[-1, -1, z], [2, -1, z], [2, 2, z]], [[-1, -1, z], [2, 2, z], [-1, 2, z]]])[:, ::flip]
    meshes = [quad(0.0, 1), quad(1.0, -1)]
    res, lo, hi, L, albedo, N = (2, 2, 2), np.float32([0.2] * 3), np.float32([0.8] * 3), 1.0, 0.5, 4
    series = br.bounced(meshes, np.tile(vc.constant_record(L), (8, 1)), res, lo, hi, 16, 16, albedo, N)
    probes = vr.probe_positions(res, lo, hi)
    hit = br.hits(meshes, probes, 16, 16)
    assert hit["unsafe"].mean() <= UNSAFE_CAP and 0.5 < (hit["tri"] >= 0).mean() < 1
    q, bound = albedo * 1.0625 * 1.02, 0.0
    for b in range(1, N + 1):
        B, _ = br.bounce_rays(hit, probes, 16, 16, albedo, None, br.source(series[b - 1].astype(np.float32), res, lo, hi))
        bound = q * (L + bound)
        print("bounce %d: c_0 %.4f -> %.4f, largest B %.4f (bound %.4f)" % (b, series[b - 1][:, 0].max(), series[b][:, 0].max(), B.max(), bound))
        assert np.all(series[b][:, 0] > series[b - 1][:, 0]) and B.max() <= bound
        assert np.array_equal(series[b][:, 27], series[0][:, 27])
    assert series[N][:, 0].max() - series[N - 1][:, 0].max() < 0.5 * (series[1][:, 0].max() - series[0][:, 0].max())  # (and the steps shrink)


# ------------------------------------------------------------------------------------------------------------ the library
def test_bounce_desc_layout(native):
    C = native.C
    s = native.IrradianceBounceDesc
    assert [f for f, _ in s._fields_] == ["n_bounces", "albedo"] and C.sizeof(s) == 16 and s.albedo.offset == 4
    with open(native.HEADER_PATH) as f:
        h = f.read()
    body = re.search(r"typedef struct ngp_irradiance_bounce_desc \{(.*?)\} ngp_irradiance_bounce_desc;", h, re.S).group(1)
    assert re.findall(r"\b(n_bounces|albedo)\b(?=[\[,;])", body) == ["n_bounces", "albedo"]


def test_bounce_entries_refuse_host_only_and_bad_descriptors(native):
    L = native.load_library()
    for name in ("ngp_compute_irradiance_volume_bounced", "ngp_irradiance_sh_bounce", "ngp_get_irradiance_bounce_ms"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    ctx = native.Context(-1)
    p = np.float32([[0.5, 0.5, 0.5]])
    box = (np.float32([0, 0, 0]), np.float32([1, 1, 1]))
    for call in (lambda: ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, bounces=1, albedo=0.5), lambda: ctx.irradiance_sh_bounce(p, 0.5, 4, 4),
                 lambda: ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, bounces=2, albedo=(0.1, 0.2, 0.3), visibility=dict(n_u=4, n_v=4)), lambda: ctx.irradiance_bounce_ms()):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    # the descriptor is looked at first: each refusal names its field
    with pytest.raises(RuntimeError, match="n_bounces must be at most 16"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, bounces=17, albedo=0.5)
    for bad in (1.5, -0.1, float("nan"), float("inf"), (0.5, 0.5, 1.5), (float("nan"), 0.5, 0.5)):
        with pytest.raises(RuntimeError, match="albedo must be finite and in"):
            ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, bounces=1, albedo=bad)
        with pytest.raises(RuntimeError, match="albedo must be finite and in"):
            ctx.irradiance_sh_bounce(p, bad, 4, 4)
    # the argument checks of native.py come before the library
    with pytest.raises(ValueError, match="belong to bounces"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, albedo=0.5)
    with pytest.raises(ValueError, match="n x K values"):
        ctx.irradiance_sh_bounce(p, 0.5, 4, 4, alpha=np.zeros(15, np.float32))
    ctx.close()
