"""The NeRF shadow of the sun pass without a GPU: the mix of blocked and open shadow rays in the floor case as the oracle traces them, what
B' = max(1 - alpha_s, 0) B can and cannot do, the new descriptor's layout and the library's refusals on a host-only context."""
import re

import numpy as np
import pytest

import irradiance_bounce_reference as br
import irradiance_sh_reference as sh_ref
import irradiance_sun_reference as sr
import irradiance_sun_shadow_reference as ssr
from test_irradiance_traced import _box_start, _cam_along, _linear, _oracle_payloads

FLOOR_SUN = (1.0, 1.0, 1.0)
BLOCKED_SHARE, OPEN_SHARE = 0.15, 0.50  # of the lit rays: alpha_s > 0.9, alpha_s = 0
TEST_POINTS = np.float32([[0.5, 0.05, 0.5], [0.3, 0.1, 0.6]])
DOWN = np.float32([[0, -1, 0], [0, -1, 0]])
_cache = {}


def oracle_alpha(oracle, scene, q, sun, box, t_min=0.0):
    """alpha of rays from q (n, 3) along the unit sun direction through the oracle's trace of `scene`, as test_irradiance_traced.py calls it:
    `box` is the render box of the oracle's model, the rays start at the contract's t_start for it, and the probe rule zeroes what is not
    shaded"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
    d = np.tile(sr.unit_sun(sun), (q.shape[0], 1))
    t0, alive = _box_start(q, d, box[0], box[1], np.full(q.shape[0], t_min, np.float32))
    m = oracle.make_model(dict(scene, render_aabb=(tuple(float(x) for x in box[0]), tuple(float(x) for x in box[1]))))
    rgba, _, _ = oracle.trace_payloads(m, _cam_along(np.zeros(3), np.zeros(3)), _oracle_payloads(q, d, t0, alive), oracle.make_opts(capped_skip=True))
    oracle.release(m)
    return _linear(oracle, rgba)[:, 3]


def mix(alpha_s):
    """(share with alpha_s > 0.9, share with alpha_s = 0) of the lit rays' alpha_s"""
    a = np.asarray(alpha_s)
    return float((a > 0.9).mean()), float((a == 0).mean())


def floor_case(oracle, scene_unit):
    """FLOOR_CASE under the sun (1, 1, 1): irradiance_sun_shadow_reference.case, B (float32, the sun pass's float32 form without a NeRF in
    front of the hits) and alpha_s (P, K; the oracle's on the reference's q with the unit cube as render box, 0 where there is no shadow ray)"""
    if "floor" not in _cache:
        albedo, res, lo, hi, nu, nv = br.FLOOR_CASE
        c = ssr.case(br.floor_scene(), res, lo, hi, nu, nv, FLOOR_SUN)
        B, _ = sr.sun_rays(c["hit"], c["probes"], nu, nv, FLOOR_SUN, sr.STAGE_RADIANCE, sr.STAGE_BIAS, albedo, None, np.float32)
        alpha_s = np.zeros(c["lit"].shape, np.float32)
        alpha_s[c["lit"]] = oracle_alpha(oracle, scene_unit, c["q"][c["lit"]], FLOOR_SUN, scene_unit["render_aabb"])
        _cache["floor"] = dict(c, B=B.astype(np.float32), alpha_s=alpha_s)
    return _cache["floor"]


def test_floor_case_has_blocked_and_open_shadow_rays(oracle, scene_unit):
    """conditions on the case, not tolerances: at least 15 % of the lit rays are blocked (alpha_s > 0.9), at least 50 % open (alpha_s = 0),
    and no ray is unsafe. Measured: 66 blocked and 201 open of 272."""
    c = floor_case(oracle, scene_unit)
    a = c["alpha_s"][c["lit"]]
    blocked, open_ = mix(a)
    print("\nfloor case: %d rays, lit %d, alpha_s > 0.9: %d, = 0: %d, between: %d, unsafe %d, float32 deviation of q %.2e"
          % (c["lit"].size, c["lit"].sum(), (a > 0.9).sum(), (a == 0).sum(), ((a > 0) & (a <= 0.9)).sum(), c["unsafe"].sum(), c["dev"]))
    assert c["lit"].size == 2048 and c["lit"].sum() > 100
    assert blocked >= BLOCKED_SHARE and open_ >= OPEN_SHARE
    assert not c["unsafe"].any()
    assert np.all(c["q"][~c["lit"]] == 0) and np.all(c["q32"][~c["lit"]] == 0)
    assert c["dev"] < 1e-6  # float32 of points of size 1, a few roundings


def test_the_shadow_only_takes_away(oracle, scene_unit):
    """B' <= B per ray and channel, B' = B as bytes where alpha_s = 0; under FLOOR_CASE's two points E(down) from the projection of B' is <= E
    from B on every channel and strictly below it on at least one point: every floor ray has a positive cosine to that normal and the SH9
    kernel is positive there, so a smaller radiance is a smaller E"""
    albedo, res, lo, hi, nu, nv = br.FLOOR_CASE
    c = floor_case(oracle, scene_unit)
    B, a = c["B"], c["alpha_s"]
    Bs = ssr.apply(B, a)
    assert Bs.dtype == np.float32 and B.max() > 0.1
    assert np.all(Bs <= B) and np.all(Bs >= 0)
    assert Bs[a == 0].tobytes() == B[a == 0].tobytes() and (a == 0).sum() > 1000
    assert np.all(Bs[a >= 1] == 0) and (Bs < B).any()
    # alpha above 1 (a tracer's rounding) clamps to no light, not to negative light
    assert np.all(ssr.apply(np.float32([[1, 2, 3]]), np.float32([1.0000001])) == 0)
    E = []
    for rays in (B, Bs):
        S = sr.sunlit(np.zeros((c["probes"].shape[0], 28)), rays, nu, nv)
        S[:, 27] = 1.0
        e, W = sh_ref.lookup(S, res, lo, hi, TEST_POINTS, DOWN)
        assert np.all(W > 0)
        E.append(e)
    print("\nE(down) from B %s, from B' %s" % (E[0], E[1]))
    assert np.all(E[1] <= E[0]) and np.all(E[1] > 0)
    assert np.any(np.all(E[1] < E[0], axis=1))


# ------------------------------------------------------------------------------------------------------------ the library
def test_sun_nerf_desc_layout(native):
    C = native.C
    s = native.IrradianceSunNerfDesc
    assert [f for f, _ in s._fields_] == ["min_transmittance", "t_min"] and C.sizeof(s) == 8 and s.min_transmittance.offset == 0 and s.t_min.offset == 4
    with open(native.HEADER_PATH) as f:
        h = f.read()
    body = re.search(r"typedef struct ngp_irradiance_sun_nerf_desc \{(.*?)\} ngp_irradiance_sun_nerf_desc;", h, re.S).group(1)
    assert re.findall(r"\b(min_transmittance|t_min)\b(?=[\[,;])", body) == ["min_transmittance", "t_min"]
    d = native.Context._sun_nerf_desc(True)
    assert (d.min_transmittance, d.t_min) == (np.float32(0.01), 0.0)
    d = native.Context._sun_nerf_desc({"t_min": 0.25})
    assert (d.min_transmittance, d.t_min) == (np.float32(0.01), 0.25)
    d = native.Context._sun_nerf_desc((0.5, 2.0))
    assert (d.min_transmittance, d.t_min) == (0.5, 2.0)
    assert native.Context._sun_nerf_desc(None) is None and native.Context._sun_nerf_desc(False) is None


def test_shadowed_entries_refuse_host_only_and_bad_descriptors(native):
    L = native.load_library()
    for name in ("ngp_compute_irradiance_volume_sunlit_shadowed", "ngp_irradiance_sh_sun_shadowed", "ngp_get_irradiance_sun_shadow_ms"):
        assert name in native.EXPORTS and getattr(L, name).argtypes is not None
    C = native.C
    ctx = native.Context(-1)
    p = np.float32([[0.5, 0.5, 0.5]])
    box = (np.float32([0, 0, 0]), np.float32([1, 1, 1]))
    up = {"direction": (0, 1, 0)}
    for call in (lambda: ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=up, sun_nerf_shadow=True),
                 lambda: ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, bounces=1, sun_nerf_shadow=(0.02, 0.5)),
                 lambda: ctx.irradiance_sh_sun(p, up, 0.5, 4, 4, nerf_shadow=True), lambda: ctx.irradiance_sun_shadow_ms()):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    # the stage entry traces the model, and says so
    with pytest.raises(RuntimeError, match="model"):
        ctx.irradiance_sh_sun(p, up, 0.5, 4, 4, nerf_shadow=True, return_rays=True, return_shadow=True)
    # the descriptors are looked at first, the bounce's, the sun's, then the new one: each refusal names its field
    nan, inf = float("nan"), float("inf")
    bad = [(dict(min_transmittance=nan), "min_transmittance is NaN"), (dict(t_min=-1e-3), "t_min must be finite and >= 0"), (dict(t_min=nan), "t_min"), (dict(t_min=inf), "t_min"),
           (dict(t_min=-inf), "t_min")]
    for shadow, message in bad:
        with pytest.raises(RuntimeError, match="invalid irradiance sun NeRF descriptor: " + message):
            ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=up, sun_nerf_shadow=shadow)
        with pytest.raises(RuntimeError, match="invalid irradiance sun NeRF descriptor: " + message):
            ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun_nerf_shadow=shadow)  # (and without a sun)
        with pytest.raises(RuntimeError, match="invalid irradiance sun NeRF descriptor: " + message):
            ctx.irradiance_sh_sun(p, up, 0.5, 4, 4, nerf_shadow=shadow)
    bad_shadow = dict(t_min=-1.0)
    with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: shadow_bias"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=dict(direction=(0, 1, 0), shadow_bias=-1.0), sun_nerf_shadow=bad_shadow)
    with pytest.raises(RuntimeError, match="albedo must be finite and in"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, albedo=1.5, sun=dict(direction=(0, 0, 0)), sun_nerf_shadow=bad_shadow)
    with pytest.raises(RuntimeError, match="n_bounces must be at most 16"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, bounces=17, sun=up, sun_nerf_shadow=bad_shadow)
    with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: direction"):
        ctx.irradiance_sh_sun(p, dict(direction=(0, 0, 0)), 0.5, 4, 4, nerf_shadow=bad_shadow)
    # a min_transmittance <= 0 or above 1 is no refusal (<= 0 selects 0.01, as in ngp_trace_nerf_rays)
    for mt in (0.0, -1.0, 2.0, inf):
        with pytest.raises(RuntimeError, match="no HIP device"):
            ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=up, sun_nerf_shadow=(mt, 0.0))
    # a sun without the bounce descriptor that carries the albedo, and no descriptors at all, through the C ABI alone
    d = ctx._volume_desc((2, 2, 2), box, ctx._sh_desc(4, 4, True, 0.01))
    ns = ctx._sun_nerf_desc(True)
    with pytest.raises(RuntimeError, match="invalid irradiance sun descriptor: the bounce descriptor"):
        ctx._check(L.ngp_compute_irradiance_volume_sunlit_shadowed(ctx.h, C.byref(d), None, None, C.byref(ctx._sun_desc(up)), C.byref(ns)))
    with pytest.raises(RuntimeError, match="null argument"):
        ctx._check(L.ngp_compute_irradiance_volume_sunlit_shadowed(ctx.h, C.byref(d), None, None, None, C.byref(ns)))
    sh = ctx._sh_desc(4, 4, True, 0.01)
    albedo = np.float32([0.5] * 3)
    with pytest.raises(RuntimeError, match="null argument"):
        ctx._check(L.ngp_irradiance_sh_sun_shadowed(ctx.h, 1, p.ctypes.data, C.byref(sh), C.byref(ctx._sun_desc(up)), albedo.ctypes.data, None, None, None, None, None))
    with pytest.raises(RuntimeError, match="null argument"):
        ctx._check(L.ngp_irradiance_sh_sun_shadowed(ctx.h, 1, p.ctypes.data, C.byref(sh), None, albedo.ctypes.data, None, C.byref(ns), None, None, None))
    # the argument checks of native.py come before the library
    with pytest.raises(ValueError, match="sun_nerf_shadow: min_transmittance and t_min"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=up, sun_nerf_shadow=dict(tmin=0.0))
    with pytest.raises(ValueError, match="sun: direction"):
        ctx.compute_irradiance_volume((2, 2, 2), box, 4, 4, sun=dict(direction=(0, 1, 0), t_min=0.0), sun_nerf_shadow=True)  # the sun dict keeps refusing unknown keys
    with pytest.raises(ValueError, match="return_shadow belongs to nerf_shadow"):
        ctx.irradiance_sh_sun(p, up, 0.5, 4, 4, return_shadow=True)
    ctx.close()
