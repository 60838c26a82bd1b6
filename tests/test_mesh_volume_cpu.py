"""The float64 side of the ShadeIrradianceVolume tests (mesh_volume_cases.py), without a device: the restated mesh pass is the existing
reference, the sky volume holds the sky term exactly, the varying volume's frame reaches the branches the GPU test is after (dead probes,
the clamp, lit pixels) on enough safe pixels, and the position term of the GPU colour bound does not loosen it."""
import numpy as np

import irradiance_sh_reference as sh_ref
import mesh_cases as mc
import mesh_reference as ref
import mesh_volume_cases as mv


def test_restated_render_is_the_reference():
    meshes = mc.normalised(mc.render_scene())
    for name in ("ambient_x", "sun_down"):
        opts = dict(mc.FRAMES[name])
        fn = mv.sky_ambient_fn(opts.pop("ambientcolor"), opts.pop("up_dir", (0.0, 1.0, 0.0)))
        got = mv.render_with_ambient(meshes, mc.camera_matrix(name), mc.WIDTH, mc.HEIGHT, mc.focal(name), fn, **opts)
        want = mc.reference_frame(name)
        for key in ("rgba", "depth", "unsafe", "covered", "shadowed", "lit", "occluded"):
            assert np.array_equal(got[key], want[key]), (name, key)
        assert got["pos"].shape == (mc.HEIGHT, mc.WIDTH, 3) and np.abs(np.linalg.norm(got["N"], axis=-1) - 1).max() < 1e-12


def test_sky_volume_holds_the_sky_term():
    sh, res, lo, hi = mv.sky_volume()
    assert res == (2, 2, 2) and sh.shape == (8, 28) and np.all(sh[:, 27] == 1)
    rng = np.random.default_rng(3)
    n = ref._unit(rng.normal(size=(1000, 3)))
    p = rng.uniform(np.float64(lo) - 1.0, np.float64(hi) + 1.0, (1000, 3))  # (some outside the box: clamped onto it)
    E, W = sh_ref.lookup(sh, res, lo, hi, p, n)
    want = mv.sky_ambient_fn(mv.SKY_AMBIENT, (1.0, 0.0, 0.0))(p, n)
    top = want.max(0)  # relative to each channel's largest value: the term itself passes through 0 at N = up
    assert np.abs(E / np.pi - want).max() <= 1e-12 * top.min() and np.abs(W - 1).max() < 1e-12
    assert (E / np.pi).min() >= -1e-12  # the clamp is inactive up to rounding
    # and through the ambient function the renderer's restatement uses
    assert np.abs(mv.volume_ambient_fn(sh, res, lo, hi)(p, n) - want).max() <= 1e-12 * top.max()
    # the scale the GPU test's 256 ULP refer to bounds the absolute evaluation everywhere
    scale, _ = sh_ref.lookup(sh, res, lo, hi, p, n, absolute=True)
    assert scale.max() <= mv.sky_scale()


def test_varying_volume_layout():
    sh, res, lo, hi = mv.varying_volume()
    box_lo, box_hi = ref.scene_box(mc.normalised(mc.render_scene()))
    assert res == (4, 3, 3) and sh.dtype == np.float32 and sh.shape == (36, 28)
    assert np.allclose(lo, box_lo - 0.25) and np.allclose(hi, box_hi + 0.25)
    dead = np.nonzero(sh[:, 27] == 0)[0]
    assert 1 <= dead.size <= 2 and np.abs(sh[:, :27]).max() < 10
    # the dead probes sit next to visible surface: within a cell of a covered pixel's hit point
    fr = mv.varying_frame()
    P = sh_ref.volume_points(res, lo, hi)[dead]
    cell = (np.float64(hi) - np.float64(lo)) / (np.asarray(res) - 1)
    hits = fr["pos"][fr["covered"]]
    for q in P:
        assert (np.abs(hits - q) < cell).all(1).any(), q


def test_varying_frame_reaches_its_branches_on_safe_pixels():
    for metallic in (0.0, 1.0):
        fr = mv.varying_frame(metallic)
        base = mc.reference_frame("defaults")
        assert np.array_equal(fr["covered"], base["covered"]) and np.array_equal(fr["depth"], base["depth"]) and np.array_equal(fr["lit"], base["lit"])
        share = fr["unsafe_volume"].mean()
        safe = ~fr["unsafe_volume"] & fr["covered"]
        partial = (safe & (fr["W"] < 0.999)).sum()
        clamped = (safe & (fr["E"] < 0).any(-1)).sum()
        lit = (safe & fr["lit"]).sum()
        print("\nmetallic %g: unsafe %.2f %% (the frame's own %.2f %%), safe covered %d, W < 0.999 on %d, a channel clamped on %d, lit %d, W in [%.3f, %.3f]"
              % (metallic, 100 * share, 100 * fr["unsafe"].mean(), safe.sum(), partial, clamped, lit, fr["W"][safe].min(), fr["W"][safe].max()))
        assert share <= mc.UNSAFE_CAP, share
        assert partial > 30 and clamped > 30 and lit > 100, (partial, clamped, lit)
        assert (safe & (fr["E"] > 0).all(-1)).sum() > safe.sum() // 2  # most E > 0
        # the ambient light is visible in the colour: the frame is not the ambient-free one
        assert np.abs(fr["rgba"][..., :3][safe] - base["rgba"][..., :3][safe]).max() > 0.02


def test_position_term_does_not_loosen_the_bound():
    for metallic in (0.0, 1.0):
        fr = mv.varying_frame(metallic)
        safe = ~fr["unsafe_volume"] & fr["covered"]
        ratio = (fr["bound_dE"][safe] / fr["bound_first"][safe]).max()
        print("\nmetallic %g: k dE / pi is at most %.3f of the frame tolerance; the bound is at most %.2e" % (metallic, ratio, fr["bound"][safe].max()))
        assert ratio < 1.0
        assert fr["bound"][safe].max() < 1e-4  # (a colour tolerance, not a licence)
