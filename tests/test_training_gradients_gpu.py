"""The training step off the noise floor and at its batch caps (cases, budgets and bounds: tests/training_cases.py; the oracle's side alone:
tests/test_training_cases_cpu.py). The targets are images the model does not fit, so lgrad is of order one and every link behind it counts:
the loss kernel's chunk carries and early termination under all seven loss types, the fused backward level by level, the room clamp of the
compaction and the fit test of the sample generation, and six optimizer steps replayed entry by entry."""
import numpy as np
import pytest

import training_cases as TC

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


@pytest.fixture(scope="module")
def images():
    return TC.target_images()


@pytest.fixture(scope="module")
def unit_data(tmp_path_factory, images):
    return TC.write_dataset(tmp_path_factory.mktemp("grad_ds"), images)


@pytest.fixture(scope="module")
def big_data(tmp_path_factory, images):
    return TC.write_dataset(tmp_path_factory.mktemp("grad_ds4"), images, aabb_scale=4, radius=3.0)


def _views(native, data):
    ctx = TC.ctx_with_data(native, data)
    views = TC.oracle_views(ctx, data)
    ctx.close()
    return views


@pytest.fixture(scope="module")
def unit_views(native, unit_data):
    return _views(native, unit_data)


@pytest.fixture(scope="module")
def unit_ref(native, oracle, scene_unit, unit_views):
    """One march and one network evaluation of the oracle for every test of the unit case's first step; left unchanged (its arrays are read-only)."""
    ref = TC.Reference(oracle, scene_unit, unit_views)
    yield ref
    ref.release()


def _params64(scene):
    return np.asarray(scene["params"], np.uint16).view(np.float16).astype(np.float64)


def _prepare(ctx, target, pad=0):
    """train_prepare_batch into host arrays `pad` rows longer than the target, filled with sentinels: the call may write `target` rows."""
    native = TC.pkg("native")
    n_rays = ctx.training_state()["rays_per_batch"]
    b = {"counters": np.zeros(3, np.uint32), "ray_indices": np.zeros(n_rays, np.uint32), "numsteps": np.zeros((n_rays, 2), np.uint32),
         "coords": np.full((target + pad, 7), SENTINEL, np.float32), "dloss": np.full((target + pad, 4), SENTINEL, np.float16), "loss": np.zeros(n_rays, np.float32), "n_rays": n_rays}
    p = native._p
    ctx._check(ctx.L.ngp_train_prepare_batch(ctx.h, target, p(b["counters"]), p(b["ray_indices"]), p(b["numsteps"]), p(b["coords"]), p(b["dloss"]), p(b["loss"])))
    return b


def _compare_full_batch(b, ref, opts, label, coord_tol=2e-6, count_tol=2e-4, allow_shifted=False, min_long=300):
    """kept rays -> counts -> coords -> loss -> dloss, the rollover factor included"""
    ls = ref.loss(opts)
    assert b["n_rays"] == ref.n_rays
    TC.check_kept_rays_and_counts(b, ref, ls, TC.TARGET, count_tol)
    stats = TC.compare_batch(b, ref, ls, target=TC.TARGET, coord_tol=coord_tol, relative_l2=(opts or {}).get("loss_type") == 6, allow_shifted=allow_shifted)
    assert stats["worst_coord"] <= coord_tol and stats["shifted"] <= 0.005 * stats["n_kept"] and stats["unknown"] <= 0.005 * stats["n_kept"], (label, stats)
    for g in TC.GROUPS:
        assert stats[g]["rays"] >= (500 if g != "long" else min_long), (label, g, stats[g]["rays"])  # the path is populated on the device's side too
    TC.assert_loss_within_bounds(stats, label)
    return ls


@pytest.mark.parametrize("loss_type", range(7), ids=TC.LOSS_NAMES)
def test_loss_kernel_matches_the_oracle_off_the_noise_floor(native, unit_data, unit_ref, scene_unit, loss_type):
    ctx = TC.ctx_with_data(native, unit_data)
    ctx.set_model(scene_unit)
    ctx.set_training_opts(loss_type=loss_type)
    b = ctx.train_prepare_batch(TC.TARGET)
    ctx.close()
    _compare_full_batch(b, unit_ref, {"loss_type": loss_type}, f"unit/{TC.LOSS_NAMES[loss_type]}")


def test_loss_kernel_with_a_fixed_background_and_linear_colors(native, unit_data, unit_ref, scene_unit):
    ctx = TC.ctx_with_data(native, unit_data)
    ctx.set_model(scene_unit)
    ctx.set_training_opts(**TC.FIXED_BG_OPTS)
    b = ctx.train_prepare_batch(TC.TARGET)
    ctx.close()
    _compare_full_batch(b, unit_ref, TC.FIXED_BG_OPTS, "unit/fixed_bg")


def test_loss_kernel_with_cascades(native, oracle, big_data, scene_big):
    """varying dt (cone angle 1 / 256) through unwarp_dt in both passes; tolerances of the march as in test_sample_generation_and_loss_with_cascades.
    The march's positions differ from the oracle's by ulps here (device exp / log against libm), so the oracle's network and loss run on the
    device's own coordinates: what is left is the loss kernel."""
    ctx = TC.ctx_with_data(native, big_data)
    views = TC.oracle_views(ctx, big_data)
    ctx.set_model(scene_big)
    b = ctx.train_prepare_batch(TC.TARGET)
    ctx.close()
    ref = TC.Reference(oracle, scene_big, views)
    try:
        _compare_full_batch(b, ref.at_device_coords(b, 2e-5), None, "big/Huber", coord_tol=2e-5, count_tol=5e-3, allow_shifted=True, min_long=1)
    finally:
        ref.release()


def test_backward_matches_the_oracle_level_by_level(native, unit_data, scene_unit):
    """The fused backward on a batch whose dloss is a loss gradient, not regularisers and noise: every matrix layer and every grid level on its own."""
    ctx = TC.ctx_with_data(native, unit_data)
    ctx.set_model(scene_unit)
    b = ctx.train_prepare_batch(TC.TARGET)
    n = int(b["counters"][2])
    g = ctx.train_gradients(TC.TARGET)
    ctx.close()
    assert np.abs(b["dloss"][:n].astype(np.float32)).max() > 1e-3
    TC.check_backward(g, _params64(scene_unit), scene_unit["encoding"], b["coords"][:n], b["dloss"][:n], label="unit/Huber backward")


@pytest.mark.parametrize("target", [TC.CAP_COMPACTION, TC.CAP_GENERATION], ids=["compaction_overflows", "generation_overflows"])
def test_batch_caps(native, unit_data, unit_ref, scene_unit, target):
    """The first step's 4096 rays against a target they overflow: room / min(room, ...) in the loss kernel, `fits` in the sample generation,
    the n == target early-out of the rollover. Which rays lose the race for room is the atomics' business; every ray that got room is
    compared with the oracle's uncapped ray of the same index."""
    pad = 64
    ctx = TC.ctx_with_data(native, unit_data)
    ctx.set_model(scene_unit)
    b = _prepare(ctx, target, pad)
    g = ctx.train_gradients(target)
    ctx.train_apply()
    st = ctx.training_state()
    ctx.close()
    ls = unit_ref.loss()
    c = b["counters"].astype(np.int64)
    assert c[2] > target
    if target == TC.CAP_GENERATION:
        assert c[0] > 16 * target and c[1] < unit_ref.kept.size
    else:
        assert c[0] == unit_ref.total and c[1] == unit_ref.kept.size
    # nothing at or beyond the target is written
    assert (b["coords"][target:] == SENTINEL).all() and (b["dloss"][target:] == np.float16(SENTINEL)).all()
    assert np.isfinite(b["coords"][:target]).all() and np.isfinite(b["dloss"][:target].astype(np.float32)).all()
    assert not (b["coords"][:target] == SENTINEL).any()
    # the rays with samples tile [0, target): disjoint intervals, no hole
    n_kept = int(c[1])
    kept = b["ray_indices"][:n_kept]
    assert len(set(kept.tolist())) == n_kept and set(kept.tolist()) <= set(unit_ref.kept.tolist())
    cn, cb = b["numsteps"][:n_kept, 0].astype(np.int64), b["numsteps"][:n_kept, 1].astype(np.int64)
    has = cn > 0
    order = np.argsort(cb[has])
    starts, ends = cb[has][order], (cb[has] + cn[has])[order]
    assert starts[0] == 0 and ends[-1] == target and np.array_equal(starts[1:], ends[:-1])
    # no ray is longer than the oracle's; at most one is shorter for lack of room, the rest of the shorter ones are the T < 1e-4 noise of a full batch
    on = ls["compacted_numsteps"][kept].astype(np.int64)
    assert (cn <= unit_ref.gen["numsteps"][kept]).all()
    stats = TC.compare_batch(b, unit_ref, ls, target=target)
    print(f"[cap {target}] counters {c.tolist()} rays with room {int(has.sum())} without {stats['no_room']} clamped {stats['clamped']}")
    assert stats["clamped"] <= 1 and stats["no_room"] == int((~has).sum()) and stats["no_room"] > 0 and stats["unknown"] == 0
    assert stats["worst_coord"] <= 2e-6
    noise = int(np.sum(has & (cn != on))) - stats["clamped"]
    assert noise <= np.ceil(TC.bound("unequal_share") * has.sum()), (noise, int(has.sum()))
    # prefix coords, loss and dloss within the bounds of the full batch ("long" and "cut" have too few rays here to carry a percentile)
    print(f"[cap {target}] {TC.describe(stats)}")
    for q in ("loss_sum", "loss_ray", "dloss_sum", "dloss_p999"):
        assert stats["all"][q] <= TC.bound(q), (q, stats["all"][q])
    # the backward pass sees exactly those target rows
    TC.check_backward(g, _params64(scene_unit), scene_unit["encoding"], b["coords"][:target], b["dloss"][:target], label=f"cap {target} backward", full_batch=False)
    # NerfCounters::update_after_training
    assert st["training_step"] == 1 and st["measured_batch_size"] == c[2] and st["measured_batch_size_before_compaction"] == c[0]
    assert st["rays_per_batch"] == TC.next_multiple(TC.N_RAYS_FIRST_STEP * target // int(c[2]), 128)
    want_loss = float(b["loss"].astype(np.float64).sum()) * int(c[2]) / target
    assert abs(st["loss"] - want_loss) <= 1e-5 * want_loss, (st["loss"], want_loss)


def _step(ctx, target=TC.TARGET):
    b = ctx.train_prepare_batch(target)
    g = ctx.train_gradients(target)
    lr = ctx.training_state()["learning_rate"]
    ctx.train_apply()
    return b, g, lr


@pytest.mark.parametrize("decay", [False, True], ids=["constant_rate", "decayed_rate"])
def test_six_optimizer_steps_replayed(native, unit_data, scene_unit, decay):
    """Adam with per-entry step counts (grid entries are touched in some steps and not in others), ExponentialDecay and Ema, replayed in
    float64 from the device's own gradients with m1, m2 and the counts carried over."""
    import train_oracle as T

    ctx = TC.ctx_with_data(native, unit_data)
    ctx.set_model(scene_unit)
    if decay:
        ctx.set_training_opts(decay_start=3, decay_interval=2, decay_base=0.5)
    w_prev, ema0 = ctx.training_params()
    assert np.array_equal(w_prev, ema0)
    m1, m2, steps = np.zeros(w_prev.size), np.zeros(w_prev.size), np.zeros(w_prev.size, np.int64)
    ema = w_prev.astype(np.float64)
    rates = []
    for k in range(1, 7):
        _, g, lr = _step(ctx)
        rates.append(lr)
        w_now, ema_now = ctx.training_params()
        w = w_prev.astype(np.float64)
        upd = T.adam_step(w, g.astype(np.float64), m1, m2, steps, TC.N_MATRIX, lr=lr)
        assert np.allclose(w_now, w, rtol=1e-5, atol=1e-7), (k, float(np.abs(w_now - w).max()))
        assert np.array_equal(w_now[~upd], w_prev[~upd]), k  # entries no sample touched stay bit-equal
        assert (~upd).sum() > 1000 and upd[TC.N_MATRIX:].sum() > 1000
        T.ema_step(ema, w_now.astype(np.float16).astype(np.float64), k)
        assert np.allclose(ema_now, ema, rtol=1e-5, atol=1e-7), (k, float(np.abs(ema_now - ema).max()))
        assert ctx.training_state()["training_step"] == k
        w_prev = w_now
    ctx.close()
    assert np.allclose(rates, [0.01, 0.01, 0.01, 0.005, 0.005, 0.0025] if decay else [0.01] * 6, rtol=1e-6)
    counts = np.bincount(steps[TC.N_MATRIX:], minlength=7)
    print(f"grid entries by number of steps that touched them: {counts.tolist()}")
    assert (counts[:7] >= 100).all() and counts.size == 7, counts  # every per-entry count from 0 to 6 is exercised
    assert (steps[:TC.N_MATRIX] == 6).all()
    assert np.abs(w_prev[:TC.N_MATRIX] - _params64(scene_unit)[:TC.N_MATRIX]).mean() > 0.005  # the weights have moved by the order of lr per step


@pytest.mark.parametrize("k", [2, 4])
def test_the_step_after_k_optimizer_steps_uses_the_new_weights(native, oracle, unit_data, unit_views, scene_unit, k):
    """After k steps every weight has moved by about k * 0.01: the loss kernel and the backward of step k are compared with an oracle model
    rebuilt from fp16(w_k), under train_rng(1337, k) and the state's rays_per_batch. Fragments or a grid left at an earlier step's weights
    fail by far more than the bounds. Such a step's batch may fill the target, and its march is capped by the previous step's sample count
    (train_nerf_step's max_inference), so the room clamp and the fit test run here as well."""
    ctx = TC.ctx_with_data(native, unit_data)
    ctx.set_model(scene_unit)
    for _ in range(k):
        _step(ctx)
    w, _ = ctx.training_params()
    st = ctx.training_state()
    assert st["training_step"] == k and st["rays_per_batch"] != TC.N_RAYS_FIRST_STEP
    b = ctx.train_prepare_batch(TC.TARGET)
    g = ctx.train_gradients(TC.TARGET)
    ctx.close()
    sc = TC.scene_with_params(scene_unit, w)
    ref = TC.Reference(oracle, sc, unit_views, n_rays=st["rays_per_batch"], step=k)
    try:
        ls = ref.loss()
        c = b["counters"].astype(np.int64)
        n_kept = int(c[1])
        # (sample generation is capped by the previous step's count, train_nerf_step's max_inference: rays may be missing, none may be new)
        kept = b["ray_indices"][:n_kept]
        assert b["n_rays"] == ref.n_rays and len(set(kept.tolist())) == n_kept and set(kept.tolist()) <= set(ref.kept.tolist()) and abs(c[0] - ref.total) <= 2e-4 * ref.total
        assert abs(c[2] - int(ls["compacted_numsteps"][kept].sum())) <= 2e-3 * c[2]
        print(f"[step {k}] rays {ref.n_rays} kept {n_kept} of {ref.kept.size} counters {c.tolist()}")
        stats = TC.compare_batch(b, ref, ls, target=TC.TARGET)
        assert stats["worst_coord"] <= 2e-6 and stats["unknown"] == 0 and stats["clamped"] <= 1
        if c[2] < TC.TARGET:
            assert stats["no_room"] == 0
        TC.assert_loss_within_bounds(stats, f"step {k}/Huber")
        n = int(min(c[2], TC.TARGET))
        TC.check_backward(g, _params64(sc), sc["encoding"], b["coords"][:n], b["dloss"][:n], label=f"step {k} backward")
    finally:
        ref.release()


def test_inference_model_follows_the_ema_weights(native, oracle, unit_data, scene_unit):
    """sync_inference_model after optimizer steps: the render model's xor-layout table (train_xor_layout_kernel) and inference fragments are
    rebuilt from fp16 of Ema's weights. The encoded features equal the oracle's on those weights as values, as in test_grid_encode, positions
    outside the xor layout's range included; the network outputs are held to test_network_outputs' bounds."""
    ctx = TC.ctx_with_data(native, unit_data)
    ctx.set_model(scene_unit)
    rng = np.random.default_rng(21)
    n = 4096 + 37
    pos = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    pos[:4] = [[0, 0, 0], [1, 1, 1], [1.5, 0.2, 0.3], [-0.25, 0.5, 0.5]]
    d = rng.normal(size=(n, 3)).astype(np.float32)
    dir01 = ((d / np.linalg.norm(d, axis=1, keepdims=True) + 1) * 0.5).astype(np.float32)
    before = ctx.grid_encode(pos).astype(np.float32)
    for k in range(1, 4):
        _step(ctx)
        _, ema = ctx.training_params()
        m = oracle.make_model(TC.scene_with_params(scene_unit, ema))
        try:
            got, ref = ctx.grid_encode(pos).astype(np.float32), oracle.grid_encode(m, pos).astype(np.float32)
            bad = got != ref
            assert not bad.any(), (k, int(bad.sum()), float(np.abs(got - ref).max()))
            out, want = ctx.network(pos, dir01).astype(np.float32), oracle.network(m, pos, dir01).astype(np.float32)
        finally:
            oracle.release(m)
        assert np.mean(got != before) > 0.5, k  # the table has moved: a stale one differs in most features
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -14))) - 10)  # fp16 spacing at |want|
        err = np.abs(out - want)
        assert np.isfinite(out).all() and err.max() <= 3e-2 and (err == 0).mean() > 0.5 and (err <= ulp).mean() > 0.90, (k, float(err.max()), float((err == 0).mean()))
        before = got
    ctx.close()
