"""The training cases (tests/training_cases.py) are what they claim, shown by the oracle alone before any device result is looked at:
the target images have their regions, the unit case populates every chunk-carry and termination path of the loss kernel away from the
noise floor, the cap cases overflow what they say, and the budgets behind the GPU tests' bounds cover the reference against itself."""
import numpy as np
import pytest

import training_cases as TC


@pytest.fixture(scope="module")
def images():
    return TC.target_images()


@pytest.fixture(scope="module")
def unit_ref(oracle, scene_unit, images):
    ref = TC.Reference(oracle, scene_unit, TC.cpu_views(images), accumulate=("exact", "fp16_k16"))
    yield ref
    ref.release()


def test_target_images_have_their_regions(images):
    assert len(images) == len(TC.POSES)
    for im in images:
        a, rgb = im[..., 3], im[..., :3]
        assert im.dtype == np.float32 and im.shape == (TC.H, TC.W, 4)
        ramp = (a > 0) & (a < 1)
        assert (a == 0).sum() > 1000 and (a == 1).sum() > 1000 and ramp.sum() > 1000 and a.min() == 0.0 and a.max() == 1.0
        assert np.unique(a[ramp]).size > 100  # a smooth ramp, not a step
        assert not rgb[a == 0].any()  # premultiplied
        assert 3 <= (rgb.max(-1) > 1.0).sum() <= 8 and rgb.min() >= 0.0
    straight = np.concatenate([im[..., :3][im[..., 3] == 1] for im in images])
    assert (straight.min(0) < 0.1).all() and (np.quantile(straight, 0.95, axis=0) > 0.85).all()  # every channel sweeps its range
    assert not np.array_equal(images[0], images[1])


def test_unit_case_populates_every_path_of_the_loss_kernel(unit_ref):
    ls = unit_ref.loss()
    n = TC.path_counts(unit_ref, ls)
    print(n)
    assert n["over_64"] >= 500 and n["over_128"] >= 100 and n["cut"] >= 500 and n["cut_after_64"] >= 100
    # off the noise floor: the L1 loss is the channel mean of |prediction - target| over n_rays, so a sum of the three above 0.06 puts at
    # least one channel above 0.02 (L1's and Huber's kinks are at 0), a sum above 0.3 one channel above Huber's |diff| = 0.1 (linear branch),
    # and a sum below 0.1 every channel below it (quadratic branch)
    l1 = unit_ref.loss({"loss_type": 1})["loss"][unit_ref.kept].astype(np.float64) * 3 * unit_ref.n_rays
    assert np.mean(l1 > 0.06) >= 0.95
    assert (l1 > 0.3).sum() >= 100
    assert 0.3 < np.median(l1) < 3.0  # colours differ from the model's by order 0.1 - 1 per channel
    # Huber's two branches, per channel: dL/d(rgb logit) is lgrad * weight * rgb', and lgrad is +-1 for L1, +-0.2 on Huber's linear branch,
    # 2 |diff| (< 0.2) on its quadratic one; the ratio of the two gradients at the ray's heaviest sample tells the branch
    dh, d1 = np.abs(ls["dloss"].astype(np.float64)), np.abs(unit_ref.loss({"loss_type": 1})["dloss"].astype(np.float64))
    ratios = []
    for i in unit_ref.kept:
        b, c = int(unit_ref.gen["base"][i]), int(ls["compacted_numsteps"][i])
        for ch in range(3):
            j = b + int(np.argmax(d1[b:b + c, ch]))
            if d1[j, ch] > 1e-3:
                ratios.append(dh[j, ch] / d1[j, ch])
    ratios = np.array(ratios)
    assert (ratios < 0.15).sum() >= 100 and (ratios > 0.195).sum() >= 1000, ((ratios < 0.15).sum(), (ratios > 0.195).sum())
    # the sample positions do not depend on the loss options: one march serves every loss type
    for lt in range(7):
        assert np.array_equal(unit_ref.loss({"loss_type": lt})["compacted_numsteps"], ls["compacted_numsteps"])
    # every loss type hands the network a finite gradient well inside fp16's normal range (dloss carries loss_scale / n_rays = 1 / 32, a
    # sample's weight and the logistic's slope: 1e-3 is a sample that owns a tenth of its ray under Huber's +-0.2)
    for lt in range(7):
        d = np.abs(unit_ref.loss({"loss_type": lt})["dloss"].astype(np.float32))
        assert d.max() > 1e-3 and (d > 6.2e-5).sum() > 10000 and np.isfinite(d).all(), (lt, d.max(), (d > 6.2e-5).sum())


def test_cap_cases_overflow_what_they_say(unit_ref):
    n = TC.path_counts(unit_ref, unit_ref.loss())
    assert n["marched"] > 16 * TC.CAP_GENERATION and n["compacted"] > TC.CAP_GENERATION  # 1 << 12: sample generation and compaction both
    assert n["marched"] <= 16 * TC.CAP_COMPACTION and n["compacted"] > TC.CAP_COMPACTION  # 1 << 14: compaction only
    assert n["marched"] <= 16 * TC.TARGET and n["compacted"] < TC.TARGET  # the full target: neither


def _measure(ref, opts, relative_l2=False):
    a, b = ref.loss(opts), ref.loss(opts, accumulate="fp16_k16")
    return TC.compare_batch(ref.as_batch(b), ref, a, relative_l2=relative_l2)


def test_budgets_cover_the_reference_against_itself(oracle, scene_big, images, unit_ref):
    """The oracle's loss on its "exact" network outputs against the same on its "fp16_k16" outputs, for every case of
    tests/test_training_gradients_gpu.py: each figure stays inside its budget, and each budget is within a third of its worst figure (a budget
    may not be padded)."""
    d = np.abs(unit_ref.nets["exact"].astype(np.float32) - unit_ref.nets["fp16_k16"].astype(np.float32))
    print(f"network outputs, exact against fp16_k16: max {d.max():.4f} mean {d.mean():.5f}")
    assert d.max() > 0.01  # the bracket is wider than what test_network_outputs allows the device
    big = TC.Reference(oracle, scene_big, TC.cpu_views(images, radius=3.0), accumulate=("exact", "fp16_k16"))
    nb = TC.path_counts(big, big.loss())
    assert nb["over_64"] >= 500 and nb["cut"] >= 500
    cases = [(f"unit/{TC.LOSS_NAMES[lt]}", _measure(unit_ref, {"loss_type": lt}, relative_l2=(lt == 6))) for lt in range(7)]
    cases.append(("unit/fixed_bg", _measure(unit_ref, TC.FIXED_BG_OPTS)))
    cases.append(("big/Huber", _measure(big, None)))
    big.release()
    worst = {}
    for label, st in cases:
        print(f"[{label}] {TC.describe(st)}")
        assert st["worst_coord"] == 0.0 and st["unknown"] == 0
        assert st["unequal_share"] <= TC.BUDGET["unequal_share"], label
        worst["unequal_share"] = max(worst.get("unequal_share", 0.0), st["unequal_share"])
        for g in TC.GROUPS:
            for q in ("dloss_sum", "dloss_p999", "loss_sum", st["ray_key"]):
                assert st[g][q] <= TC.BUDGET[q][g], (label, g, q, st[g][q])
                worst[(q, g)] = max(worst.get((q, g), 0.0), st[g][q])
    for key, w in worst.items():
        budget = TC.BUDGET[key] if isinstance(key, str) else TC.BUDGET[key[0]][key[1]]
        assert w >= budget / 1.5, (key, w, budget)


def test_fp16_mode_of_the_backward_oracle(unit_ref, scene_unit):
    """train_oracle's fp16 mode against its float64 mode on the unit case's batch: the mode only rounds (same signs, same touched entries), and
    its distance per grid level is the budget of the device's per-level bound."""
    import train_oracle as T

    ls = unit_ref.loss()
    rows = unit_ref.compacted_rows(ls)
    assert rows.size == int(ls["compacted_numsteps"].sum())
    enc = scene_unit["encoding"]
    params = np.asarray(scene_unit["params"], np.uint16).view(np.float16).astype(np.float64)
    # the batch as the backward pass sees it: short of the target, so the rollover has scaled the first samples' gradients
    dloss = TC.rollover_factor(ls["dloss"][rows].astype(np.float32), 0, rows.size, rows.size, TC.TARGET).astype(np.float16).astype(np.float64)
    coords = unit_ref.gen["coords"][rows].astype(np.float64)
    (out64, k64), (out16, k16) = T.forward(params, enc, coords[:4096], keep=True), T.forward(params, enc, coords[:4096], keep=True, fp16=True)
    # the mode's encoded features are the C oracle's (tcnn's half corner sum, which the device matches bit for bit) up to a last bit here and there
    x_c = unit_ref.oracle.grid_encode(unit_ref.m, coords[:4096, :3].astype(np.float32)).astype(np.float64)
    assert np.mean(x_c != k16["x"]) < 2e-3 and np.abs(x_c - k16["x"]).max() < 1e-3 and np.abs(x_c - k64["x"]).max() > np.abs(x_c - k16["x"]).max()
    assert 0 < np.abs(out16 - out64).max() < 0.02  # fp16 storage of activations of order 1: a few 2^-11 through three layers
    g64, g16 = T.backward(params, enc, coords, dloss), T.backward(params, enc, coords, dloss, fp16=True)
    assert np.array_equal(T.backward(params, enc, coords[:512], dloss[:512], fp16=False), T.backward(params, enc, coords[:512], dloss[:512]))
    assert len(TC.GRID_LEVEL_BUDGET) == enc["n_levels"]
    rels = TC.grid_level_errors(g16, g64, enc)
    print("grid levels, fp16 mode against float64: " + " ".join(f"{r:.2e}" for r in rels))
    for l, r in enumerate(rels):
        assert TC.GRID_LEVEL_BUDGET[l] / 1.5 <= r <= TC.GRID_LEVEL_BUDGET[l], (l, r)
    for lo, hi in TC.MATRIX_LAYERS:
        assert np.linalg.norm(g16[lo:hi] - g64[lo:hi]) < 0.1 * TC.LAYER_REL * np.linalg.norm(g64[lo:hi])  # the matrices' bound is not about fp16 storage
    # every level is touched by the batch and keeps untouched entries: the exact-zero check means something on each
    offsets, _, _ = T.layout(enc)
    for l in range(enc["n_levels"]):
        lo, hi = TC.N_MATRIX + offsets[l] * 4, TC.N_MATRIX + offsets[l + 1] * 4
        assert g64[lo:hi].any(), l
    assert (g64[TC.N_MATRIX:] == 0).mean() > 0.05
    assert not np.any((g16[TC.N_MATRIX:] != 0) & (g64[TC.N_MATRIX:] == 0))
