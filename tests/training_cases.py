"""What the training tests share (tests/test_training_gpu.py, tests/test_training_gradients_gpu.py, tests/test_training_cases_cpu.py):
the dataset's shape, target images the model does NOT already fit, the oracle's side of one training batch, the ray-by-ray comparison of a
batch with that oracle, and the budgets and bounds of that comparison.

Where the bounds come from. The loss kernel is compared on the oracle's own network outputs, and the device's outputs differ from those by
its MLP summation (fp32 MFMA accumulators). The oracle has two summation modes that bracket the device's (BASELINE.md section 4,
tests/test_parity_gpu.py::test_mlp_accumulation_bracket): "exact" and "fp16_k16". BUDGET holds the distance between the oracle's loss on
those two sets of outputs, measured on these very images by tests/test_training_cases_cpu.py, which fails if a measurement leaves its
budget. Every bound is twice its budget: the factor leaves room for the scan order and fast_exp of the device's loss kernel. No figure here
was taken from a device run."""
import os
import sys

import numpy as np

from conftest import pkg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

W = H = 96
FOV = 0.6911
POSES = [(0, 30), (45, 20), (90, 40), (135, 10), (180, 30), (225, 50), (270, 25), (315, 35)]
TARGET = 1 << 17
N_RAYS_FIRST_STEP = 4096  # NerfCounters' initial rays_per_batch, whatever the batch size
CAP_COMPACTION, CAP_GENERATION = 1 << 14, 1 << 12  # target batches the first step overflows: after compaction only / already while marching
SEED = 1337
N_MATRIX = 10240
LOSS_NAMES = ("L2", "L1", "Mape", "Smape", "Huber", "LogL1", "RelativeL2")
HUBER = 4
FIXED_BG_OPTS = dict(loss_type=0, random_bg_color=0, background_color=(0.2, 0.4, 0.6), linear_colors=1)
GROUPS = ("all", "long", "cut")  # every compared ray / rays of more than 64 compacted samples (chunk carries) / rays cut early by T < 1e-4

# ---- budgets: the oracle's loss on "exact" against "fp16_k16" network outputs, worst over the cases named beside each
# (test_training_cases_cpu.py::test_budgets_cover_the_reference_against_itself measures them again and compares).
#   unit    : the unit scene, default options, worst of the seven loss types
#   fixed_bg: the unit scene, FIXED_BG_OPTS
#   big     : scene_big (three cascades), Huber
BUDGET = {
    # sum |d dloss| / sum |dloss| over the compared samples (worst: LogL1; L2 and Huber measure 2.4e-3)
    "dloss_sum": {"all": 6.4e-3, "long": 7.3e-3, "cut": 3.8e-3},
    # 99.9th percentile of |d dloss| over max |dloss| of the group (worst: big, whose "long" group is 6 rays; unit: 1.3e-3 / 1.6e-3 / 1.2e-3)
    "dloss_p999": {"all": 1.7e-3, "long": 3.6e-3, "cut": 1.9e-3},
    # sum |d loss| / sum loss over the rays (worst: Mape)
    "loss_sum": {"all": 7.4e-4, "long": 5.6e-4, "cut": 7.7e-4},
    # worst ray: |d loss| / max(loss, LOSS_FLOOR_SHARE * median loss); RelativeL2 apart, as its normaliser is the prediction squared
    "loss_ray": {"all": 8.8e-3, "long": 3.0e-3, "cut": 8.8e-3},
    "loss_ray_relative_l2": {"all": 7.5e-3, "long": 5.2e-3, "cut": 7.5e-3},
    # share of kept rays whose compacted count differs (T crosses 1e-4 one sample earlier or later): 19 of 1779 rays
    "unequal_share": 1.1e-2,
}
BOUND_FACTOR = 2.0
# A ray whose target happens to coincide with the prediction has a loss near zero, and a relative figure there measures the coincidence,
# not the kernel: rays below this share of the median loss are held to the absolute error of a ray at that share.
LOSS_FLOOR_SHARE = 0.05

# ---- backward: per grid level, |g_fp16 - g_64| / |g_64| of train_oracle.backward's fp16 mode (halves where the device stores halves, sums in
# float64) against its float64 mode, on the unit case's Huber batch (test_training_cases_cpu.py::test_fp16_mode_of_the_backward_oracle).
# The device is held to twice this distance per level, measured on the very batch it ran (check_backward says why); the matrices keep the
# bounds of test_backward_matches_the_float64_oracle.
GRID_LEVEL_BUDGET = (2.3e-3, 3.5e-3, 6.8e-3, 6.0e-3, 7.0e-3, 9.2e-3, 8.4e-3, 7.5e-3)  # the fixtures' grids have 8 levels of 4 features
MATRIX_LAYERS = ((0, 2048), (2048, 3072), (3072, 5120), (5120, 9216), (9216, 10240))
LAYER_REL, LAYER_COS = 0.03, 0.9995


def bound(quantity, group="all"):
    b = BUDGET[quantity]
    return BOUND_FACTOR * (b[group] if isinstance(b, dict) else b)


def next_multiple(v, m):
    return (v + m - 1) // m * m


# --------------------------------------------------------------------------------------------------------- images and datasets
def target_images(n=len(POSES)):
    """Deterministic float RGBA views (linear, premultiplied) that no model of the fixtures fits: per view a half plane of alpha exactly 0,
    one of alpha exactly 1 and a linear ramp between, the edge turning with the view; straight colours that sweep 0.05..0.95 in every
    channel on waves of different periods; five opaque pixels beyond 1.0."""
    y, x = np.mgrid[0:H, 0:W]
    u, v = (x + 0.5) / W, (y + 0.5) / H
    out = []
    for i in range(n):
        th = 2.0 * np.pi * i / n + 0.3
        s = (u - 0.5) * np.cos(th) + (v - 0.5) * np.sin(th)
        alpha = np.clip(s / 0.5 + 0.5, 0.0, 1.0)
        rgb = np.stack([0.5 + 0.45 * np.sin(2.0 * np.pi * (fu * u + fv * v) + ph + 0.7 * i) for fu, fv, ph in ((1.5, 0.5, 0.0), (0.5, 2.0, 2.0), (2.5, 1.5, 4.0))], -1)
        hot = np.argwhere(alpha == 1.0)[:: max(1, int((alpha == 1.0).sum()) // 5)][:5]
        for k, (py, px) in enumerate(hot):
            rgb[py, px] = (1.2 + 0.2 * k, 1.05 + 0.1 * k, 2.0 - 0.1 * k)
        out.append(np.concatenate([rgb * alpha[..., None], alpha[..., None]], -1).astype(np.float32))
    return out


def camera_matrices(radius=4.03):
    S = pkg("scene")
    return [S.orbit_camera(az, el, radius=radius) for az, el in POSES]


def write_dataset(tmp_dir, images, aabb_scale=1, radius=4.03):
    """transforms.json for POSES in tmp_dir; the images are handed over with set_training_image (ctx_with_data)."""
    S = pkg("scene")
    mats = camera_matrices(radius)
    path = S.write_transforms(os.path.join(str(tmp_dir), "transforms.json"), mats, W, H, FOV, aabb_scale=aabb_scale)
    return {"path": path, "images": images, "mats": mats, "focal": S.focal_from_fov_x(W, FOV)}


def cpu_views(images, radius=4.03):
    """The oracle's views without a device: the cameras as written, not as the loader read them back (a last-bit difference at most)."""
    focal = tuple(pkg("scene").focal_from_fov_x(W, FOV))
    return [{"pixels": im, "xform": m, "focal": focal} for im, m in zip(images, camera_matrices(radius))]


def srgb_bytes(im):
    a = np.clip(im[..., 3:4], 1e-6, 1.0)
    rgb = np.clip(im[..., :3] / a, 0, 1)
    srgb = np.where(rgb <= 0.0031308, 12.92 * rgb, 1.055 * rgb ** (1 / 2.4) - 0.055)
    return (np.concatenate([srgb, im[..., 3:4]], -1) * 255 + 0.5).astype(np.uint8)


def ctx_with_data(native, dataset, byte_images=False):
    ctx = native.Context(0)
    ctx.load_training_data(dataset["path"])
    for i, im in enumerate(dataset["images"]):
        if byte_images:
            ctx.set_training_image(i, srgb_bytes(im))
        else:
            ctx.set_training_image(i, im)
    return ctx


def oracle_views(ctx, dataset):
    views = []
    for i, im in enumerate(dataset["images"]):
        v = ctx.training_view(i)
        views.append({"pixels": im, "xform": v["matrix"], "focal": tuple(v["focal_length"]), "principal": tuple(v["principal_point"])})
    return views


# --------------------------------------------------------------------------------------------------------- the oracle's side of a batch
def train_opts(oracle, scene, n_rays=N_RAYS_FIRST_STEP, step=0, opts=None):
    """The product's default training options (ngp_train.cpp default_opts) at training step `step`, with `opts` on top."""
    import oracle as O

    o = O.TrainOpts()
    o.n_rays, o.n_images, o.rng = n_rays, len(POSES), oracle.train_rng(SEED, step)
    o.snap_to_pixel_centers, o.random_bg_color, o.linear_colors, o.color_space, o.loss_type = 1, 1, 0, 1, HUBER
    o.near_distance, o.loss_scale, o.density_grid_mean = 0.1, 128.0, float(scene["density_grid_mean"])
    for k, v in (opts or {}).items():
        if k == "background_color":
            o.background = (O.C.c_float * 3)(*v)
        else:
            setattr(o, k, v)
    return o


def scene_with_params(scene, weights):
    """The scene with its parameters replaced by fp16(weights): what the training kernels read after an optimizer step."""
    sc = dict(scene)
    sc["params"] = np.ascontiguousarray(np.asarray(weights, np.float32).astype(np.float16)).view(np.uint16)
    return sc


class Reference:
    """Samples and network outputs of one batch from the oracle, marched without a cap; losses per option set on request."""

    def __init__(self, oracle, scene, views, n_rays=N_RAYS_FIRST_STEP, step=0, accumulate=("exact",)):
        self.oracle, self.scene, self.n_rays, self.step = oracle, scene, n_rays, step
        self.images = oracle.make_train_images(views)
        self.models = {a: oracle.make_model(dict(scene, mlp_accumulate=a)) for a in accumulate}
        self.m = self.models[accumulate[0]]
        gen = oracle.train_generate_samples(self.m, self.images, train_opts(oracle, scene, n_rays, step), TARGET * 16)
        self.total = int(gen["total"])
        assert self.total <= TARGET * 16
        gen["coords"] = np.ascontiguousarray(gen["coords"][: self.total])
        self.gen = gen
        self.kept = np.flatnonzero(gen["numsteps"])
        self.nets = {a: oracle.network(m, gen["coords"][:, :3], gen["coords"][:, 4:7]) for a, m in self.models.items()}
        self._loss = {}

    def loss(self, opts=None, accumulate=None):
        """The sample positions depend on none of the loss options (snap_to_pixel_centers stays as it is), so one march serves them all."""
        accumulate = accumulate or next(iter(self.models))
        key = (accumulate, tuple(sorted((opts or {}).items())))
        if key not in self._loss:
            o = train_opts(self.oracle, self.scene, self.n_rays, self.step, opts)
            ls = self.oracle.train_loss(self.models[accumulate], self.images, o, self.gen, self.nets[accumulate])
            for a in ls.values():
                a.setflags(write=False)
            self._loss[key] = ls
        return self._loss[key]

    def at_device_coords(self, b, coord_tol):
        """The same reference with the device's coordinates in place of its own wherever a ray's compacted prefix agrees within coord_tol
        (the rest of such a ray, behind T < 1e-4, stays the oracle's), and the networks evaluated again there. With cascades the device's
        exp / log move positions by ulps of the march, and the fixtures' networks turn an ulp of position into more than the whole budget
        of the loss kernel: on the device's own inputs the comparison is about the loss kernel alone. Shares the models: release once."""
        import copy

        new = copy.copy(self)
        gen = dict(self.gen)
        coords = self.gen["coords"].copy()
        for r in range(int(b["counters"][1])):
            i = int(b["ray_indices"][r])
            k, cb, ob = min(int(b["numsteps"][r, 0]), int(gen["numsteps"][i])), int(b["numsteps"][r, 1]), int(gen["base"][i])
            if k and float(np.abs(b["coords"][cb:cb + k] - coords[ob:ob + k]).max()) <= coord_tol:
                coords[ob:ob + k] = b["coords"][cb:cb + k]
        gen["coords"] = coords
        new.gen = gen
        new.nets = {a: self.oracle.network(m, coords[:, :3], coords[:, 4:7]) for a, m in self.models.items()}
        new._loss = {}
        return new

    def as_batch(self, ls):
        """An oracle result laid out like the device's batch (its samples stay where they were marched): for reference against reference."""
        kept, gen = self.kept, self.gen
        return {"counters": np.array([self.total, kept.size, int(ls["compacted_numsteps"].sum())], np.uint32), "ray_indices": kept.astype(np.uint32),
                "numsteps": np.stack([ls["compacted_numsteps"][kept], gen["base"][kept]], 1), "coords": gen["coords"], "dloss": ls["dloss"],
                "loss": ls["loss"][kept], "n_rays": self.n_rays}

    def compacted_rows(self, ls):
        """Row indices of every kept ray's compacted prefix, in ray order: the batch the backward pass sees."""
        return np.concatenate([np.arange(b, b + c) for b, c in zip(self.gen["base"], ls["compacted_numsteps"]) if c > 0])

    def release(self):
        for m in self.models.values():
            self.oracle.release(m)


def path_counts(ref, ls):
    """How many kept rays exercise each path of the loss kernel (the oracle alone)."""
    n, c = ref.gen["numsteps"][ref.kept].astype(np.int64), ls["compacted_numsteps"][ref.kept].astype(np.int64)
    cut = c < n
    return {"kept": int(ref.kept.size), "marched": ref.total, "compacted": int(c.sum()), "longest": int(n.max()), "over_64": int((n > 64).sum()), "over_128": int((n > 128).sum()),
            "cut": int(cut.sum()), "cut_after_64": int((cut & (c > 64)).sum())}


def rollover_factor(ref_d, cb, cn, n_compacted, target):
    """fill_rollover_and_rescale: the sample at compacted index c carries 1 + copies * n / target, each copy rounded to fp16 on its own."""
    copies = (target - 1 - np.arange(cb, cb + cn)) // n_compacted
    scale = n_compacted / target
    return ref_d + copies[:, None] * (ref_d * np.float32(scale)).astype(np.float16).astype(np.float32)


def compare_batch(b, ref, ls, target=None, coord_tol=2e-6, relative_l2=False, allow_shifted=False):
    """A batch (the device's, or Reference.as_batch) against the oracle ray by ray, by ray index. Returns the figures the bounds are about,
    for every group of GROUPS; asserts nothing but the order of the comparison's preconditions being meaningful.
    target: the device's target batch; None for an oracle layout. A batch short of it carries the rollover factor on dloss. A batch that
    overflows it is compared by prefix: a ray without room must report no loss ("no_room"), the ray that ends at the target may be shorter
    than the oracle's ("clamped"), every other ray is held to the oracle's count like in a full batch.
    allow_shifted: with cascades, libm against the device's exp / log can put a position on the other side of a cell wall; such a ray is
    counted in "shifted" and left out, as in check_batch_against_oracle."""
    gen = ref.gen
    n_kept = int(b["counters"][1])
    kept = b["ray_indices"][:n_kept]
    n_compacted = int(b["counters"][2])
    ref_kept = set(ref.kept.tolist())
    rows = []  # per ray: loss_got, loss_ref, long, cut, equal
    d_err, d_ref, d_long, d_cut = [], [], [], []
    worst_coord, unequal, unequal_uncut, unknown, shifted, no_room, clamped = 0.0, 0, 0, 0, 0, 0, 0
    for r in range(n_kept):
        i = int(kept[r])
        if i not in ref_kept:
            unknown += 1
            continue
        cn, cb = int(b["numsteps"][r, 0]), int(b["numsteps"][r, 1])
        ob, on = int(gen["base"][i]), int(ls["compacted_numsteps"][i])
        is_long, is_cut = on > 64, on < int(gen["numsteps"][i])
        capped = target is not None and n_compacted >= target
        if capped and cn == 0:  # lost the race for room: no sample, no loss
            assert float(b["loss"][r]) == 0.0, ("a ray without room reports a loss", i)
            no_room += 1
            continue
        ray_coord = float(np.abs(b["coords"][cb:cb + min(cn, on)] - gen["coords"][ob:ob + min(cn, on)]).max()) if min(cn, on) else 0.0
        if ray_coord > coord_tol and allow_shifted:
            shifted += 1  # a position on a cell wall taken on one side and not on the other: the rest of the ray is shifted by one
            continue
        worst_coord = max(worst_coord, ray_coord)
        rows.append((float(b["loss"][r]), float(ls["loss"][i]), is_long, is_cut, cn == on))
        if capped and cn < on and cb + cn == target:
            clamped += 1  # the ray that took the last room: its prefix, with dloss from the whole ray's rgb_ray
        elif cn != on:  # left out of the per-sample comparison (its loss is still compared): counted, and the count bounded
            unequal += 1
            unequal_uncut += not is_cut
            continue
        ref_d = ls["dloss"][ob:ob + cn].astype(np.float32)
        if target is not None and n_compacted < target:
            ref_d = rollover_factor(ref_d, cb, cn, n_compacted, target)
        d_err.append(np.abs(b["dloss"][cb:cb + cn].astype(np.float32) - ref_d).reshape(-1))
        d_ref.append(np.abs(ref_d).reshape(-1))
        d_long.append(np.full(cn * 4, is_long))
        d_cut.append(np.full(cn * 4, is_cut))
    rows = np.array(rows, np.float64).reshape(-1, 5)
    d_err, d_ref = np.concatenate(d_err), np.concatenate(d_ref)
    d_sel = {"all": np.ones(d_err.size, bool), "long": np.concatenate(d_long), "cut": np.concatenate(d_cut)}
    r_sel = {"all": np.ones(rows.shape[0], bool), "long": rows[:, 2] > 0, "cut": rows[:, 3] > 0}
    floor = LOSS_FLOOR_SHARE * float(np.median(rows[:, 1]))
    ray_key = "loss_ray_relative_l2" if relative_l2 else "loss_ray"
    out = {"n_kept": n_kept, "unknown": unknown, "unequal_share": unequal / max(n_kept - no_room, 1), "unequal_uncut_share": unequal_uncut / max(n_kept - no_room, 1), "worst_coord": worst_coord, "shifted": shifted, "no_room": no_room, "clamped": clamped,
           "ray_key": ray_key}
    for g in GROUPS:
        e, d, rr = d_err[d_sel[g]], d_ref[d_sel[g]], rows[r_sel[g]]
        lerr = np.abs(rr[:, 0] - rr[:, 1])
        if e.size == 0 or rr.shape[0] == 0:  # a group without rays (a batch cut short by a cap): nothing to report
            out[g] = {"rays": 0, "samples": 0, "dloss_sum": 0.0, "dloss_p999": 0.0, "loss_sum": 0.0, ray_key: 0.0}
            continue
        out[g] = {"rays": int(rr.shape[0]), "samples": int(e.size // 4), "dloss_sum": float(e.sum() / d.sum()), "dloss_p999": float(np.quantile(e, 0.999) / d.max()),
                  "loss_sum": float(lerr.sum() / rr[:, 1].sum()), ray_key: float((lerr / np.maximum(rr[:, 1], floor)).max())}
    return out


def describe(stats):
    return " | ".join(f"{g}: rays {s['rays']} samples {s['samples']} dloss_sum {s['dloss_sum']:.2e} dloss_p999 {s['dloss_p999']:.2e} loss_sum {s['loss_sum']:.2e} "
                      f"{stats['ray_key']} {s[stats['ray_key']]:.2e}" for g, s in ((g, stats[g]) for g in GROUPS)) + f" | unequal {stats['unequal_share']:.2e} (not cut by the oracle: {stats['unequal_uncut_share']:.2e}) shifted {stats['shifted']} coord {stats['worst_coord']:.1e}"


def assert_loss_within_bounds(stats, label):
    """loss, then dloss, group by group: the first failure names the path that broke."""
    print(f"[{label}] {describe(stats)}")
    assert stats["unequal_share"] <= bound("unequal_share"), (label, "rays left out of the per-sample comparison", stats["unequal_share"])
    for q in ("loss_sum", stats["ray_key"], "dloss_sum", "dloss_p999"):
        for g in GROUPS:
            assert stats[g][q] <= bound(q, g), (label, g, q, stats[g][q], bound(q, g))


def check_kept_rays_and_counts(b, ref, ls, target, count_tol=2e-4):
    """generate_training_samples_nerf: the same rays survive with the same number of steps; the compacted total agrees."""
    n_kept = int(b["counters"][1])
    kept = b["ray_indices"][:n_kept]
    assert len(set(kept.tolist())) == n_kept
    if count_tol <= 2e-4:
        assert set(kept.tolist()) == set(ref.kept.tolist())
    else:  # libm vs device exp / log in the stepping can move a ray's first or last step across a cell wall
        assert len(set(kept.tolist()) ^ set(ref.kept.tolist())) <= 0.005 * ref.kept.size
    assert abs(int(b["counters"][0]) - ref.total) <= count_tol * ref.total
    n_compacted = int(b["counters"][2])
    assert n_compacted < target and abs(n_compacted - int(ls["compacted_numsteps"].sum())) <= max(2e-3, 2 * count_tol) * n_compacted


def check_backward(g, params, enc, coords, dloss, label="", full_batch=True):
    """The fused backward against train_oracle.backward on the same coords and dloss: every matrix layer against float64 within the bounds of
    test_backward_matches_the_float64_oracle; every grid level against float64 within twice the distance of the oracle's own fp16 mode from
    float64 ON THIS BATCH (a level's error is a handful of ReLU masks that flip under the half roundings, and which samples carry the
    rollover factor moves it by a third from run to run: GRID_LEVEL_BUDGET is the figure of the oracle's batch, a full batch's budget may
    not leave it by more than a factor of four); and the device closer to the fp16 mode than the fp16 mode is to float64, level by level:
    the modelled roundings explain the device's distance from float64."""
    import train_oracle as T

    coords, dloss = np.asarray(coords, np.float64), np.asarray(dloss, np.float64)
    g = np.asarray(g, np.float64)
    ref_g, ref_16 = T.backward(params, enc, coords, dloss), T.backward(params, enc, coords, dloss, fp16=True)
    assert g.shape == ref_g.shape and np.isfinite(g).all()
    for name, (got, want) in {"matrices": (g[:N_MATRIX], ref_g[:N_MATRIX]), "grid": (g[N_MATRIX:], ref_g[N_MATRIX:])}.items():
        cos = float(got @ want / (np.linalg.norm(got) * np.linalg.norm(want)))
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        assert cos > LAYER_COS and rel < LAYER_REL, (label, name, cos, rel)
    for lo, hi in MATRIX_LAYERS:
        assert np.linalg.norm(g[lo:hi] - ref_g[lo:hi]) <= LAYER_REL * np.linalg.norm(ref_g[lo:hi]), (label, lo, hi)
    rels, budget, model = grid_level_errors(g, ref_g, enc), grid_level_errors(ref_16, ref_g, enc), grid_level_errors(g, ref_16, enc)
    for name, v in (("device vs float64", rels), ("fp16 mode vs float64", budget), ("device vs fp16 mode", model)):
        print(f"[{label}] grid levels, {name}: " + " ".join(f"{r:.2e}" for r in v))
    for l in range(enc["n_levels"]):
        assert rels[l] <= BOUND_FACTOR * budget[l], (label, "grid level", l, rels[l], BOUND_FACTOR * budget[l])
        assert model[l] <= budget[l], (label, "grid level against the fp16 mode", l, model[l], budget[l])
        if full_batch:
            assert budget[l] <= 4.0 * GRID_LEVEL_BUDGET[l], (label, "budget of grid level", l, budget[l])
    # untouched grid entries receive exactly nothing; touched ones may underflow to zero in the fp16 hand-over
    gz, rz = g[N_MATRIX:] != 0, ref_g[N_MATRIX:] != 0
    assert not np.any(gz & ~rz) and np.mean(gz != rz) < 0.01, label
    return rels


def grid_level_errors(g, ref_g, enc):
    import train_oracle as T

    offsets, _, _ = T.layout(enc)
    F = enc["n_features_per_level"]
    out = []
    for l in range(enc["n_levels"]):
        lo, hi = N_MATRIX + offsets[l] * F, N_MATRIX + offsets[l + 1] * F
        out.append(float(np.linalg.norm(g[lo:hi] - ref_g[lo:hi]) / np.linalg.norm(ref_g[lo:hi])))
    return out


# --------------------------------------------------------------------------------------------------------- the batch check of test_training_gpu.py
def check_batch_against_oracle(ctx, oracle, view_pixels, scene_unit, coord_tol=2e-6, same_frac=0.985, count_tol=2e-4, opts=None):
    import oracle as O

    dataset = {"images": view_pixels}
    ctx.set_model(scene_unit)
    if opts:
        ctx.set_training_opts(**opts)
    b = ctx.train_prepare_batch(TARGET)
    n_rays = b["n_rays"]
    assert n_rays == 4096
    m = oracle.make_model(scene_unit)
    images = oracle.make_train_images(oracle_views(ctx, dataset))
    o = O.TrainOpts()
    o.n_rays, o.n_images, o.rng = n_rays, len(POSES), oracle.train_rng(1337, 0)
    o.snap_to_pixel_centers, o.random_bg_color, o.linear_colors, o.color_space, o.loss_type = 1, 1, 0, 1, 4
    o.near_distance, o.loss_scale, o.density_grid_mean = 0.1, 128.0, float(scene_unit["density_grid_mean"])
    for k, v in (opts or {}).items():
        if k == "background_color":
            o.background = (O.C.c_float * 3)(*v)
        else:
            setattr(o, k, v)
    gen = oracle.train_generate_samples(m, images, o, TARGET * 16)
    # --- generate_training_samples_nerf: the same rays survive with the same number of steps
    n_kept = int(b["counters"][1])
    kept = b["ray_indices"][:n_kept]
    assert len(set(kept.tolist())) == n_kept
    ref_kept = set(np.flatnonzero(gen["numsteps"]).tolist())
    if count_tol <= 2e-4:
        assert set(kept.tolist()) == ref_kept
    else:  # libm vs device exp / log in the stepping can move a ray's first or last step across a cell wall
        assert len(set(kept.tolist()) ^ ref_kept) <= 0.005 * len(ref_kept)
    assert abs(int(b["counters"][0]) - int(gen["total"])) <= count_tol * gen["total"]
    # --- compute_loss_kernel_train_nerf on the oracle's own network output
    net = oracle.network(m, gen["coords"][: gen["total"], :3], gen["coords"][: gen["total"], 4:7])
    ls = oracle.train_loss(m, images, o, gen, net)
    n_compacted = int(b["counters"][2])
    assert n_compacted < TARGET and abs(n_compacted - int(ls["compacted_numsteps"].sum())) <= max(2e-3, 2 * count_tol) * n_compacted
    same, checked, worst_coord, dl_err, dl_ref, loss_got, loss_ref, shifted = 0, 0, 0.0, [], [], [], [], 0
    scale = n_compacted / TARGET
    for r in range(n_kept):
        i = int(kept[r])
        if i not in ref_kept:
            continue
        cn, cb = int(b["numsteps"][r, 0]), int(b["numsteps"][r, 1])
        ob, on = int(gen["base"][i]), int(ls["compacted_numsteps"][i])
        if cn != on:
            continue
        same += 1
        got_c, ref_c = b["coords"][cb:cb + cn], gen["coords"][ob:ob + cn]
        ray_coord = float(np.abs(got_c - ref_c).max()) if cn else 0.0
        if ray_coord > coord_tol and count_tol > 2e-4:
            shifted += 1  # a position on a cell wall taken on one side and not on the other: the rest of the ray is shifted by one
            continue
        worst_coord = max(worst_coord, ray_coord)
        loss_got.append(float(b["loss"][r]))
        loss_ref.append(float(ls["loss"][i]))
        # fill_rollover_and_rescale: sample at compacted index c carries 1 + copies * n / target
        copies = (TARGET - 1 - np.arange(cb, cb + cn)) // n_compacted
        ref_d = ls["dloss"][ob:ob + cn].astype(np.float32)
        ref_d = ref_d + copies[:, None] * (ref_d * np.float32(scale)).astype(np.float16).astype(np.float32)
        dl_err.append(np.abs(b["dloss"][cb:cb + cn].astype(np.float32) - ref_d).reshape(-1))
        dl_ref.append(np.abs(ref_d).reshape(-1))
        checked += cn
    assert same >= same_frac * n_kept and checked > 20000
    assert worst_coord <= coord_tol and shifted <= 0.005 * n_kept
    # per-ray losses (already divided by n_rays): the two sides evaluate the network with fp16 outputs that differ by ulps
    loss_got, loss_ref = np.array(loss_got), np.array(loss_ref)
    lerr = np.abs(loss_got - loss_ref)
    # (the model IS the ground truth here, so the losses are the fp16 noise floor: compared in sum and with a loose per-ray bound)
    loose = count_tol > 2e-4
    assert np.median(lerr / np.maximum(loss_ref, 1e-12)) < (3e-2 if loose else 1e-2) and lerr.sum() < (3e-2 if loose else 1e-2) * loss_ref.sum()
    assert np.all(lerr <= 0.25 * loss_ref + 1e-7)  # positions, dt, directions: the same arithmetic up to the device's division / exp
    dl_err, dl_ref = np.concatenate(dl_err), np.concatenate(dl_ref)
    # the network outputs differ by fp16 ulps (test_network_outputs); gradients inherit that through sigmoid' / exp
    assert np.sum(dl_err) <= (0.03 if loose else 0.02) * np.sum(dl_ref) and np.quantile(dl_err, 0.999) <= 0.05 * dl_ref.max()
    oracle.release(m)
