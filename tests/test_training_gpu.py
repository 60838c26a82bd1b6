"""Training step against the oracle: sample generation and loss ray by ray, the fused
backward against the float64 restatement, the optimizer, and an end-to-end fit of images rendered from a known scene."""
import os
import sys

import numpy as np
import pytest

from conftest import pkg, psnr
from training_cases import FOV, H, POSES, TARGET, W
from training_cases import check_batch_against_oracle as _check_batch_against_oracle
from training_cases import ctx_with_data as _ctx_with_data
from training_cases import srgb_bytes as _srgb_bytes

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

pytestmark = pytest.mark.gpu


def _make_dataset(tmp_dir, native, scene_mod, scene, aabb_scale=1, radius=4.03):
    """Ground-truth views of a synthetic scene from the renderer itself: linear, premultiplied RGBA."""
    ctx = native.Context(0)
    ctx.set_model(scene)
    focal = scene_mod.focal_from_fov_x(W, FOV)
    mats = [scene_mod.orbit_camera(az, el, radius=radius) for az, el in POSES]
    imgs = [ctx.render(native.make_camera(m, W, H, focal), native.make_opts(background=(0.0, 0.0, 0.0, 0.0))) for m in mats]
    ctx.close()
    path = scene_mod.write_transforms(os.path.join(str(tmp_dir), "transforms.json"), mats, W, H, FOV, aabb_scale=aabb_scale)
    return {"path": path, "images": imgs, "mats": mats, "focal": focal}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, native, scene_mod, scene_unit):
    return _make_dataset(tmp_path_factory.mktemp("ds"), native, scene_mod, scene_unit)


@pytest.fixture(scope="module")
def dataset_big(tmp_path_factory, native, scene_mod, scene_big):
    """aabb_scale 4: three cascades, exponential stepping (cone angle 1/256), cameras inside the training box."""
    return _make_dataset(tmp_path_factory.mktemp("ds4"), native, scene_mod, scene_big, aabb_scale=4, radius=3.0)


def _write_png(path, rgba, filter_type=0):
    """Minimal PNG encoder (8-bit RGBA, or RGB when alpha is dropped) with one filter type for every scanline."""
    import struct
    import zlib

    h, w, c = rgba.shape
    raw = bytearray()
    prev = np.zeros(w * c, np.int32)
    for y in range(h):
        cur = rgba[y].reshape(-1).astype(np.int32)
        left = np.concatenate([np.zeros(c, np.int32), cur[:-c]])
        upleft = np.concatenate([np.zeros(c, np.int32), prev[:-c]])
        if filter_type == 0:
            pred = np.zeros_like(cur)
        elif filter_type == 1:
            pred = left
        elif filter_type == 2:
            pred = prev
        elif filter_type == 3:
            pred = (left + prev) >> 1
        else:
            pq = left + prev - upleft
            pa, pb, pc = np.abs(pq - left), np.abs(pq - prev), np.abs(pq - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        raw.append(filter_type)
        raw += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6 if c == 4 else 2, 0, 0, 0))
    comp = zlib.compress(bytes(raw), 6)
    data += chunk(b"IDAT", comp[: len(comp) // 2]) + chunk(b"IDAT", comp[len(comp) // 2:]) + chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(data)


def test_sample_generation_and_loss_match_the_oracle(native, oracle, dataset, scene_unit):
    ctx = _ctx_with_data(native, dataset)
    _check_batch_against_oracle(ctx, oracle, dataset["images"], scene_unit)
    ctx.close()


@pytest.mark.parametrize("opts", [
    dict(loss_type=0, random_bg_color=0, background_color=(0.2, 0.4, 0.6), snap_to_pixel_centers=0, linear_colors=1),  # L2, fixed background, free uv, linear
    dict(loss_type=6, color_space=0, near_distance=0.5),  # RelativeL2, linear colour space targets, a wide near-distance penalty
    dict(loss_type=1, random_bg_color=0),  # L1 on the default black background
])
def test_training_options_reach_the_kernels(native, oracle, dataset, scene_unit, opts):
    ctx = _ctx_with_data(native, dataset)
    _check_batch_against_oracle(ctx, oracle, dataset["images"], scene_unit, opts=opts)
    ctx.close()


def test_exponential_decay_schedule(native, dataset, scene_unit):
    """tcnn ExponentialDecay around Adam (configs/nerf/base.json: decay_start 20000, decay_interval 10000, decay_base 0.33):
    the rate drops by decay_base at optimizer steps decay_start, decay_start + decay_interval, ..."""
    ctx = _ctx_with_data(native, dataset)
    ctx.set_model(scene_unit)
    ctx.set_training_opts(decay_start=3, decay_interval=2, decay_base=0.5)
    rates = []
    for _ in range(7):
        ctx.train(1, 1 << 15)
        rates.append(ctx.training_state()["learning_rate"])
    assert np.allclose(rates, [0.01, 0.01, 0.005, 0.005, 0.0025, 0.0025, 0.00125], rtol=1e-6)
    # the step after a drop moves the weights by the lower rate (first Adam steps move by ~lr)
    ctx.close()


def test_train_network_and_encoding_switches(native, dataset, scene_unit):
    """m_train_network / m_train_encoding -> optimize_matrix_params / optimize_non_matrix_params (src/testbed.cu:4436-4442)"""
    for net, enc in ((1, 0), (0, 1)):
        ctx = _ctx_with_data(native, dataset)
        ctx.set_model(scene_unit)
        ctx.set_training_opts(train_network=net, train_encoding=enc)
        w0, _ = ctx.training_params()
        ctx.train(2, 1 << 15)
        w1, _ = ctx.training_params()
        assert (np.any(w1[:10240] != w0[:10240])) == bool(net) and (np.any(w1[10240:] != w0[10240:])) == bool(enc)
        ctx.close()


def test_sample_generation_and_loss_with_cascades(native, oracle, dataset_big, scene_big):
    """mip_from_dt across cascades, exponential stepping in calc_dt / advance_to_next_voxel, rays that start inside the box."""
    ctx = _ctx_with_data(native, dataset_big)
    assert ctx.dataset_info()["aabb_scale"] == 4
    _check_batch_against_oracle(ctx, oracle, dataset_big["images"], scene_big, coord_tol=2e-5, same_frac=0.96, count_tol=5e-3)
    ctx.close()


def test_training_fits_with_cascades(native, scene_mod, dataset_big):
    ctx = _ctx_with_data(native, dataset_big)
    ctx.reset_network(log2_hashmap_size=15, seed=7)
    assert ctx.get_model().aabb_scale == 4 and abs(ctx.get_model().cone_angle_constant - 1 / 256) < 1e-9
    first = ctx.train(1, 1 << 16)
    last = ctx.train(400, 1 << 16)
    assert np.isfinite(last) and last < 0.15 * first, (first, last)
    cam = native.make_camera(dataset_big["mats"][5], W, H, dataset_big["focal"])
    got = ctx.render(cam, native.make_opts(background=(0.0, 0.0, 0.0, 0.0)))
    assert psnr(got[..., :3], dataset_big["images"][5][..., :3]) > 20.0
    ctx.close()


def test_png_images_decode_to_the_same_batch(native, oracle, dataset, scene_unit, tmp_path, scene_mod):
    """ngp_load_training_images: PNG files with every scanline filter type and split IDAT chunks; the per-ray loss is
    compared with the oracle reading the very bytes that were encoded."""
    os.makedirs(tmp_path / "train")
    pixels = [_srgb_bytes(im) for im in dataset["images"]]
    for i, px in enumerate(pixels):
        _write_png(str(tmp_path / "train" / f"r_{i:04d}.png"), px, filter_type=i % 5)
    path = scene_mod.write_transforms(str(tmp_path / "transforms.json"), dataset["mats"], W, H, FOV)
    ctx = native.Context(0)
    ctx.load_training_data(path)
    assert ctx.load_training_images() == len(pixels)
    _check_batch_against_oracle(ctx, oracle, pixels, scene_unit)
    # an RGB file (no alpha) and a missing file: the first loads opaque, the second leaves its view without pixels
    _write_png(str(tmp_path / "train" / "r_0000.png"), np.ascontiguousarray(pixels[0][..., :3]), filter_type=4)
    os.remove(tmp_path / "train" / "r_0001.png")
    ctx.load_training_data(path)
    assert ctx.load_training_images() == len(pixels) - 1
    ctx.close()


def _split(g):
    return g[:10240], g[10240:]


def test_backward_matches_the_float64_oracle(native, dataset, scene_unit):
    import train_oracle as T

    ctx = _ctx_with_data(native, dataset)
    ctx.set_model(scene_unit)
    b = ctx.train_prepare_batch(TARGET)
    n = int(b["counters"][2])
    g = ctx.train_gradients(TARGET).astype(np.float64)
    params = np.asarray(scene_unit["params"], np.uint16).view(np.float16).astype(np.float64)
    ref = T.backward(params, scene_unit["encoding"], b["coords"][:n].astype(np.float64), b["dloss"][:n].astype(np.float64))
    assert g.shape == ref.shape and np.isfinite(g).all()
    for name, (got, want) in {"matrices": (_split(g)[0], _split(ref)[0]), "grid": (_split(g)[1], _split(ref)[1])}.items():
        cos = float(got @ want / (np.linalg.norm(got) * np.linalg.norm(want)))
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        # fp16 activations and gradients in the device path (like the reference), float64 in the oracle
        assert cos > 0.9995 and rel < 0.03, (name, cos, rel)
    # every layer on its own: a wrong fragment would hide in the total
    for lo, hi in ((0, 2048), (2048, 3072), (3072, 5120), (5120, 9216), (9216, 10240)):
        got, want = g[lo:hi], ref[lo:hi]
        assert np.linalg.norm(got - want) <= 0.03 * np.linalg.norm(want), (lo, hi)
    # untouched grid entries receive exactly nothing; touched ones may underflow to zero in the fp16 hand-over
    gz, rz = _split(g)[1] != 0, _split(ref)[1] != 0
    assert not np.any(gz & ~rz) and np.mean(gz != rz) < 0.01
    ctx.close()


def test_optimizer_step_matches_adam_and_ema(native, dataset, scene_unit):
    import train_oracle as T

    ctx = _ctx_with_data(native, dataset)
    ctx.set_model(scene_unit)
    ctx.train_prepare_batch(TARGET)
    g = ctx.train_gradients(TARGET).astype(np.float64)
    w0, _ = ctx.training_params()
    ctx.train_apply()
    w1, ema1 = ctx.training_params()
    w = w0.astype(np.float64)
    m1, m2, steps = np.zeros_like(w), np.zeros_like(w), np.zeros(w.size, np.int64)
    upd = T.adam_step(w, g, m1, m2, steps, 10240)
    assert np.allclose(w1, w, rtol=1e-5, atol=1e-7)
    assert np.array_equal(w1[~upd], w0[~upd])  # grid entries no sample touched
    moved = np.abs(w1 - w0)[upd]
    sel = np.abs(g[upd]) > 1e-6
    bad = np.flatnonzero(np.abs(moved[sel] - 0.01) > 1e-5)
    ui = np.flatnonzero(upd)[sel]
    assert bad.size == 0, (bad.size, ui[bad][:8], moved[sel][bad][:8], g[ui[bad]][:8], w0[ui[bad]][:8])  # first Adam step: lr * m / sqrt(v) = lr
    ema = T.ema_step(w0.astype(np.float64).copy(), w1.astype(np.float16).astype(np.float64), 1)
    assert np.allclose(ema1, ema, rtol=1e-5, atol=1e-7)
    st = ctx.training_state()
    assert st["training_step"] == 1 and st["measured_batch_size"] > 0 and st["rays_per_batch"] > 4096 and st["loss"] > 0
    ctx.close()


def test_training_fits_the_rendered_views(native, scene_mod, dataset, tmp_path):
    ctx = _ctx_with_data(native, dataset, byte_images=True)
    ctx.reset_network(log2_hashmap_size=15, seed=1337)
    losses = [ctx.train(1, 1 << 16)]
    losses += [ctx.train(50, 1 << 16) for _ in range(8)]
    st = ctx.training_state()
    assert st["training_step"] == 401 and np.isfinite(losses).all()
    assert losses[-1] < 0.1 * losses[0], losses
    cam = native.make_camera(dataset["mats"][2], W, H, dataset["focal"])
    got = ctx.render(cam, native.make_opts(background=(0.0, 0.0, 0.0, 0.0)))
    ref = dataset["images"][2]
    assert psnr(got[..., :3], ref[..., :3]) > 22.0
    # a held-out pose between two training views
    ctx_gt_psnr = psnr(got[..., 3], ref[..., 3])
    assert ctx_gt_psnr > 15.0
    # the trained model survives a snapshot round trip (training parameters, like the reference's Trainer::serialize)
    p = str(tmp_path / "trained.ingp")
    ctx.save_snapshot_file(p)
    ctx2 = native.Context(0)
    ctx2.load_snapshot_file(p)
    again = ctx2.render(cam, native.make_opts(background=(0.0, 0.0, 0.0, 0.0)))
    assert psnr(again[..., :3], ref[..., :3]) > 20.0
    ctx2.close()
    ctx.close()


def test_training_errors(native, dataset):
    ctx = native.Context(0)
    with pytest.raises(RuntimeError, match="No network available"):
        ctx.train(1, 1 << 14)
    ctx.reset_network(log2_hashmap_size=14)
    with pytest.raises(RuntimeError, match="No training data available"):
        ctx.train(1, 1 << 14)
    ctx.load_training_data(dataset["path"])
    ctx.set_training_image(0, dataset["images"][0])
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ctx.train(1, 1000)
    with pytest.raises(RuntimeError, match="invalid frame index"):
        ctx.set_training_image(99, dataset["images"][0])
    ctx.close()


def test_pyngp_and_cli_train_a_png_dataset(native, dataset, scene_mod, tmp_path):
    """scripts/run.py's loop -- load_training_data, shall_train, frame() until training_step -- and ngp_hip_main's
    --n_steps / --save_snapshot on a dataset of PNG files."""
    import subprocess

    os.makedirs(tmp_path / "train")
    for i, im in enumerate(dataset["images"]):
        _write_png(str(tmp_path / "train" / f"r_{i:04d}.png"), _srgb_bytes(im), filter_type=1 + i % 4)
    scene_mod.write_transforms(str(tmp_path / "transforms.json"), dataset["mats"], W, H, FOV)
    ngp = pkg("build").import_pyngp()
    testbed = ngp.Testbed()
    testbed.render_mode = ngp.RenderMode.Shade  # (the fork's default, ShadeGridEnvMap, leaves NeRF colours un-linearised: tests/test_pyngp.py)
    testbed.load_training_data(str(tmp_path))
    assert testbed.nerf.training.n_images_for_training == len(POSES) and testbed.nerf.training.loss_type == ngp.LossType.Huber
    testbed.training_batch_size = 1 << 16
    testbed.shall_train = True
    first = None
    while testbed.frame():
        assert not testbed.want_repl()  # run.py:185
        if first is None:
            first = testbed.loss
        if testbed.training_step >= 300:
            break
    assert testbed.training_step == 300 and 0 < testbed.loss < 0.2 * first
    testbed.shall_train = False
    assert testbed.frame() and testbed.training_step == 300
    # scripts/run.py --test_transforms (run.py:210-262): ground truth of a view, then the render of the same camera
    testbed.background_color = [0.0, 0.0, 0.0, 1.0]
    testbed.snap_to_pixel_centers = True
    testbed.nerf.render_min_transmittance = 1e-4
    res = testbed.nerf.training.dataset.metadata[2].resolution
    testbed.render_ground_truth = True
    testbed.set_camera_to_training_view(2)
    ref_image = testbed.render(res[0], res[1], 1, True)
    testbed.render_ground_truth = False
    image = testbed.render(res[0], res[1], 4, True)
    assert ref_image.shape == image.shape == (H, W, 4) and psnr(image[..., :3], ref_image[..., :3]) > 20.0
    testbed.reset()
    assert testbed.training_step == 0
    del testbed
    exe = pkg("build").build_main()
    (tmp_path / "small.json").write_text('{"encoding": {"otype": "HashGrid", "log2_hashmap_size": 15}}')
    out = subprocess.run([exe, "--scene", str(tmp_path), "--network", str(tmp_path / "small.json"), "--n_steps", "120", "--save_snapshot", str(tmp_path / "out.ingp"),
                          "--screenshot", str(tmp_path / "shot.png"), "--width", "64", "--height", "64"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(tmp_path / "out.ingp") > 100000 and os.path.getsize(tmp_path / "shot.png") > 200
    ctx = native.Context(0)
    ctx.load_snapshot_file(str(tmp_path / "out.ingp"))
    assert ctx.get_model().log2_hashmap_size == 15
    ctx.close()


def test_render_ground_truth_is_the_training_image(native, dataset):
    """CudaRenderBuffer::overlay_image (src/render_buffer.cu:344-414), the m_render_ground_truth path of scripts/run.py
    --test_transforms: same resolution -> the image itself over the background; other resolutions -> nearest resampling
    about the centre; byte images decode through sRGB."""
    from conftest import psnr as _psnr

    ctx = _ctx_with_data(native, dataset)
    img = dataset["images"][3]
    a = img[..., 3:4]
    # Linear colour space: premultiplied colour + (1 - a) * srgb_to_linear(bg)
    bg = np.array([0.25, 0.5, 0.75, 1.0], np.float32)
    bg_lin = np.where(bg[:3] <= 0.04045, bg[:3] / 12.92, ((bg[:3] + 0.055) / 1.055) ** 2.4)
    got = ctx.render_ground_truth(3, W, H, background=bg, color_space=0)
    want = np.concatenate([img[..., :3] + (1 - a) * bg_lin, a + (1 - a)], -1)
    assert np.abs(got - want).max() < 2e-6
    # exposure doubles linear values; sRGB output applies the transfer curve
    got2 = ctx.render_ground_truth(3, W, H, background=bg, color_space=0, exposure=1.0)
    assert np.allclose(got2[..., :3], 2 * want[..., :3], rtol=1e-5, atol=1e-6)
    # SRGB colour space (the default): blending happens on sRGB values, the result returns to linear; opaque pixels are unchanged
    got3 = ctx.render_ground_truth(3, W, H, background=(0, 0, 0, 1), color_space=1)
    opaque = a[..., 0] > 0.9999
    assert opaque.sum() > 100 and np.abs(got3[opaque][:, :3] - img[opaque][:, :3]).max() < 2e-3
    # half resolution: pixel (x, y) shows source pixel (2x + 1, 2y + 1)
    half = ctx.render_ground_truth(3, W // 2, H // 2, background=bg, color_space=0)
    assert np.abs(half - want[1::2, 1::2]).max() < 2e-6
    # zoom 2 about the centre: the middle half of the image, each source pixel twice
    zoomed = ctx.render_ground_truth(3, W, H, background=bg, color_space=0, zoom=2.0)
    assert np.abs(zoomed[::2, ::2] - want[H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2]).max() < 2e-6
    with pytest.raises(RuntimeError, match="Invalid training view"):
        ctx.render_ground_truth(99, W, H)
    ctx.close()
    # byte images: sRGB, straight alpha
    ctx = _ctx_with_data(native, dataset, byte_images=True)
    got4 = ctx.render_ground_truth(3, W, H, background=(0, 0, 0, 1), color_space=0)
    assert _psnr(got4[..., :3], img[..., :3]) > 38.0  # 8-bit quantisation of the colours and of alpha
    ctx.close()


def test_transparency_flags_and_dynamic_masks(native, dataset, scene_mod, scene_unit, tmp_path):
    """convert_rgba32 (src/nerf_loader.cu:41-63) and the dynamic mask beside an image (:596-615)."""
    import json

    os.makedirs(tmp_path / "train")
    px = np.zeros((H, W, 4), np.uint8)
    px[..., 3] = 255
    px[: H // 2] = [255, 255, 255, 255]   # white half
    px[H // 2:, : W // 2] = [0, 0, 0, 255]  # black quarter
    px[H // 2:, W // 2:] = [200, 40, 90, 255]
    for i in range(len(POSES)):
        _write_png(str(tmp_path / "train" / f"r_{i:04d}.png"), px, filter_type=0)
    path = scene_mod.write_transforms(str(tmp_path / "transforms.json"), dataset["mats"], W, H, FOV)
    j = json.load(open(path))
    j["white_transparent"] = True
    json.dump(j, open(path, "w"))
    ctx = native.Context(0)
    ctx.load_training_data(path)
    assert ctx.load_training_images() == len(POSES)
    gt = ctx.render_ground_truth(0, W, H, background=(0.0, 0.0, 0.0, 0.0), color_space=0)
    assert (gt[: H // 2, :, 3] == 0).all() and (gt[H // 2:, :, 3] == 1).all()  # white became transparent, black stayed
    j["white_transparent"], j["black_transparent"] = False, True
    json.dump(j, open(path, "w"))
    ctx.load_training_data(path)
    ctx.load_training_images()
    gt = ctx.render_ground_truth(0, W, H, background=(0.0, 0.0, 0.0, 0.0), color_space=0)
    assert (gt[: H // 2, :, 3] == 1).all() and (gt[H // 2:, : W // 2, 3] == 0).all() and (gt[H // 2:, W // 2:, 3] == 1).all()
    # a mask that covers every image entirely: no ray can be drawn
    mask = np.full((H, W, 4), 255, np.uint8)
    for i in range(len(POSES)):
        _write_png(str(tmp_path / "train" / f"dynamic_mask_r_{i:04d}.png"), mask, filter_type=0)
    ctx.load_training_data(path)
    ctx.load_training_images()
    ctx.set_model(scene_unit)
    b = ctx.train_prepare_batch(1 << 15)
    assert b["counters"][1] == 0 and b["counters"][0] == 0
    # half-masked: rays only from the unmasked half
    mask[:, W // 2:] = 0
    for i in range(len(POSES)):
        _write_png(str(tmp_path / "train" / f"dynamic_mask_r_{i:04d}.png"), mask, filter_type=0)
    ctx.load_training_data(path)
    ctx.load_training_images()
    ctx.set_model(scene_unit)
    b = ctx.train_prepare_batch(1 << 15)
    assert 0 < b["counters"][1] < 4096
    _write_png(str(tmp_path / "train" / "dynamic_mask_r_0000.png"), mask[:10], filter_type=0)
    ctx.load_training_data(path)
    with pytest.raises(RuntimeError, match="wrong resolution"):
        ctx.load_training_images()
    ctx.close()
