"""The schedule knobs of the persistent render kernel (ngp_set_schedule, NGP_TUNE) are "performance only, except block_jumps"
(include/ngp_hip.h); bench.py tunes on the strength of that sentence. Here every kernel the knobs reach renders the same frames under a
designed set of schedules, and rgba, depth and the counters have to be the same BYTES as under the anchor schedule -- not a tolerance: a
ray's samples are emitted and composited in its own order, and one sample's network output does not depend on which samples share its
MFMA tile. The anchor (64, 1, 1, 0, 1, 1, 1, 0) -- one sample per ray and round, the network as soon as anything waits, no stalling, no
hand-over -- is the schedule closest to the reference's loop, and its frame is compared with the CPU oracle: oracle -> anchor -> every
other schedule.

Schedules (tests/schedule_frames.py): anchor, default, each knob but block_jumps alone at its lowest and highest allowed value, the corners
all-low, all-high and mixed; anchor, default and the corners again with block_jumps = 0, compared among themselves (block_jumps
legitimately changes sample sets). Frames: one per kernel the knobs reach, the kernel asserted by name (ngp_last_render_kernel). The wide
kernel (Frequency / Identity encodings) overwrites knobs 1-3 from its own table and its block_jumps is tested in test_frequency_gpu.py: it
is left out. The stamped *_prof twins are diagnostics: out of scope.

Why every wave makes progress at the corners (csrc/nerf_kernels.hip fused_body; written down before the first run of the in-range
extremes). A round ends in one of three ways: no sample waits (the marching lanes have each advanced max_it >= 1 steps towards the end
of their ray: box exit, opacity or MARCH_ITER); a stall (counted, the counter is reset only by a network run); network + composite
(empties the list). A ray slot is free as soon as its ray ends, and the refill hands a wave n_dead >> 4 strips.
  all low  (16, 1, 1, 0, 1, 1, *, 0): max_it = max(skip_steps, k_max) = 1, one march step per round, never zero. go_min 1 / max_stall 0:
    `n_slots < 1` is false whenever a sample waits, so the network runs in that round. refill_min 16: 16 free slots ask for one strip
    (want = n_dead >> 4 >= 1). share 0: a wave leaves once the queue is dry and no lane is alive or waits to be shaded.
  all high (64, 64, 64, 64, 8, 8, *, 1): refill_min 64 refills only a wave whose 64 slots are all free -- every ray ends, and a finished
    lane counts as free, so n_dead reaches 64; a dry queue retires at any count. go_min 64 can hold the network back only while
    can_march (some lane has fewer than k_max samples waiting and is neither blocked by the full list nor out of the box) and for
    max_stall = 64 rounds at most; a full list (64 slots) runs at once. k = 8: a lane that finds the list full stands still for the
    round and emits the same sample in the next. share 1: an idle wave spins on s_xstate / s_active with s_sleep and leaves when
    s_active is 0; every busy wave lowers it exactly once, a donor raises it before it publishes rays, and busy waves end by the above.
  mixed    (16, 64, 64, 0, 8, 1, *, 1): max_stall 0 makes `stall < 0` false, so go_min 64 never delays anything: the network runs in
    every round that emitted a sample. k_busy 8 / k_drain 1 flips the per-ray sample count when the live rays fall to 32; hand-over as above.
The probe kernel (compute_envmap, trace_nerf_rays) reads knobs 0-3 only (k_max = 1, no hand-over): the same three arguments.

The hand-over really happens in these frames: MEASURED_HANDOVERS below, measured once on an MI355X with a temporary counter in
fused_body (rays received through s_xray, summed over the frame's waves; not committed). Every frame of more than one tile hands
thousands of rays over under every schedule with share = 1 and none with share = 0; the counts depend on the waves' timing and move
from run to run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import schedule_frames as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "schedule_frames.py")
COUNTERS = ("n_rays", "n_rays_alive_after_init", "n_rays_hit", "n_samples")
# rays handed from a busy wave to an idle one, per frame, default schedule / all-high corner / mixed corner (see the module docstring)
MEASURED_HANDOVERS = {
    "unit/pinhole": (7872, 6615, 5432), "unit/inside": (6307, 6115, 5395), "unit/share8": (1627, 1318, 1220), "unit/packed": (13048, 10218, 9846),
    "unit/odd_101x67": (1303, 811, 864), "unit/8x8": (0, 0, 0), "unit/1x1": (0, 0, 0), "unit/spp4": (19232, 15884, 13393),
    "unit/depth_of_field": (7797, 6375, 5216), "unit/depth_of_field_envmap": (7071, 5852, 4854), "unit/normals": (3230, 2578, 1997),
    "unit/hybrid": (2813, 1895, 1605), "big/pinhole": (4427, 3340, 3851), "big/depth_of_field": (3893, 2875, 2993),
    "big_beyond_grid/pinhole": (5506, 3553, 3892), "rgb_1layer/pinhole": (7185, 6660, 5548), "rgb_3layer/pinhole": (6902, 5954, 5206),
    "rgb_0layer/pinhole": (7238, 6485, 5609), "linear/pinhole": (6316, 5448, 4817),
}


def _child(args=(), env=None, timeout=900):
    """Runs tests/schedule_frames.py; a time-out or a crash reports the last progress line: the schedule and frame it happened on."""
    try:
        r = subprocess.run([sys.executable, CHILD, *args], env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        last = [l for l in out.splitlines() if l.startswith("SCHED ")][-1:]
        pytest.fail(f"the render child did not finish in {timeout} s; last progress line: {last}")
    progress = [l for l in r.stdout.splitlines() if l.startswith("SCHED ")]
    assert r.returncode == 0, f"last progress line: {progress[-1:]}\n{r.stderr[-2000:]}"
    line = [l for l in r.stdout.splitlines() if l.startswith("RECORDS ")]
    assert line, r.stdout[-1000:]
    return json.loads(line[-1][len("RECORDS "):])


@pytest.fixture(scope="module")
def records(native):
    return _child()


def _row(r):
    return "%-5s %-24s %-16s %-22s %-34s rgba %s depth %s rays %s alive %s hit %s samples %s" % (
        r["group"], ",".join(map(str, r["schedule"])), r["model"], r["frame"], r["kernel"], r["rgba"][:12], r["depth"][:12],
        r.get("n_rays", "-"), r.get("n_rays_alive_after_init", "-"), r.get("n_rays_hit", "-"), r.get("n_samples", "-"))


def test_schedule_set_is_the_designed_one():
    """the schedule lists are what the module docstring says, every value inside validate_schedule's ranges"""
    jumps, exact = SF.SCHEDULES["jumps"], SF.SCHEDULES["exact"]
    assert jumps[0] == (64, 1, 1, 0, 1, 1, 1, 0) and jumps[1] == (64, 4, 32, 1, 1, 4, 1, 1)
    one = SF.one_knob_schedules()
    assert len(one) == 14 and set(one) <= set(jumps)
    for i, (lo, hi) in enumerate(SF.RANGE):
        if i != 6:
            for v in (lo, hi):
                assert SF.DEFAULT[:i] + (v,) + SF.DEFAULT[i + 1:] in one, (i, v)
    assert sorted(s for s in one if s == SF.DEFAULT) == [SF.DEFAULT] * 3  # refill_min 64, k_busy 1, share 1
    assert {(16, 1, 1, 0, 1, 1, 1, 0), (64, 64, 64, 64, 8, 8, 1, 1), (16, 64, 64, 0, 8, 1, 1, 1)} <= set(jumps)
    assert len(jumps) == len(set(jumps)) == 2 + 14 - 3 + 3
    assert exact == ((64, 1, 1, 0, 1, 1, 0, 0), (64, 4, 32, 1, 1, 4, 0, 1), (16, 1, 1, 0, 1, 1, 0, 0), (64, 64, 64, 64, 8, 8, 0, 1), (16, 64, 64, 0, 8, 1, 0, 1))
    for s in jumps + exact:
        assert len(s) == 8 and all(lo <= v <= hi for v, (lo, hi) in zip(s, SF.RANGE)), s
    assert all(s[6] == 1 for s in jumps) and all(s[6] == 0 for s in exact)
    assert len(SF.FRAMES) == 21 and len(set((m, f) for m, f, _ in SF.FRAMES)) == 21
    assert {k for _, _, k in SF.FRAMES} == {"render_nerf_fused" + s for s in ("", "_unit", "_unit_plain", "_c5", "_c5_plain", "_mid0", "_mid2", "_lin_rgb", "_lin", "_normals")} | {"trace_probe_fused"}


@pytest.mark.gpu
def test_frames_are_the_same_bytes_under_every_schedule(records):
    """21 frames x (16 schedules with block jumps + 5 without): rgba, depth, n_rays, n_rays_alive_after_init, n_rays_hit and n_samples
    ("network queries composited": samples a ray emits past its terminating one are dropped, not counted) equal the anchor's of the
    group; every frame shows something and ran the kernel it is listed for. No record is left out."""
    for r in records:
        print(_row(r))
    assert len(records) == 21 * 16 + 21 * 5
    want = [(g, s, m, f) for m in dict.fromkeys(m for m, _, _ in SF.FRAMES) for g in ("jumps", "exact") for s in SF.SCHEDULES[g] for mm, f, _ in SF.FRAMES if mm == m]
    assert [(r["group"], tuple(r["schedule"]), r["model"], r["frame"]) for r in records] == want
    kernel_of = {(m, f): k for m, f, k in SF.FRAMES}
    anchors = {}
    compared = 0
    for r in records:
        key = (r["group"], r["model"], r["frame"])
        where = _row(r)
        assert r["kernel"] == kernel_of[(r["model"], r["frame"])], where
        assert r["nonzero"] > 0, where
        if r["frame"] in SF.PROBE_FRAMES:
            assert not any(c in r for c in COUNTERS), where  # (not a camera frame: no counters to compare)
        else:
            assert r["n_rays_hit"] > 0 and r["n_samples"] > 0, where
        a = anchors.setdefault(key, r)
        assert tuple(a["schedule"]) == SF.SCHEDULES[r["group"]][0]
        differing = {k: (r[k], r[k + "_first"]) for k in ("diff_rgba", "diff_depth") if r[k]}
        assert not differing, f"pixels that differ from the anchor's, and the first of them: {differing}\n{where}\n{_row(a)}"
        assert r["rgba"] == a["rgba"] and r["depth"] == a["depth"], f"{where}\n{_row(a)}"
        for c in COUNTERS:
            assert r.get(c) == a.get(c), f"{c}\n{where}\n{_row(a)}"
        compared += 1
    assert compared == 21 * 16 + 21 * 5 and len(anchors) == 21 * 2
    # block jumps on and off are different marches of the same scene: the two groups are not trivially the same pictures
    assert any(anchors[("jumps", m, f)]["rgba"] != anchors[("exact", m, f)]["rgba"] for m, f, _ in SF.FRAMES)


@pytest.mark.gpu
def test_anchor_schedule_matches_the_oracle(gpu_ctx, oracle, native, scene_mod, scene_unit):
    """the anchor schedule's unit_plain 256x144 frame at az 45 against the CPU oracle, with the assertions of test_render_unit_scene"""
    from test_parity_gpu import _render_both, assert_image_close

    w, h = 256, 144
    gpu_ctx.clear_meshes()
    try:
        gpu_ctx.set_schedule(*SF.ANCHOR)
        img, depth, st, ref, db, ost = _render_both(gpu_ctx, oracle, native, scene_mod, scene_unit, w, h, 45.0)
        assert gpu_ctx.last_render_kernel() == "render_nerf_fused_unit_plain"
    finally:
        gpu_ctx.set_schedule(*SF.DEFAULT)
    print({k: (int(st[k]), int(ost[k])) for k in ("n_rays_alive_after_init", "n_rays_hit", "n_samples")})
    assert st["n_rays"] == ((w + 7) // 8) * ((h + 7) // 8) * 64
    assert abs(int(st["n_rays_alive_after_init"]) - int(ost["n_rays_alive_after_init"])) <= 2
    assert abs(int(st["n_rays_hit"]) - int(ost["n_rays_hit"])) <= 3
    assert abs(int(st["n_samples"]) - int(ost["n_samples"])) <= 1e-4 * ost["n_samples"]
    assert st["n_samples"] / max(st["n_rays_hit"], 1) > 10
    assert_image_close(img, ref, 50.0)
    assert (np.abs(img[..., 3] - ref[..., 3]) < 5e-3).mean() > 0.9995
    both = (depth < 16000) & (db < 16000)
    assert both.sum() > 1000 and (np.not_equal(depth >= 16000, db >= 16000)).sum() <= 3
    assert np.median(np.abs(depth[both] - db[both])) < 1e-4


@pytest.mark.gpu
def test_ngp_tune_sets_the_same_schedule(records):
    """NGP_TUNE (read at ngp_create) = the mixed corner, set_schedule never called: the two frames are the bytes set_schedule gave"""
    env = _child(["--env-route"], env={"NGP_TUNE": ",".join(map(str, SF.MIXED))}, timeout=300)
    assert [(r["model"], r["frame"]) for r in env] == list(SF.ENV_FRAMES) and len(env) == 2
    for r in env:
        print(_row(r))
        same = [q for q in records if q["group"] == "jumps" and tuple(q["schedule"]) == SF.MIXED and (q["model"], q["frame"]) == (r["model"], r["frame"])]
        assert len(same) == 1 and tuple(r["schedule"]) == SF.MIXED
        for k in ("rgba", "depth", "kernel") + COUNTERS:
            assert r[k] == same[0][k], f"{k}\n{_row(r)}\n{_row(same[0])}"


NGP_TUNE_SCRIPT = """
import importlib, sys
sys.path.insert(0, {root!r})
native = importlib.import_module("surface-irradiance-estimation-from-neural-radiance-fields_amd.native")
ctx = native.Context(-1)
ctx.close()
print("CREATED")
"""


@pytest.mark.parametrize("tune,knob", [("65", "refill_min = 65"), ("64,0", "skip_steps = 0"), ("64,4,32,1,1,4,1,2", "share = 2"), ("x", None)])
def test_ngp_tune_goes_through_the_schedule_gate(native, tune, knob):
    """the environment route on a host-only context: an out-of-range list fails the creation with the message ngp_set_schedule gives
    (no number at all is refused as well)"""
    r = subprocess.run([sys.executable, "-c", NGP_TUNE_SCRIPT.format(root=ROOT)], env=dict(os.environ, NGP_TUNE=tune), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "CREATED" not in r.stdout, r.stdout + r.stderr
    assert "ngp_create failed" in r.stderr
    if knob:
        lo, hi = SF.RANGE[SF.KNOBS.index(knob.split(" ")[0])]
        assert f"schedule knob {knob} outside [{lo}, {hi}]" in r.stderr, r.stderr
        ctx = native.Context(-1)
        with pytest.raises(RuntimeError) as e:  # the same words as through ngp_set_schedule
            ctx.set_schedule(*(int(v) for v in tune.split(",")))
        ctx.close()
        assert f"schedule knob {knob} outside [{lo}, {hi}]" in str(e.value)
    else:
        assert "NGP_TUNE" in r.stderr, r.stderr


@pytest.mark.parametrize("tune", ["16,64,64,0,8,1,1,1", "32,8", "64,4,32,1,1,4,0,0", ""])
def test_ngp_tune_accepts_a_valid_list(native, tune):
    r = subprocess.run([sys.executable, "-c", NGP_TUNE_SCRIPT.format(root=ROOT)], env=dict(os.environ, NGP_TUNE=tune), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CREATED" in r.stdout, r.stdout + r.stderr
