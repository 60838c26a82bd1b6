"""The unit render kernels' tile cull (csrc/nerf_kernels.hip tile_cull, csrc/tile_probe.h) drops a camera tile right after ray setup when no
ray of it can meet an occupied cell. Such rays emit no sample, so the cull changes nothing but the time: libngp_hip.so and
libngp_hip_nocull.so (-DNGP_NO_TILE_CULL) are compared as BYTES -- rgba, depth, the four counters, the kernel's name. A difference is a
tile that was culled although one of its rays had something in front of it. Each build renders in a process of its own.

Mutation check, done by hand: with the dilation left out of near_table_word (dx = dy = dz = 0 only) the comparison below fails; the
figures are in DESIGN.md 3.3."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import tile_cull_cases as T
from conftest import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tile_cull_frames.py")], env=dict(os.environ, NGP_HIP_LIBRARY=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, r.stdout[-1000:]
    return json.loads(line[-1][len("RESULT "):])


@pytest.mark.gpu
def test_frames_with_and_without_tile_cull_are_equal_as_bytes(native, tmp_path):
    """Small frames with the benchmark's pixel footprint that look past the object's edge (256 x 144, and 250 x 140 with partial edge tiles;
    a packed 1-of-3 share), a camera inside the cube, a wide-angle frame whose tiles spread too far for the bound (no tile goes), a camera
    turned away from the object (every tile goes, and the launch still ends), the non-plain unit kernel, block_jumps = 0, frames after a
    training occupancy refresh, and one 1920 x 1080 benchmark frame."""
    build = pkg("build")
    lib_cull, lib_plain = build.build(), build.build(nocull=True)
    digest = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()
    assert digest(lib_cull) != digest(lib_plain), "the two libraries are the same file: the cull is not compared with anything"
    cull, plain = _frames(lib_cull), _frames(lib_plain)
    assert set(cull) == set(plain) and len(cull) == 12
    for name in sorted(cull):
        print(name, cull[name], plain[name])
        a, b = dict(cull[name]), dict(plain[name])
        culled, tiles = a.pop("culled"), a.pop("tiles")
        assert b.pop("culled") == 0 and b.pop("tiles") == tiles, name  # (the twin culls nothing)
        assert a["kernel"] == ("render_nerf_fused_unit" if name.endswith("depth_of_field") else "render_nerf_fused_unit_plain"), name
        assert a == b, name
        if name == "away":
            assert culled == tiles and a["n_rays_hit"] == 0 and a["n_samples"] == 0
        elif name == "wide":
            assert culled == 0 and a["n_samples"] > 0
        elif name == "inside" or name.startswith("refresh"):
            assert a["n_samples"] > 0  # (inside, the CPU model keeps every tile; the refresh: below)
        else:
            if name.endswith("packed"):
                tiles = len(range(1, tiles, 3))
            assert 0 < culled < tiles, name  # some tiles went and some stayed
            assert a["n_rays_hit"] > 0 and a["n_samples"] > 0 and a["nonzero"] > 0, name
    # the refresh changed the occupancy for good -- five times the rays find something -- so tables left over from before it, which culled 4 tiles
    # in 9 of this very frame, would have culled rays that now emit: the equal bytes above say that the tables followed the bitfield
    before, after = cull["before_refresh_narrow"], cull["refresh_narrow"]
    assert before["culled"] > 200 and after["n_rays_alive_after_init"] > 5 * before["n_rays_alive_after_init"] and after["culled"] < before["culled"] // 4
    # the GPU's count is the CPU model's (tests/aux/tile_probe_check.cpp: the same header on the host, rays formed in the same fp32 steps)
    exe = T.build_check(tmp_path, sanitize=False)
    cams = T.gpu_cameras()
    _, _, res = T.run_check(exe, tmp_path, T.bench_occupancy(), [cams["narrow"], cams["narrow_odd"]], "gpu_frames")
    for name, (dec, false_culls) in zip(("narrow", "narrow_odd"), res):
        assert false_culls == 0 and cull[name]["culled"] == int((dec != 0).sum()), (name, cull[name]["culled"], int((dec != 0).sum()))
