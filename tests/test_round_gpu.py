"""The render round outside the network (csrc/nerf_kernels.hip fused_body: march, composite, retire) was trimmed of work its result
does not need: the occupancy summaries and a copy of the bitfield's block words are indexed by block coordinates instead of a Morton code
(csrc/occ_index.h, rebuilt whenever the bitfield changes), and a ray that ends by transmittance is normalised when it is shaded instead
of in the composite. libngp_hip_round_v1.so (-DNGP_ROUND_V1) keeps the earlier forms, layouts included; both libraries run the same
arithmetic on the same values, so frames, depth and counters are compared as BYTES. Each library works in a process of its own
(tests/round_frames.py).

Mutation check on an MI355X: with lane 5 left out of the deferred normalisation, 21 of the 22 records differ from
libngp_hip_round_v1.so in their rgba digest (all but kernels/wide, which wide_kernels.hip renders); depth and counters stay equal."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = {
    "kernels/normals": "render_nerf_fused_normals", "kernels/probe_rays": "trace_probe_fused", "kernels/c5_plain": "render_nerf_fused_c5_plain",
    "kernels/c5": "render_nerf_fused_c5", "kernels/c5_plain_exact_march": "render_nerf_fused_c5_plain", "kernels/generic": "render_nerf_fused",
    "kernels/wide": "wide",
}


def _run(lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "round_frames.py")], env=dict(os.environ, NGP_HIP_LIBRARY=lib), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, r.stdout[-1000:]
    return json.loads(line[-1][len("RESULT "):])


@pytest.mark.gpu
def test_trimmed_round_gives_the_same_bytes(native):
    """The frame list of tests/test_netsec_gpu.py (both unit kernels under the default and the EXACT_MARCH schedule: plain, inside the
    object, depth of field, a 1/8 share; both 1080p frames; the render box beyond the unit cube), one frame each through c5, c5_plain
    (also with the reference's climb), the generic kernel (8 cascades, rays from outside the grid), normals, one probe call and the
    frequency.json kernel, and frames after a training occupancy refresh: every digest of rgba and depth, all four counters and the
    kernel's name of libngp_hip.so equal those of libngp_hip_round_v1.so."""
    build = pkg("build")
    lib_new, lib_v1 = build.build(), build.build(round_v1=True)
    digest = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()
    assert digest(lib_new) != digest(lib_v1), "the two libraries are the same file: nothing is compared"
    new, v1 = _run(lib_new), _run(lib_v1)
    assert set(new) == set(v1) and len(new) == 8 + 2 + 2 + 7 + 3
    for name in sorted(new):
        print(name, new[name], v1[name])
        assert new[name]["nonzero"] > 0, name  # (a frame of something)
        if name != "kernels/probe_rays":
            assert new[name]["n_rays_hit"] > 0 and new[name]["n_samples"] > 0, name
        if name in KERNELS:
            assert new[name]["kernel"] == KERNELS[name], name
        elif name.startswith(("default/", "exact_march/", "wide_box/", "refresh/")):
            assert new[name]["kernel"] == ("render_nerf_fused_unit" if name.endswith("depth_of_field") else "render_nerf_fused_unit_plain"), name
        assert new[name] == v1[name], name
    # the refresh changed the occupancy grid (else the frames behind it prove nothing about rebuilt tables)
    assert new["refresh/after"]["n_samples"] != new["refresh/before"]["n_samples"]
