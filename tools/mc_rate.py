"""Marching-cubes rates on the MI355X: device-event times of the three stages of ngp_compute_marching_cubes_mesh (lattice, marching
cubes, normals + colours), lattice samples per second next to the render kernel's on the same model, and the bytes the marching-cubes
stages must move over their time as a share of HBM peak.

    python tools/mc_rate.py [--res 256 512] [--repeat 5] [--out profiles/mc_rate.json]

Models: the benchmark's (bench.py: synthetic aabb_scale 1, 2^19 table) and the committed fox snapshot. Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "surface-irradiance-estimation-from-neural-radiance-fields_amd"
HBM_PEAK = 8.0e12  # B/s, MI355X HBM3E spec
FOX = os.path.join(ROOT, "tests", "golden", "fox", "fox_base_t16.ingp")


def pkg(sub):
    import importlib

    return importlib.import_module(PKG + "." + sub)


def mc_bytes(n_points, nv, nt):
    """what the marching-cubes kernels must move: the fp32 lattice read by count, emit-vertices and emit-triangles (3 x 4 B), the
    per-point vertex offsets written and read back (2 x 4 B) and crossing masks (2 x 1 B), the vertices and triangles written (12 B each)"""
    return n_points * (3 * 4 + 2 * 4 + 2 * 1) + 12 * (nv + nt)


def render_rate(native, scene_mod, ctx):
    w, h = 1920, 1080
    cam = native.make_camera(scene_mod.orbit_camera(45.0), w, h, scene_mod.focal_from_fov_x(w, 0.6911))
    for _ in range(3):
        ctx.render(cam)
    st = ctx.render_stats()
    return st["n_samples"] / (st["kernel_ms"] * 1e-3), st


def measure(ctx, res, repeat):
    ctx.compute_marching_cubes_mesh(res)  # warm-up (code objects, allocations)
    runs = []
    for _ in range(repeat):
        m = ctx.compute_marching_cubes_mesh(res)
        runs.append(ctx.marching_cubes_timings())
    ms = np.median(np.asarray(runs), axis=0)
    n = res ** 3
    nv, nt = len(m["V"]), len(m["F"])
    b = mc_bytes(n, nv, nt)
    return {"res": res, "n_points": n, "n_verts": nv, "n_tris": nt, "lattice_ms": round(float(ms[0]), 3), "mc_ms": round(float(ms[1]), 3),
            "normals_colours_ms": round(float(ms[2]), 3), "lattice_gsamples_s": round(n / (ms[0] * 1e-3) / 1e9, 2), "mc_bytes": int(b),
            "mc_gb_s": round(b / (ms[1] * 1e-3) / 1e9, 1), "mc_hbm_share": round(b / (ms[1] * 1e-3) / HBM_PEAK, 3),
            "runs_ms": [[round(float(x), 3) for x in r] for r in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg("build").build()
    native, synthetic, scene_mod = pkg("native"), pkg("synthetic"), pkg("scene")
    out = {"hbm_peak_B_s": HBM_PEAK, "how": "HIP events around the stages of ngp_compute_marching_cubes_mesh (median of --repeat runs); "
           "the marching-cubes interval includes the read-back of the two totals that sizes the outputs", "models": {}}
    for name in ("bench", "fox"):
        ctx = native.Context(0)
        if name == "bench":
            ctx.set_model(synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19))
        else:
            ctx.load_snapshot_file(FOX)
        rate, st = render_rate(native, scene_mod, ctx)
        rows = [measure(ctx, r, args.repeat) for r in args.res]
        out["models"][name] = {"render_gsamples_s": round(rate / 1e9, 2), "render_kernel_ms": round(st["kernel_ms"], 3), "render_samples": int(st["n_samples"]),
                               "lattice": rows}
        for r in rows:
            print(f"{name:5s} {r['res']}^3: lattice {r['lattice_ms']:.3f} ms ({r['lattice_gsamples_s']:.1f} G/s; render {rate / 1e9:.1f} G/s), "
                  f"marching cubes {r['mc_ms']:.3f} ms ({r['mc_gb_s']:.0f} GB/s = {100 * r['mc_hbm_share']:.1f} % of HBM peak), "
                  f"normals + colours {r['normals_colours_ms']:.3f} ms; {r['n_verts']} vertices, {r['n_tris']} triangles", flush=True)
        ctx.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
