"""Traced-irradiance rates on the MI355X: rays per second of the trace stage of ngp_irradiance_traced against a probe fan
(ngp_compute_envmap, multi-centre) of about the same number of rays on the same model, and wall times of the pipeline and of its stage entries.

    python tools/irradiance_rate.py [--points 65536] [--k 16] [--repeat 3] [--out profiles/irradiance_rate.json]

Models: the benchmark's (bench.py: synthetic aabb_scale 1, 2^19 table) and the committed fox snapshot. Points lie in the middle of the
occupancy grid with random normals. Device times are the tracer's own clock (kernel_device_ms, summed over the 2^21-ray chunks);
per-kernel times of the generator and the reduction come from a rocprofv3 --kernel-trace --stats run of this tool.
Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "surface-irradiance-estimation-from-neural-radiance-fields_amd"
FOX = os.path.join(ROOT, "tests", "golden", "fox", "fox_base_t16.ingp")


def pkg(sub):
    import importlib

    return importlib.import_module(PKG + "." + sub)


def wall(f, repeat):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def measure(ctx, n_points, k, repeat):
    rng = np.random.default_rng(0)
    p = rng.uniform(0.3, 0.7, (n_points, 3)).astype(np.float32)
    nrm = rng.normal(size=(n_points, 3)).astype(np.float32)
    n_rays = n_points * k * k
    ctx.irradiance_traced(p, nrm, n_u=k, n_v=k)  # warm-up
    t_total, _ = wall(lambda: ctx.irradiance_traced(p, nrm, n_u=k, n_v=k), repeat)
    st = ctx.render_stats()
    t_gen, _ = wall(lambda: ctx.irradiance_rays(p, nrm, n_u=k, n_v=k), repeat)
    # probe fans of about the same number of rays: a 128 x 64 texture traced from n_origin^2 Halton-jittered centres per texel
    nt, nph = 128, 64
    no = int(np.ceil(np.sqrt(n_rays / (nt * nph))))
    ctx.compute_envmap(2, nt, nph, n_origin=no)
    t_probe, _ = wall(lambda: ctx.compute_envmap(2, nt, nph, n_origin=no), repeat)
    sp = ctx.render_stats()
    traced = n_rays / (st["kernel_device_ms"] * 1e-3)
    probe = sp["n_rays"] / (sp["kernel_device_ms"] * 1e-3)
    return {"points": n_points, "rays_per_point": k * k, "rays": n_rays,
            "trace_kernel_ms": round(st["kernel_device_ms"], 3), "trace_grays_s": round(traced / 1e9, 3),
            "trace_samples": int(st["n_samples"]), "trace_samples_per_ray": round(st["n_samples"] / n_rays, 2),
            "irradiance_traced_wall_ms": round(1e3 * t_total, 2), "irradiance_rays_wall_ms_incl_readback": round(1e3 * t_gen, 2),
            "probe_fan": [nt, nph, no], "probe_rays": int(sp["n_rays"]), "probe_kernel_ms": round(sp["kernel_device_ms"], 3), "probe_grays_s": round(probe / 1e9, 3),
            "probe_samples_per_ray": round(sp["n_samples"] / sp["n_rays"], 2), "compute_envmap_wall_ms": round(1e3 * t_probe, 2),
            "probe_over_traced_per_ray": round(probe / traced, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pkg("build").build()
    native, synthetic = pkg("native"), pkg("synthetic")
    out = {"how": "median wall time of --repeat calls after a warm-up; trace and probe kernels on the tracer's device clock", "models": {}}
    for name in ("bench", "fox"):
        ctx = native.Context(0)
        if name == "bench":
            ctx.set_model(synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19))
        else:
            ctx.load_snapshot_file(FOX)
        r = measure(ctx, args.points, args.k, args.repeat)
        out["models"][name] = r
        print(f"{name:5s} {r['points']} points x {r['rays_per_point']} rays: trace {r['trace_kernel_ms']:.2f} ms = {r['trace_grays_s']:.2f} Grays/s "
              f"({r['trace_samples_per_ray']} samples/ray); probe fan {r['probe_kernel_ms']:.2f} ms = {r['probe_grays_s']:.2f} Grays/s "
              f"({r['probe_samples_per_ray']} samples/ray); irradiance_traced {r['irradiance_traced_wall_ms']:.1f} ms wall, "
              f"irradiance_rays {r['irradiance_rays_wall_ms_incl_readback']:.1f} ms wall", flush=True)
        ctx.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
