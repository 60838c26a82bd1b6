"""SH9 irradiance volume rates on the MI355X: what computing a 16^3 volume at 32 x 32 rays a probe costs, how much of it is spent outside
the tracer (generator, projection, copies, host) against the same share of ngp_irradiance_traced on an equal ray count in the same run,
and the lookup rate for random points and for points along a surface.

    python tools/irradiance_volume_rate.py [--res 16] [--k 32] [--lookups 1048576] [--repeat 3] [--out profiles/irradiance_volume_rate.json]

Models: the benchmark's (bench.py: synthetic aabb_scale 1, 2^19 table) and the committed fox snapshot. The volume spans the middle of the
occupancy grid. Tracer times are the tracer's own device clock (kernel_device_ms of the render stats, summed over the 2^21-ray chunks);
wall and tracer times are medians over the same --repeat calls after a warm-up; wall times include the host copies. Lookup bytes: 24 B in
and 16 B out a point plus the 8 x 112 B of probe records it reads (most of them from cache). Needs a GPU; there is no CPU path."""
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


def wall(f, repeat, after=None):
    """median wall time of `repeat` calls, the last result, and the median of after() taken behind every call"""
    ts, extra = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
        if after:
            extra.append(after())
    return float(np.median(ts)), r, (float(np.median(extra)) if after else None)


def measure(ctx, res, k, n_lookups, repeat):
    rng = np.random.default_rng(0)
    box = (np.float32([0.3, 0.3, 0.3]), np.float32([0.7, 0.7, 0.7]))
    probes, n_rays = res ** 3, res ** 3 * k * k
    ctx.compute_irradiance_volume((res,) * 3, box, k, k)  # warm-up
    device_ms = lambda: ctx.render_stats()["kernel_device_ms"]
    t_vol, _, dev_vol = wall(lambda: ctx.compute_irradiance_volume((res,) * 3, box, k, k), repeat, device_ms)
    sv = ctx.render_stats()
    # the same number of rays through ngp_irradiance_traced: one point per probe, k x k hemisphere rays each
    p = rng.uniform(0.3, 0.7, (probes, 3)).astype(np.float32)
    nrm = rng.normal(size=(probes, 3)).astype(np.float32)
    ctx.irradiance_traced(p, nrm, n_u=k, n_v=k)
    t_tr, _, dev_tr = wall(lambda: ctx.irradiance_traced(p, nrm, n_u=k, n_v=k), repeat, device_ms)
    st = ctx.render_stats()
    out = {"resolution": [res] * 3, "probes": probes, "rays_per_probe": k * k, "rays": n_rays,
           "volume_wall_ms": round(1e3 * t_vol, 2), "volume_trace_device_ms": round(dev_vol, 3),
           "volume_share_outside_tracer": round(1 - dev_vol * 1e-3 / t_vol, 3), "volume_samples_per_ray": round(sv["n_samples"] / n_rays, 2),
           "traced_wall_ms": round(1e3 * t_tr, 2), "traced_trace_device_ms": round(dev_tr, 3),
           "traced_share_outside_tracer": round(1 - dev_tr * 1e-3 / t_tr, 3), "traced_samples_per_ray": round(st["n_samples"] / n_rays, 2)}
    # lookups: random points in the box, and points along a surface (a sphere inside it, in the order of a lat-long sweep: neighbours share probes)
    q = rng.uniform(box[0], box[1], (n_lookups, 3)).astype(np.float32)
    nq = rng.normal(size=(n_lookups, 3)).astype(np.float32)
    side = int(np.sqrt(n_lookups))
    th, ph = np.meshgrid(np.linspace(0.01, np.pi - 0.01, side), np.linspace(0, 2 * np.pi, n_lookups // side, endpoint=False), indexing="ij")
    ns = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], -1).reshape(-1, 3).astype(np.float32)
    qs = (0.5 + 0.17 * ns).astype(np.float32)
    for name, (a, b) in (("random", (q, nq)), ("surface", (qs, ns))):
        ctx.irradiance_volume_at(a, b)
        t, e, _ = wall(lambda: ctx.irradiance_volume_at(a, b), repeat)
        n = a.shape[0]
        out["lookup_" + name] = {"points": n, "wall_ms_incl_copies": round(1e3 * t, 2), "points_per_s": round(n / t), "bytes_per_s": round(n * (24 + 16 + 8 * 112) / t),
                                 "mean_weight": round(float(e[:, 3].mean()), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=16)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--lookups", type=int, default=1 << 20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irradiance_volume_rate.json"))
    args = ap.parse_args()
    pkg("build").build()
    native, synthetic = pkg("native"), pkg("synthetic")
    out = {"how": "median wall time of --repeat calls after a warm-up, host copies included; tracer times on the tracer's device clock, the median over the same calls; "
                  "share outside the tracer = 1 - device time / wall time; lookup bytes = 40 B a point + 8 x 112 B of records", "models": {}}
    for name in ("bench", "fox"):
        ctx = native.Context(0)
        if name == "bench":
            ctx.set_model(synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19))
        else:
            ctx.load_snapshot_file(FOX)
        r = measure(ctx, args.res, args.k, args.lookups, args.repeat)
        out["models"][name] = r
        print(f"{name:5s} {r['probes']} probes x {r['rays_per_probe']} rays: volume {r['volume_wall_ms']:.1f} ms wall, tracer {r['volume_trace_device_ms']:.2f} ms "
              f"({100 * r['volume_share_outside_tracer']:.1f} % outside); irradiance_traced {r['traced_wall_ms']:.1f} ms wall, tracer {r['traced_trace_device_ms']:.2f} ms "
              f"({100 * r['traced_share_outside_tracer']:.1f} % outside); lookups {r['lookup_random']['points_per_s'] / 1e6:.1f} M/s random, "
              f"{r['lookup_surface']['points_per_s'] / 1e6:.1f} M/s along a surface", flush=True)
        ctx.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
