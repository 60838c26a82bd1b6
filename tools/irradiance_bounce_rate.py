"""What bounces cost on the MI355X: the wall time of a 16^3 volume at 32 x 32 rays a probe on the benchmark's model among the meshes of
tools/mesh_shade_rate.py's scene with N = 0, 1, 2 and 4 bounce passes, and the device time of one pass.

    python tools/irradiance_bounce_rate.py [--res 16] [--k 32] [--repeat 3] [--out profiles/irradiance_bounce_rate.json]
    python tools/irradiance_bounce_rate.py --sun [--repeat 5] [--out profiles/irradiance_sun_rate.json]
    python tools/irradiance_bounce_rate.py --sun --nerf-shadow [--repeat 6] [--out profiles/irradiance_sun_shadow_rate.json]
    python tools/irradiance_bounce_rate.py --mesh-albedos [--repeat 8] [--out profiles/irradiance_mesh_albedo_rate.json]

The volume spans the box of the meshes (it overlaps the NeRF's unit cube), the meshes occlude, albedo 0.64. Wall times are
medians over --repeat calls after a warm-up and include the host's share; the pass time is HIP events around the last pass's chunks in
the context's stream (ngp_get_irradiance_bounce_ms), the median over the same calls, with the plain and with the visible lookup (distance
maps of 16 x 16 rays, computed inside the call and inside its wall time). Nothing is asserted on these numbers. Needs a GPU; there is
no CPU path.

--sun measures the sun pass instead (ngp_get_irradiance_sun_ms), beside the bounce pass and the NeRF trace of the same call: a volume with
the frames' sun (1, 1, 1) and N = 1, every repeat listed so that the run-to-run spread shows. It then runs the same calls in a child process
on libngp_hip_sun_any_hit.so (build.py: build(sun_any_hit=True)), whose shadow query is an unsorted traversal that ends at the first hit
instead of the shipped closest hit: what that early exit would buy. --lib PATH measures one library alone and builds nothing.

--sun --nerf-shadow measures what the NeRF's density in front of the sun costs: the same volume with and without sun_nerf_shadow, every
repeat listed, the shadow trace's own device time (ngp_get_irradiance_sun_shadow_ms) and its tracer statistics beside the V_0 trace's, and
the share of the uncompacted shadow-ray list that is live (one stage pass at the volume's probes, outside the timing).

--mesh-albedos measures what the meshes' own albedos cost (ngp_set_mesh_albedo): the sunlit volume with N = 2 while no mesh owns an
albedo and while every mesh owns one (0.64, so that both compute the same records), in alternating calls of one process: the device time of
the sun pass and of the last bounce pass, and the wall time of the call, as medians with their p10 and p90."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "surface-irradiance-estimation-from-neural-radiance-fields_amd"
BOUNCES = (0, 1, 2, 4)


def pkg(sub):
    import importlib

    return importlib.import_module(PKG + "." + sub)


def timed(ctx, f, repeat):
    """median wall time of `repeat` calls of f after one warm-up call, and the median of the last pass's device time behind each"""
    f()
    ts, dev = [], []
    for _ in range(repeat):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
        dev.append(ctx.irradiance_bounce_ms())
    return float(np.median(ts)), float(np.median(dev))


def load(native, synthetic):
    """the benchmark's model among mesh_shade_rate's meshes: (context, the box of the meshes)"""
    from mesh_shade_rate import scene

    ctx = native.Context(0)
    ctx.set_model(synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19))
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i, (tris, center) in enumerate(scene()):
        ctx.add_mesh(tris, center)
        bmin, bmax = ctx.mesh_info(i)["aabb"]
        lo, hi = np.minimum(lo, bmin), np.maximum(hi, bmax)
    return ctx, (lo.astype(np.float32), hi.astype(np.float32))


def sun_passes(args):
    """the device times of --repeat sunlit volumes with one bounce pass on the library native.py loads: every repeat's sun pass, bounce pass
    and trace, ms"""
    native, synthetic = pkg("native"), pkg("synthetic")
    ctx, box = load(native, synthetic)
    res, k = (args.res,) * 3, args.k
    sun, bounce, trace = [], [], []
    for i in range(args.repeat + 1):
        ctx.compute_irradiance_volume(res, box, k, k, bounces=1, albedo=0.64, sun=((1.0, 1.0, 1.0), native.SUN_RADIANCE, 1e-3))
        if i:  # (the first call warms up)
            sun.append(round(ctx.irradiance_sun_ms(), 3))
            bounce.append(round(ctx.irradiance_bounce_ms(), 3))
            trace.append(round(ctx.render_stats()["kernel_ms"], 3))
    _, sh = ctx.get_irradiance_volume()
    ctx.close()
    return {"library": os.path.basename(native.load_library()._name), "sun_pass_ms": sun, "bounce_pass_ms": bounce, "trace_ms": trace,
            "blocked_share": round(float(1.0 - sh[..., 27].mean()), 4)}


def main_sun_shadow(args):
    pkg("build").build()
    native, synthetic = pkg("native"), pkg("synthetic")
    ctx, box = load(native, synthetic)
    res, k = (args.res,) * 3, args.k
    sun = ((1.0, 1.0, 1.0), native.SUN_RADIANCE, 1e-3)
    out = {"how": "HIP events around the chunks of the last sun pass (sun_pass_ms), around the shadow rays' prep and trace inside it (shadow_trace_ms), and the tracer's kernel time "
                  "and samples of the last tracer call (plain: the V_0 trace; shadowed: the shadow trace), of a sunlit volume with N = 1; every repeat after a warm-up; "
                  "plain and shadowed alternate call by call in one session; one MI355X, one run",
           "resolution": [args.res] * 3, "rays_per_probe": k * k, "rays": args.res ** 3 * k * k, "albedo": 0.64, "sun": [1, 1, 1], "min_transmittance": 0.01, "t_min": 0.0,
           "plain": {"sun_pass_ms": [], "v0_trace_ms": [], "v0_trace_samples": []}, "shadowed": {"sun_pass_ms": [], "shadow_trace_ms": [], "shadow_trace_kernel_ms": [], "shadow_trace_samples": []}}
    for i in range(args.repeat + 1):
        for name, shadow in (("plain", None), ("shadowed", True)):
            ctx.compute_irradiance_volume(res, box, k, k, bounces=1, albedo=0.64, sun=sun, sun_nerf_shadow=shadow)
            if not i:  # (the first call of each warms up)
                continue
            st, o = ctx.render_stats(), out[name]
            o["sun_pass_ms"].append(round(ctx.irradiance_sun_ms(), 3))
            if shadow:
                o["shadow_trace_ms"].append(round(ctx.irradiance_sun_shadow_ms(), 3))
                o["shadow_trace_kernel_ms"].append(round(st["kernel_ms"], 3))
                o["shadow_trace_samples"].append(int(st["n_samples"]))
            else:
                o["v0_trace_ms"].append(round(st["kernel_ms"], 3))
                o["v0_trace_samples"].append(int(st["n_samples"]))
    # the list's live share: the probes of the volume, as the library places them (double from the box's floats, rounded to float)
    ax = [(np.float64(box[0][a]) + np.arange(args.res) / max(args.res - 1, 1) * (np.float64(box[1][a]) - np.float64(box[0][a]))).astype(np.float32) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    probes = np.stack([x, y, z], -1).reshape(-1, 3)
    live = blocked = n = 0
    for p0 in range(0, probes.shape[0], 512):
        _, shadow = ctx.irradiance_sh_sun(probes[p0:p0 + 512], sun, 0.64, k, k, nerf_shadow=True, return_shadow=True)
        has = np.any(shadow[..., :3] != 0, axis=-1)
        live, blocked, n = live + int(has.sum()), blocked + int((shadow[..., 3][has] > 0.9).sum()), n + has.size
    ctx.close()
    out["live_share"] = round(live / n, 4)
    out["blocked_share_of_live"] = round(blocked / max(live, 1), 4)
    med = lambda v: float(np.median(v))
    print(f"sun pass: plain {out['plain']['sun_pass_ms']} ms, shadowed {out['shadowed']['sun_pass_ms']} ms; shadow trace {out['shadowed']['shadow_trace_ms']} ms; "
          f"V_0 trace {out['plain']['v0_trace_ms']} ms; live share {out['live_share']}", flush=True)
    out["medians"] = {"sun_pass_plain_ms": med(out["plain"]["sun_pass_ms"]), "sun_pass_shadowed_ms": med(out["shadowed"]["sun_pass_ms"]),
                      "shadow_trace_ms": med(out["shadowed"]["shadow_trace_ms"]), "v0_trace_ms": med(out["plain"]["v0_trace_ms"])}
    print(json.dumps(out))
    path = args.out or os.path.join(ROOT, "profiles", "irradiance_sun_shadow_rate.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def main_mesh_albedos(args):
    pkg("build").build()
    native, synthetic = pkg("native"), pkg("synthetic")
    ctx, box = load(native, synthetic)
    res, k = (args.res,) * 3, args.k
    sun = ((1.0, 1.0, 1.0), native.SUN_RADIANCE, 1e-3)
    n_meshes = ctx.n_meshes()
    out = {"how": "a sunlit volume with N = 2: HIP events around the chunks of the sun pass and of the last bounce pass, and the wall time of the call; none: no mesh owns an "
                  "albedo (the kernels that take the call's three scalars); every: every mesh owns 0.64 (their per-mesh twins, one float4 of the call's table a hit ray); the "
                  "two alternate call by call in one process after a warm-up call of each; medians with p10 and p90 over --repeat calls; one MI355X, one run",
           "resolution": [args.res] * 3, "rays_per_probe": k * k, "rays": args.res ** 3 * k * k, "albedo": 0.64, "sun": [1, 1, 1], "n_bounces": 2, "meshes": n_meshes,
           "none": {"sun_pass_ms": [], "bounce_pass_ms": [], "wall_ms": []}, "every": {"sun_pass_ms": [], "bounce_pass_ms": [], "wall_ms": []}}
    records = {}
    for i in range(args.repeat + 1):
        for name in ("none", "every"):
            for m in range(n_meshes):
                ctx.set_mesh_albedo(m, 0.64 if name == "every" else None)
            t0 = time.perf_counter()
            ctx.compute_irradiance_volume(res, box, k, k, bounces=2, albedo=0.64, sun=sun)
            wall = time.perf_counter() - t0
            if not i:  # (the first call of each warms up)
                continue
            o = out[name]
            o["sun_pass_ms"].append(round(ctx.irradiance_sun_ms(), 3))
            o["bounce_pass_ms"].append(round(ctx.irradiance_bounce_ms(), 3))
            o["wall_ms"].append(round(1e3 * wall, 2))
            records[name] = ctx.get_irradiance_volume()[1].tobytes()
    ctx.close()
    out["same_records"] = records["none"] == records["every"]
    out["summary"] = {}
    for name in ("none", "every"):
        out["summary"][name] = {key: {"median": round(float(np.median(v)), 3), "p10": round(float(np.percentile(v, 10)), 3), "p90": round(float(np.percentile(v, 90)), 3)}
                                for key, v in out[name].items()}
        print(f"{name:5s}: " + ", ".join(f"{key} {q['median']} ({q['p10']}-{q['p90']})" for key, q in out["summary"][name].items()), flush=True)
    print(json.dumps(out))
    path = args.out or os.path.join(ROOT, "profiles", "irradiance_mesh_albedo_rate.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def main_sun(args):
    import subprocess

    if args.nerf_shadow:
        return main_sun_shadow(args)

    if args.lib:  # one library, as the parent asks
        os.environ["NGP_HIP_LIBRARY"] = os.path.abspath(args.lib)
        print(json.dumps(sun_passes(args)))
        return
    out = {"how": "HIP events around the chunks of the last sun pass and bounce pass, and the tracer's kernel time, of a sunlit volume with N = 1; every repeat after a warm-up; "
                  "closest_hit: the shipped library; any_hit: the same calls on the build whose shadow query ends at the first hit; one MI355X, one run",
           "resolution": [args.res] * 3, "rays_per_probe": args.k * args.k, "rays": args.res ** 3 * args.k * args.k, "albedo": 0.64, "sun": [1, 1, 1]}
    for name, lib in (("closest_hit", pkg("build").build()), ("any_hit", pkg("build").build(sun_any_hit=True))):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sun", "--lib", lib, "--res", str(args.res), "--k", str(args.k), "--repeat", str(args.repeat)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stdout + r.stderr)
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{name:11s}: sun pass {out[name]['sun_pass_ms']} ms, bounce pass {out[name]['bounce_pass_ms']} ms, trace {out[name]['trace_ms']} ms", flush=True)
    print(json.dumps(out))
    path = args.out or os.path.join(ROOT, "profiles", "irradiance_sun_rate.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=16)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sun", action="store_true")
    ap.add_argument("--nerf-shadow", action="store_true", help="with --sun: what the NeRF's density in front of the sun costs")
    ap.add_argument("--mesh-albedos", action="store_true", help="what the meshes' own albedos cost in a sunlit volume with N = 2")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.mesh_albedos:
        return main_mesh_albedos(args)
    if args.sun:
        return main_sun(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "irradiance_bounce_rate.json")
    pkg("build").build()
    native, synthetic = pkg("native"), pkg("synthetic")
    ctx, box = load(native, synthetic)
    res, k = (args.res,) * 3, args.k
    rays = args.res ** 3 * k * k
    out = {"how": "median wall time of --repeat calls after a warm-up; pass = HIP events around the last bounce pass's chunks, the median over the same calls; one MI355X, one run",
           "resolution": list(res), "rays_per_probe": k * k, "rays": rays, "albedo": 0.64, "plain": {}, "visible": {}}
    for name, vis in (("plain", None), ("visible", {})):
        for n in BOUNCES:
            if n == 0 and vis is not None:
                continue
            kw = dict(bounces=n, albedo=0.64, visibility=vis) if n else {}
            t, dev = timed(ctx, lambda: ctx.compute_irradiance_volume(res, box, k, k, **kw), args.repeat)
            out[name][str(n)] = {"wall_ms": round(1e3 * t, 2), "pass_device_ms": round(dev, 3) if n else None, "pass_ms_per_million_rays": round(dev / (rays * 1e-6), 3) if n else None}
            print(f"{name:7s} N = {n}: {1e3 * t:8.2f} ms wall" + (f", one pass {dev:.3f} ms on the device ({dev / (rays * 1e-6):.3f} ms per million rays)" if n else ""), flush=True)
    d, sh = ctx.get_irradiance_volume()
    out["blocked_share"] = round(float(1.0 - sh[..., 27].mean()), 4)
    ctx.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
