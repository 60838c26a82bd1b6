"""What the mesh pass costs per shade mode on the MI355X: the device time of render_mesh_fused at 1920 x 1080 on the meshes of the mesh
tests' render scene (cube, icosphere, upright torus; the icosphere and the torus finer, so that the BVHs have some depth), lit by the sky
term (Shade), by the grid of lat-long irradiance tables (ShadeGridEnvMap) and by the SH9 irradiance volume (ShadeIrradianceVolume) at 8^3 and
at 32^3 probes. With --visibility: Shade, the plain volume and the volume with its probes weighted by visibility (distance maps of 16 x 16 rays,
sharpness 2^5, default D) at 8^3 and 32^3 probes in one run, and the wall time of computing the maps of 16^3 probes x 16 x 16 rays.

    python tools/mesh_shade_rate.py [--width 1920] [--height 1080] [--frames 30] [--warmup 5] [--out profiles/mesh_shade_rate.json]
    python tools/mesh_shade_rate.py --visibility [--out profiles/mesh_shade_visibility_rate.json]
    python tools/mesh_shade_rate.py --sun-nerf-shadow [--out profiles/mesh_shade_sun_shadow_rate.json]

With --sun-nerf-shadow: per shade mode, in one run, the mesh pass with the option off (render_mesh_fused) and on (G-buffer kernel, prep and
ray-list trace of one shadow ray a local pixel, deferred shade kernel; ngp_set_sun_nerf_shadow at its defaults), of the latter the prep and
trace alone (ngp_get_frame_sun_shadow_ms), the frame's NeRF pass (kernel_ms) beside them, and how many pixels own a shadow ray.
    python tools/mesh_shade_rate.py --mesh-shadow-on-nerf [--out profiles/mesh_shadow_on_nerf_rate.json]
    python tools/mesh_shade_rate.py --mesh-materials [--out profiles/mesh_materials_rate.json]
    python tools/mesh_shade_rate.py --sun-disk [--sun-disk-rays K] [--out profiles/sun_disk_rate.json]

With --sun-disk: Shade-mode frames with the meshes' shadow on the NeRF on and the sun's disk (ngp_set_sun_disk) off, on in the wave layout and on
in the one-thread-a-pixel layout, alternating in one run, for the real sun's radius and for 5 degrees: the frame, the mesh pass, the disk
kernel and the NeRF shadow kernel.

With --mesh-shadow-on-nerf: Shade-mode frames with the meshes' shadow on the NeRF off and on (ngp_set_mesh_shadow_on_nerf at its defaults),
the calls alternating: the whole frame on the device (frame_ms), its NeRF pass (kernel_ms), its mesh pass, the new kernel alone
(ngp_get_frame_mesh_shadow_ms), and how many pixels own a surface point and how many of those a mesh shadows.
    python tools/mesh_shade_rate.py --ambient-change-on-nerf [--out profiles/ambient_change_on_nerf_rate.json]

With --ambient-change-on-nerf: Shade-mode frames with ngp_set_ambient_change_on_nerf off and on (its defaults), the calls alternating, in
two views: the one above, and one in which the NeRF fills the frame (the model alone over a far floor: the normals kernel's cost follows
the number of pixels that own a surface point). The volumes: 8^3 probes over the scene box, 16 x 16 rays, the context's with the meshes
occluding, sunlit and one bounce, the reference beside it. Per view: the whole frame (frame_ms), its NeRF pass (kernel_ms), its mesh pass,
the two new kernels together (ngp_get_frame_ambient_change_ms), and how many pixels own a surface point and how many were scaled.
    python tools/mesh_shade_rate.py --mesh-reflection [--out profiles/mesh_reflection_rate.json]

With --mesh-reflection: per shade mode, in one run, the mesh pass with ngp_set_mesh_reflection off (render_mesh_fused) and on at its defaults
(G-buffer kernel, reflection-ray kernel, prep and ray-list trace of one mirror ray a local pixel, deferred shade kernel), of the latter the
prep and trace alone (ngp_get_frame_mesh_reflection_ms), the frame's NeRF pass beside them, and how many pixels own a ray, how many of the
rays a mesh cuts and how many see the NeRF.
    python tools/mesh_shade_rate.py --mesh-reflection-meshes [--out profiles/mesh_reflection_meshes_rate.json]

With --mesh-reflection-meshes: per shade mode and view, in one process, ngp_set_mesh_reflection on with ngp_set_mesh_reflection_meshes off and
then on: the mesh pass, the reflection's prep and trace (which holds the new kernel), the hit-shade kernel alone
(ngp_get_frame_mesh_reflection_hits_ms), and the share of the rays that own a hit. Two views: the one above, whose mirror rays are hardly
ever cut, and a low view over a floor with a wall behind the model, whose floor mirrors the wall.

Times: HIP events around the mesh pass's launch in the frame's stream (ngp_get_mesh_pass_ms), median over --frames frames after --warmup.
The frames are Geometry-mode frames of the benchmark's model (bench.py) with the meshes; the tables and the volumes are traced in it, the
volumes over the scene box with the meshes occluding. Needs a GPU; there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "surface-irradiance-estimation-from-neural-radiance-fields_amd"


def pkg(sub):
    import importlib

    return importlib.import_module(PKG + "." + sub)


def scene():
    mi = pkg("meshio")
    cube = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.asarray([[cube[a], cube[b], cube[c]] for q in quads for a, b, c in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.float32)
    return [(tris, (0.0, 0.0, 0.0)), (mi.icosphere(4), (0.3, 1.6, 0.3)), (np.ascontiguousarray(mi.torus(96, 48)[..., [0, 2, 1]]), (1.15, 0.3, 0.0))]


def look_at(pos, target, up=(0.0, 0.0, 1.0)):
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    fwd = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross(fwd, np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(fwd, right), fwd, pos], 1).astype(np.float32)


def median_ms(ctx, cam, opts, frames, warmup):
    ts = []
    for i in range(warmup + frames):
        _, depth = ctx.render(cam, opts, want_depth=True)
        if i >= warmup:
            ts.append(ctx.mesh_pass_ms())
    return float(np.median(ts)), float(np.min(ts)), float((depth < 16384.0).mean()), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def median_on_off(ctx, cam, opts, frames, warmup, n_pixels):
    """the option off, then on, in one run: medians (and p10 / p90) of the mesh pass, of the shadow rays' prep and trace, and of the NeRF pass"""
    row = {}
    for key, shadow in (("off", None), ("on", True)):
        ctx.set_sun_nerf_shadow(shadow)
        mesh, trace, nerf = [], [], []
        for i in range(warmup + frames):
            ctx.render(cam, opts)
            if i >= warmup:
                mesh.append(ctx.mesh_pass_ms())
                trace.append(ctx.frame_sun_shadow_ms())
                nerf.append(ctx.render_stats()["kernel_ms"])
        q = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4), "p90_ms": round(float(np.percentile(x, 90)), 4)}
        row[key] = {"mesh_pass": q(mesh), "nerf_pass": q(nerf)}
        if shadow:
            row[key]["shadow_prep_and_trace"] = q(trace)
            rec = ctx.frame_sun_shadow(n_pixels)
            row[key]["pixels_with_shadow_ray"] = round(float(np.any(rec[:, :3] != 0, axis=1).mean()), 4)
            row[key]["shadow_rays_blocked_above_0.9"] = round(float((rec[:, 3] > 0.9).mean()), 4)
    ctx.set_sun_nerf_shadow(None)
    row["mesh_pass_on_over_off"] = round(row["on"]["mesh_pass"]["median_ms"] / row["off"]["mesh_pass"]["median_ms"], 3)
    row["gbuffer_and_shade_ms"] = round(row["on"]["mesh_pass"]["median_ms"] - row["on"]["shadow_prep_and_trace"]["median_ms"], 4)
    return row


def main_sun_nerf_shadow(args, ctx, native, cam, geo, lo, hi, out):
    out["how"] = ("per shade mode, one run: option off, then on (ngp_set_sun_nerf_shadow, min_transmittance 0.01, t_min 0). mesh_pass: HIP events around the whole mesh "
                  "pass of the frame (ngp_get_mesh_pass_ms: off = render_mesh_fused; on = G-buffer kernel, prep, ray-list trace, deferred shade); "
                  "shadow_prep_and_trace: HIP events around prep + trace inside it (ngp_get_frame_sun_shadow_ms); nerf_pass: the frame's NeRF launch "
                  "(ngp_get_render_stats kernel_ms); gbuffer_and_shade_ms = the difference of the first two medians. Medians of --frames frames after --warmup, "
                  "with p10 / p90. parent_off_median_ms: the parent commit's profiles/mesh_shade_rate.json, another run on another day.")
    parent = {}
    try:
        with open(os.path.join(ROOT, "profiles", "mesh_shade_rate.json")) as f:
            parent = {k: v["median_ms"] for k, v in json.load(f)["modes"].items()}
    except (OSError, KeyError, ValueError):
        pass
    rows = [("Shade", native.RENDER_SHADE, None), ("ShadeGridEnvMap", native.RENDER_SHADE_GRID_ENVMAP, "grid"),
            ("ShadeIrradianceVolume_8", native.RENDER_SHADE_IRRADIANCE_VOLUME, 8), ("ShadeIrradianceVolumeVisible_8", native.RENDER_SHADE_IRRADIANCE_VOLUME, -8)]
    for name, mode, what in rows:
        if what == "grid":
            ctx.compute_envmap_grid(8, 8, 64, 32)
        elif what is not None and what > 0:
            ctx.compute_irradiance_volume((what,) * 3, (lo, hi), 16, 16)
        elif what is not None:
            ctx.compute_irradiance_volume_visibility(16, 16, 5)
        row = median_on_off(ctx, cam, native.make_opts(render_mode=mode, **geo), args.frames, args.warmup, args.width * args.height)
        if name in parent:
            row["parent_off_median_ms"] = parent[name]
        out["modes"][name] = row
        print(f"{name:30s} mesh pass off {row['off']['mesh_pass']['median_ms']:.4f} ms, on {row['on']['mesh_pass']['median_ms']:.4f} ms "
              f"(prep + trace {row['on']['shadow_prep_and_trace']['median_ms']:.4f} ms), NeRF pass {row['on']['nerf_pass']['median_ms']:.4f} ms", flush=True)
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


def median_reflection_on_off(ctx, cam, opts, frames, warmup, n_pixels):
    """median_on_off for ngp_set_mesh_reflection: the option off, then on, in one run"""
    row = {}
    for key, reflection in (("off", None), ("on", True)):
        ctx.set_mesh_reflection(reflection)
        mesh, trace, nerf = [], [], []
        for i in range(warmup + frames):
            ctx.render(cam, opts)
            if i >= warmup:
                mesh.append(ctx.mesh_pass_ms())
                trace.append(ctx.frame_mesh_reflection_ms())
                nerf.append(ctx.render_stats()["kernel_ms"])
        q = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4), "p90_ms": round(float(np.percentile(x, 90)), 4)}
        row[key] = {"mesh_pass": q(mesh), "nerf_pass": q(nerf)}
        if reflection:
            row[key]["reflection_prep_and_trace"] = q(trace)
            rec = ctx.frame_mesh_reflection(n_pixels)
            owns = np.any(rec[:, 4:7] != 0, axis=1)
            row[key]["pixels_with_reflection_ray"] = round(float(owns.mean()), 4)
            row[key]["rays_cut_by_a_mesh"] = round(float((owns & np.isfinite(rec[:, 3])).mean()), 4)
            row[key]["rays_with_alpha_above_0"] = round(float((rec[:, 11] > 0).mean()), 4)
            row[key]["rays_with_alpha_above_0.9"] = round(float((rec[:, 11] > 0.9).mean()), 4)
    ctx.set_mesh_reflection(None)
    row["mesh_pass_on_over_off"] = round(row["on"]["mesh_pass"]["median_ms"] / row["off"]["mesh_pass"]["median_ms"], 3)
    row["gbuffer_rays_and_shade_ms"] = round(row["on"]["mesh_pass"]["median_ms"] - row["on"]["reflection_prep_and_trace"]["median_ms"], 4)
    return row


def main_mesh_reflection(args, ctx, native, cam, geo, lo, hi, out):
    out["how"] = ("per shade mode, one run: option off, then on (ngp_set_mesh_reflection, strength 1, min_transmittance 0.01, t_min 0). mesh_pass: HIP events around the whole "
                  "mesh pass of the frame (ngp_get_mesh_pass_ms: off = render_mesh_fused; on = G-buffer kernel, reflection-ray kernel, prep, ray-list trace, deferred shade); "
                  "reflection_prep_and_trace: HIP events around prep + trace inside it (ngp_get_frame_mesh_reflection_ms); nerf_pass: the frame's NeRF launch "
                  "(ngp_get_render_stats kernel_ms); gbuffer_rays_and_shade_ms = the difference of the first two medians. Medians of --frames frames after --warmup, "
                  "with p10 / p90. sun_shadow_run_off: the off figures of profiles/mesh_shade_sun_shadow_rate.json, another run on another day.")
    earlier = {}
    try:
        with open(os.path.join(ROOT, "profiles", "mesh_shade_sun_shadow_rate.json")) as f:
            earlier = {k: v["off"]["mesh_pass"] for k, v in json.load(f)["modes"].items()}
    except (OSError, KeyError, ValueError):
        pass
    rows = [("Shade", native.RENDER_SHADE, None), ("ShadeGridEnvMap", native.RENDER_SHADE_GRID_ENVMAP, "grid"),
            ("ShadeIrradianceVolume_8", native.RENDER_SHADE_IRRADIANCE_VOLUME, 8), ("ShadeIrradianceVolumeVisible_8", native.RENDER_SHADE_IRRADIANCE_VOLUME, -8)]
    for name, mode, what in rows:
        if what == "grid":
            ctx.compute_envmap_grid(8, 8, 64, 32)
        elif what is not None and what > 0:
            ctx.compute_irradiance_volume((what,) * 3, (lo, hi), 16, 16)
        elif what is not None:
            ctx.compute_irradiance_volume_visibility(16, 16, 5)
        row = median_reflection_on_off(ctx, cam, native.make_opts(render_mode=mode, **geo), args.frames, args.warmup, args.width * args.height)
        if name in earlier:
            row["sun_shadow_run_off"] = earlier[name]
            row["off_inside_that_runs_p10_p90"] = bool(earlier[name]["p10_ms"] <= row["off"]["mesh_pass"]["median_ms"] <= earlier[name]["p90_ms"])
        out["modes"][name] = row
        print(f"{name:30s} mesh pass off {row['off']['mesh_pass']['median_ms']:.4f} ms, on {row['on']['mesh_pass']['median_ms']:.4f} ms "
              f"(prep + trace {row['on']['reflection_prep_and_trace']['median_ms']:.4f} ms, the rest {row['gbuffer_rays_and_shade_ms']:.4f} ms), NeRF pass {row['on']['nerf_pass']['median_ms']:.4f} ms, "
              f"owners {row['on']['pixels_with_reflection_ray']}, alpha > 0: {row['on']['rays_with_alpha_above_0']}", flush=True)
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


def main_mesh_reflection_meshes(args, ctx, native, synthetic, cam, geo, lo, hi, out):
    out["how"] = ("per view and shade mode, one process: ngp_set_mesh_reflection on (strength 1, min_transmittance 0.01, t_min 0) with ngp_set_mesh_reflection_meshes off, then on. "
                  "mesh_pass: HIP events around the whole mesh pass (ngp_get_mesh_pass_ms); reflection_prep_and_trace: ngp_get_frame_mesh_reflection_ms, which holds the new "
                  "kernel; hit_shade_kernel: HIP events around mesh_reflection_hit_shade_kernel alone (ngp_get_frame_mesh_reflection_hits_ms). Medians of --frames frames after "
                  "--warmup, with p10 / p90. rays_with_a_hit: of all pixels; hits_of_the_rays: of the pixels that own a ray. Views: overhead, the other modes' view; "
                  "low_floor_and_wall: a floor under the model and a wall behind it, seen from low over the floor.")
    low = native.Context(0)
    low.set_model(synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19))
    cube = scene()[0][0]
    low.add_mesh((cube * np.float32([4.0, 0.04, 4.0])).astype(np.float32), (0.0, -0.6, 0.0))
    low.add_mesh((cube * np.float32([0.04, 1.0, 1.0])).astype(np.float32), (0.95, 0.4, 0.0))
    low.set_geometry_opts(sun_dir=(-1.0, 1.0, -0.3), ambientcolor=(0.3, 0.2, 0.1))
    llo, lhi = low.mesh_info(-1)["aabb"]
    low_cam = native.make_camera(look_at((-0.35, 1.3, -0.35), (0.3, -0.1, 0.3), up=(0.0, 1.0, 0.0)), args.width, args.height, (60.0 * args.width / 64.0,) * 2)
    rows = [("Shade", native.RENDER_SHADE, None), ("ShadeGridEnvMap", native.RENDER_SHADE_GRID_ENVMAP, "grid"),
            ("ShadeIrradianceVolume_8", native.RENDER_SHADE_IRRADIANCE_VOLUME, 8), ("ShadeIrradianceVolumeVisible_8", native.RENDER_SHADE_IRRADIANCE_VOLUME, -8)]
    q = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4), "p90_ms": round(float(np.percentile(x, 90)), 4)}
    n_pixels = args.width * args.height
    for view, c, view_cam, box in (("overhead", ctx, cam, (lo, hi)), ("low_floor_and_wall", low, low_cam, (llo, lhi))):
        out["modes"][view] = {}
        c.set_mesh_reflection(True)
        for name, mode, what in rows:
            if what == "grid":
                c.compute_envmap_grid(8, 8, 64, 32)
            elif what is not None and what > 0:
                c.compute_irradiance_volume((what,) * 3, box, 16, 16)
            elif what is not None:
                c.compute_irradiance_volume_visibility(16, 16, 5)
            opts = native.make_opts(render_mode=mode, **geo)
            row = {}
            for key, meshes in (("meshes_off", False), ("meshes_on", True)):
                c.set_mesh_reflection_meshes(meshes)
                mesh, trace, hits = [], [], []
                for i in range(args.warmup + args.frames):
                    c.render(view_cam, opts)
                    if i >= args.warmup:
                        mesh.append(c.mesh_pass_ms())
                        trace.append(c.frame_mesh_reflection_ms())
                        hits.append(c.frame_mesh_reflection_hits_ms())
                row[key] = {"mesh_pass": q(mesh), "reflection_prep_and_trace": q(trace)}
                if meshes:
                    row[key]["hit_shade_kernel"] = q(hits)
                    owns = np.any(c.frame_mesh_reflection(n_pixels)[:, 4:7] != 0, axis=1)
                    hit = c.frame_mesh_reflection_hits(n_pixels)[:, 7] != 0
                    row["pixels_with_reflection_ray"] = round(float(owns.mean()), 4)
                    row["rays_with_a_hit"] = round(float(hit.mean()), 4)
                    row["hits_of_the_rays"] = round(float(hit.sum() / max(1, owns.sum())), 4)
            c.set_mesh_reflection_meshes(False)
            row["mesh_pass_on_minus_off_ms"] = round(row["meshes_on"]["mesh_pass"]["median_ms"] - row["meshes_off"]["mesh_pass"]["median_ms"], 4)
            out["modes"][view][name] = row
            print(f"{view:20s} {name:30s} mesh pass {row['meshes_off']['mesh_pass']['median_ms']:.4f} -> {row['meshes_on']['mesh_pass']['median_ms']:.4f} ms, prep + trace "
                  f"{row['meshes_off']['reflection_prep_and_trace']['median_ms']:.4f} -> {row['meshes_on']['reflection_prep_and_trace']['median_ms']:.4f} ms, hit-shade kernel "
                  f"{row['meshes_on']['hit_shade_kernel']['median_ms']:.4f} ms, owners {row['pixels_with_reflection_ray']}, of them with a hit {row['hits_of_the_rays']}", flush=True)
        c.set_mesh_reflection(None)
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    low.close()
    ctx.close()


def main_mesh_shadow_on_nerf(args, ctx, native, cam, geo, out):
    out["how"] = ("Shade-mode Geometry frames, the option off and on (ngp_set_mesh_shadow_on_nerf, strength 0.5, bias 1e-2) in alternating calls of one run. frame: HIP "
                  "events around the whole frame (ngp_get_render_stats frame_ms); nerf_pass: its NeRF launch (kernel_ms); mesh_pass: ngp_get_mesh_pass_ms; "
                  "mesh_shadow_kernel: HIP events around nerf_mesh_shadow_kernel (ngp_get_frame_mesh_shadow_ms). Medians of --frames frames each after --warmup, with p10 / p90.")
    opts = native.make_opts(render_mode=native.RENDER_SHADE, **geo)
    ts = {key: {"frame": [], "nerf_pass": [], "mesh_pass": [], "mesh_shadow_kernel": []} for key in ("off", "on")}
    for i in range(args.warmup + args.frames):
        for key, shadow in (("off", None), ("on", True)):
            ctx.set_mesh_shadow_on_nerf(shadow)
            ctx.render(cam, opts)
            if i >= args.warmup:
                st = ctx.render_stats()
                ts[key]["frame"].append(st["frame_ms"])
                ts[key]["nerf_pass"].append(st["kernel_ms"])
                ts[key]["mesh_pass"].append(ctx.mesh_pass_ms())
                ts[key]["mesh_shadow_kernel"].append(ctx.frame_mesh_shadow_ms())
    rec = ctx.frame_mesh_shadow(args.width * args.height)  # (the last call was an on frame)
    ctx.set_mesh_shadow_on_nerf(None)
    q = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4), "p90_ms": round(float(np.percentile(x, 90)), 4)}
    row = {key: {k: q(v) for k, v in t.items()} for key, t in ts.items()}
    row["pixels_with_surface_point"] = round(float((rec[:, 3] != 0).mean()), 4)
    row["pixels_blocked"] = round(float((rec[:, 3] == 2).mean()), 4)
    row["frame_on_minus_off_ms"] = round(row["on"]["frame"]["median_ms"] - row["off"]["frame"]["median_ms"], 4)
    out["modes"]["Shade"] = row
    print(f"frame off {row['off']['frame']['median_ms']:.4f} ms, on {row['on']['frame']['median_ms']:.4f} ms (mesh shadow kernel {row['on']['mesh_shadow_kernel']['median_ms']:.4f} ms, "
          f"NeRF pass off {row['off']['nerf_pass']['median_ms']:.4f} / on {row['on']['nerf_pass']['median_ms']:.4f} ms), owners {row['pixels_with_surface_point']}, blocked {row['pixels_blocked']}", flush=True)
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


def main_mesh_materials(args, ctx, native, cam, geo, out):
    out["how"] = ("Shade-mode Geometry frames of the meshes over the benchmark's model, no mesh owning a material (off: render_mesh_fused) and every mesh owning one (on: "
                  "render_mesh_fused_materials, ngp_set_mesh_material) in alternating calls of one run. frame: HIP events around the whole frame (ngp_get_render_stats "
                  "frame_ms); mesh_pass: ngp_get_mesh_pass_ms, with materials the id plane's memset included. Medians of --frames frames each after --warmup, with p10 / p90. "
                  "Nothing is asserted on them.")
    opts = native.make_opts(render_mode=native.RENDER_SHADE, **geo)
    materials = [dict(basecolor=(0.6, 0.6, 0.65), metallic=0.9, roughness=0.2, ambientcolor=(0.3, 0.2, 0.1)),
                 dict(basecolor=(0.9, 0.15, 0.1), roughness=0.8, specular=0.5, ambientcolor=(0.3, 0.2, 0.1))]
    ts = {key: {"frame": [], "mesh_pass": []} for key in ("off", "on")}
    for i in range(args.warmup + args.frames):
        for key in ("off", "on"):
            for m in range(ctx.n_meshes()):
                ctx.set_mesh_material(m, materials[m % len(materials)] if key == "on" else None)
            ctx.render(cam, opts)
            if i >= args.warmup:
                ts[key]["frame"].append(ctx.render_stats()["frame_ms"])
                ts[key]["mesh_pass"].append(ctx.mesh_pass_ms())
    ids = ctx.frame_mesh_ids(args.width * args.height)  # (the last call was an on frame)
    q = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4), "p90_ms": round(float(np.percentile(x, 90)), 4)}
    row = {key: {k: q(v) for k, v in t.items()} for key, t in ts.items()}
    row["pixels_with_a_mesh"] = round(float((ids >= 0).mean()), 4)
    row["mesh_pass_on_minus_off_ms"] = round(row["on"]["mesh_pass"]["median_ms"] - row["off"]["mesh_pass"]["median_ms"], 4)
    out["modes"]["Shade"] = row
    print(f"mesh pass off {row['off']['mesh_pass']['median_ms']:.4f} ms, on {row['on']['mesh_pass']['median_ms']:.4f} ms; frame off {row['off']['frame']['median_ms']:.4f} ms, "
          f"on {row['on']['frame']['median_ms']:.4f} ms; pixels with a mesh {row['pixels_with_a_mesh']}", flush=True)
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


def main_sun_disk(args, ctx, native, cam, geo, out):
    out["how"] = ("Shade-mode Geometry frames with ngp_set_mesh_shadow_on_nerf at its defaults, the sun's disk (ngp_set_sun_disk: the real sun's 0.00465 rad and 5 degrees, "
                  "--sun-disk-rays rays) off, on with a pixel's rays dealt over adjacent lanes of the wave (wave) and on with one thread a pixel looping over its rays "
                  "(thread, NGP_SUN_DISK_LAYOUT=thread), in alternating calls of one run. frame: HIP events around the whole frame (ngp_get_render_stats frame_ms); mesh_pass: "
                  "ngp_get_mesh_pass_ms (with the disk on the split pass: G-buffer, disk kernel, deferred shade); sun_disk_kernel: ngp_get_frame_sun_disk_ms; "
                  "mesh_shadow_kernel: ngp_get_frame_mesh_shadow_ms (nerf_mesh_shadow_kernel, or nerf_mesh_soft_shadow_kernel with the disk). Medians of --frames frames "
                  "each after --warmup, with p10 / p90. Nothing is asserted on these.")
    out["n_rays"] = args.sun_disk_rays
    opts = native.make_opts(render_mode=native.RENDER_SHADE, **geo)
    n = args.width * args.height
    q = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4), "p90_ms": round(float(np.percentile(x, 90)), 4)}
    ctx.set_mesh_shadow_on_nerf(True)
    for name, radius in (("real_sun", 0.00465), ("five_degrees", 0.0872665)):
        keys = ("off", "wave", "thread")
        ts = {key: {"frame": [], "mesh_pass": [], "sun_disk_kernel": [], "mesh_shadow_kernel": []} for key in keys}
        recs = {}
        for i in range(args.warmup + args.frames):
            for key in keys:
                os.environ["NGP_SUN_DISK_LAYOUT"] = "thread" if key == "thread" else "wave"
                ctx.set_sun_disk(None if key == "off" else dict(angular_radius=radius, n_rays=args.sun_disk_rays))
                ctx.render(cam, opts)
                if i >= args.warmup:
                    ts[key]["frame"].append(ctx.render_stats()["frame_ms"])
                    ts[key]["mesh_pass"].append(ctx.mesh_pass_ms())
                    ts[key]["mesh_shadow_kernel"].append(ctx.frame_mesh_shadow_ms())
                    if key != "off":
                        ts[key]["sun_disk_kernel"].append(ctx.frame_sun_disk_ms())
                if i == args.warmup + args.frames - 1 and key != "off":
                    recs[key] = (ctx.frame_sun_disk(n), ctx.frame_mesh_shadow(n))
        row = {key: {k: q(v) for k, v in t.items() if v} for key, t in ts.items()}
        disk, nerf = recs["wave"]
        count = np.where(disk[:, 3] != 0, disk[:, 3] - 1, 0)
        row["layouts_give_equal_records"] = bool(disk.tobytes() == recs["thread"][0].tobytes() and nerf.tobytes() == recs["thread"][1].tobytes())
        row["mesh_pixels_with_disk"] = round(float((disk[:, 3] != 0).mean()), 4)
        row["mesh_pixels_partial"] = round(float(((count > 0) & (count < args.sun_disk_rays)).mean()), 4)
        row["mesh_pixels_full"] = round(float((count == args.sun_disk_rays).mean()), 4)
        row["nerf_pixels_with_surface_point"] = round(float((nerf[:, 3] != 0).mean()), 4)
        row["nerf_pixels_partial"] = round(float(((nerf[:, 3] > 1) & (nerf[:, 3] < 2)).mean()), 4)
        row["nerf_pixels_full"] = round(float((nerf[:, 3] == 2).mean()), 4)
        for key in ("wave", "thread"):
            row["frame_%s_minus_off_ms" % key] = round(row[key]["frame"]["median_ms"] - row["off"]["frame"]["median_ms"], 4)
        out["modes"][name] = row
        print(f"{name}: frame off {row['off']['frame']['median_ms']:.4f} ms, wave {row['wave']['frame']['median_ms']:.4f} ms, thread {row['thread']['frame']['median_ms']:.4f} ms; disk kernel "
              f"wave {row['wave']['sun_disk_kernel']['median_ms']:.4f} / thread {row['thread']['sun_disk_kernel']['median_ms']:.4f} ms; NeRF shadow kernel off {row['off']['mesh_shadow_kernel']['median_ms']:.4f} / "
              f"wave {row['wave']['mesh_shadow_kernel']['median_ms']:.4f} / thread {row['thread']['mesh_shadow_kernel']['median_ms']:.4f} ms; equal records {row['layouts_give_equal_records']}", flush=True)
    os.environ.pop("NGP_SUN_DISK_LAYOUT", None)
    ctx.set_sun_disk(None)
    ctx.set_mesh_shadow_on_nerf(None)
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


def main_ambient_change_on_nerf(args, ctx, native, synthetic, cam, geo, lo, hi, out):
    out["how"] = ("Shade-mode Geometry frames, the option off and on (ngp_set_ambient_change_on_nerf, min_irradiance 1e-3, max_gain 4) in alternating calls of one run, per view. "
                  "frame: HIP events around the whole frame (ngp_get_render_stats frame_ms); nerf_pass: its NeRF launch (kernel_ms); mesh_pass: ngp_get_mesh_pass_ms; "
                  "ambient_kernels: HIP events around nerf_surface_normals_kernel and nerf_ambient_ratio_kernel (ngp_get_frame_ambient_change_ms). "
                  "Medians of --frames frames each after --warmup, with p10 / p90. Volumes: 8^3 probes over the scene box, 16 x 16 rays; the context's sunlit with one bounce.")
    # the second view: the model alone over a far floor, seen from close by, so that the NeRF fills the frame
    fill = native.Context(0)
    fill.set_model(synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19))
    fill.add_mesh((scene()[0][0] * np.float32([8.0, 0.05, 8.0])).astype(np.float32), (0.5, -3.0, 0.5))
    fill.set_geometry_opts(ambientcolor=(0.3, 0.2, 0.1))
    flo, fhi = fill.mesh_info(-1)["aabb"]
    fill_cam = native.make_camera(look_at((0.5, 0.9, -0.8), (0.5, 0.45, 0.5), up=(0.0, 1.0, 0.0)), args.width, args.height, (0.9 * args.width,) * 2)
    opts = native.make_opts(render_mode=native.RENDER_SHADE, **geo)
    q = lambda x: {"median_ms": round(float(np.median(x)), 4), "min_ms": round(float(np.min(x)), 4), "p10_ms": round(float(np.percentile(x, 10)), 4), "p90_ms": round(float(np.percentile(x, 90)), 4)}
    for name, c, view, box in (("meshes_view", ctx, cam, (lo, hi)), ("nerf_fills_the_frame", fill, fill_cam, (flo, fhi))):
        c.compute_irradiance_volume((8,) * 3, box, 16, 16, bounces=1, sun=dict(direction=(1.0, 1.0, 1.0)))
        c.compute_reference_irradiance_volume((8,) * 3, box, 16, 16)
        ts = {key: {"frame": [], "nerf_pass": [], "mesh_pass": [], "ambient_kernels": []} for key in ("off", "on")}
        for i in range(args.warmup + args.frames):
            for key, change in (("off", None), ("on", True)):
                c.set_ambient_change_on_nerf(change)
                c.render(view, opts)
                if i >= args.warmup:
                    st = c.render_stats()
                    ts[key]["frame"].append(st["frame_ms"])
                    ts[key]["nerf_pass"].append(st["kernel_ms"])
                    ts[key]["mesh_pass"].append(c.mesh_pass_ms())
                    ts[key]["ambient_kernels"].append(c.frame_ambient_change_ms())
        rec = c.frame_ambient_change(args.width * args.height)  # (the last call was an on frame)
        c.set_ambient_change_on_nerf(None)
        row = {key: {k: q(v) for k, v in t.items()} for key, t in ts.items()}
        owner = rec[:, 3] != 0
        row["pixels_with_surface_point"] = round(float(owner.mean()), 4)
        row["pixels_scaled"] = round(float((rec[:, 3] == 2).mean()), 4)
        row["g_min_max"] = [round(float(rec[owner, 8:11].min()), 4), round(float(rec[owner, 8:11].max()), 4)] if owner.any() else None
        row["frame_on_minus_off_ms"] = round(row["on"]["frame"]["median_ms"] - row["off"]["frame"]["median_ms"], 4)
        out["modes"][name] = row
        print(f"{name}: frame off {row['off']['frame']['median_ms']:.4f} ms, on {row['on']['frame']['median_ms']:.4f} ms (ambient kernels {row['on']['ambient_kernels']['median_ms']:.4f} ms, "
              f"NeRF pass off {row['off']['nerf_pass']['median_ms']:.4f} / on {row['on']['nerf_pass']['median_ms']:.4f} ms), owners {row['pixels_with_surface_point']}, "
              f"scaled {row['pixels_scaled']}, g {row['g_min_max']}", flush=True)
    print(json.dumps(out))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    fill.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--visibility", action="store_true", help="the visibility-weighted volume against Shade and the plain volume, and the maps' compute time")
    ap.add_argument("--sun-nerf-shadow", action="store_true", help="the mesh pass with the NeRF in front of the frames' sun, off and on, per shade mode")
    ap.add_argument("--mesh-shadow-on-nerf", action="store_true", help="Shade frames with the meshes' shadow on the NeRF, off and on in alternating calls")
    ap.add_argument("--ambient-change-on-nerf", action="store_true", help="Shade frames with the meshes' change of the ambient light on the NeRF, off and on in alternating calls, in two views")
    ap.add_argument("--mesh-reflection", action="store_true", help="the mesh pass with the NeRF mirrored in the meshes, off and on, per shade mode")
    ap.add_argument("--mesh-reflection-meshes", action="store_true", help="the mesh reflection with the meshes in it, off and on, per shade mode, in two views")
    ap.add_argument("--mesh-materials", action="store_true", help="Shade frames with no mesh and with every mesh owning a material, in alternating calls")
    ap.add_argument("--sun-disk", action="store_true", help="Shade frames with the sun's disk off and on, both kernel layouts, in alternating calls")
    ap.add_argument("--sun-disk-rays", type=int, default=16, help="with --sun-disk: shadow rays a pixel (1, 2, 4, 8 or 16)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mesh_materials_rate.json" if args.mesh_materials else "sun_disk_rate.json" if args.sun_disk else "mesh_reflection_meshes_rate.json" if args.mesh_reflection_meshes else "mesh_reflection_rate.json" if args.mesh_reflection else "ambient_change_on_nerf_rate.json" if args.ambient_change_on_nerf else "mesh_shadow_on_nerf_rate.json" if args.mesh_shadow_on_nerf else "mesh_shade_sun_shadow_rate.json" if args.sun_nerf_shadow else "mesh_shade_visibility_rate.json" if args.visibility else "mesh_shade_rate.json")
    if args.frames < 20:
        raise SystemExit("--frames: at least 20")
    pkg("build").build()
    native, synthetic = pkg("native"), pkg("synthetic")
    meshes = scene()
    ctx = native.Context(0)  # the benchmark's model (bench.py): what the tables and the volumes are traced in
    ctx.set_model(synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19))
    for tris, center in meshes:
        ctx.add_mesh(tris, center)
    info = ctx.mesh_info(-1)
    lo, hi = info["aabb"]
    # the same view as the mesh tests' frames, the focal length scaled to the frame
    cam = native.make_camera(look_at((0.93, 6.3, 0.57), (1.0, 0.5, 0.5)), args.width, args.height, (100.0 * args.width / 64.0,) * 2)
    geo = dict(testbed_mode=native.MODE_GEOMETRY, background=(0, 0, 0, 0))
    out = {"how": "device time of the mesh pass (render_mesh_fused) per Geometry-mode frame, HIP events around its launch (ngp_get_mesh_pass_ms), "
                  "median (and minimum) of --frames frames after --warmup; ratio = median / the Shade median of the same run",
           "width": args.width, "height": args.height, "frames": args.frames, "triangles": int(info["n_tris"]), "modes": {}}
    ctx.set_geometry_opts(ambientcolor=(0.3, 0.2, 0.1))
    if args.mesh_materials:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return main_mesh_materials(args, ctx, native, cam, geo, out)
    if args.sun_disk:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return main_sun_disk(args, ctx, native, cam, geo, out)
    if args.sun_nerf_shadow:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return main_sun_nerf_shadow(args, ctx, native, cam, geo, lo, hi, out)
    if args.mesh_reflection_meshes:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return main_mesh_reflection_meshes(args, ctx, native, synthetic, cam, geo, lo, hi, out)
    if args.mesh_reflection:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return main_mesh_reflection(args, ctx, native, cam, geo, lo, hi, out)
    if args.mesh_shadow_on_nerf:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return main_mesh_shadow_on_nerf(args, ctx, native, cam, geo, out)
    if args.ambient_change_on_nerf:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return main_ambient_change_on_nerf(args, ctx, native, synthetic, cam, geo, lo, hi, out)
    rows = [("Shade", native.RENDER_SHADE, None), ("ShadeGridEnvMap", native.RENDER_SHADE_GRID_ENVMAP, "grid")]
    rows += [("ShadeIrradianceVolume_%d" % r, native.RENDER_SHADE_IRRADIANCE_VOLUME, r) for r in (8, 32)]
    if args.visibility:  # one run: Shade, then per resolution the plain volume and the same volume with visibility
        rows = [rows[0]] + [row for r in (8, 32) for row in (("ShadeIrradianceVolume_%d" % r, native.RENDER_SHADE_IRRADIANCE_VOLUME, r),
                                                             ("ShadeIrradianceVolumeVisible_%d" % r, native.RENDER_SHADE_IRRADIANCE_VOLUME, -r))]
    for name, mode, what in rows:
        if what == "grid":  # the reference's default grid: 8 x 8 probes of 64 x 32 texels
            ctx.compute_envmap_grid(8, 8, 64, 32)
        elif what is not None and what > 0:  # over the scene box, meshes occluding: the probes inside the closed meshes are dead
            ctx.compute_irradiance_volume((what,) * 3, (lo, hi), 16, 16)
        elif what is not None:  # the volume of the row before, with distance maps
            ctx.compute_irradiance_volume_visibility(16, 16, 5)
        med, mn, cover, p10, p90 = median_ms(ctx, cam, native.make_opts(render_mode=mode, **geo), args.frames, args.warmup)
        out["modes"][name] = {"median_ms": round(med, 4), "min_ms": round(mn, 4), "p10_ms": round(p10, 4), "p90_ms": round(p90, 4), "pixels_with_depth": round(cover, 3)}
        if isinstance(what, int) and what > 0:
            out["modes"][name]["dead_probes"] = round(float((ctx.get_irradiance_volume()[1][..., 27] == 0).mean()), 4)
        print(f"{name:28s} median {med:.4f} ms  min {mn:.4f} ms", flush=True)
    base = out["modes"]["Shade"]["median_ms"]
    for m in out["modes"].values():
        m["ratio_to_shade"] = round(m["median_ms"] / base, 3)
    if args.visibility:
        import time

        for r in (8, 32):
            out["modes"]["ShadeIrradianceVolumeVisible_%d" % r]["ratio_to_plain_volume"] = round(
                out["modes"]["ShadeIrradianceVolumeVisible_%d" % r]["median_ms"] / out["modes"]["ShadeIrradianceVolume_%d" % r]["median_ms"], 3)
        # the maps' compute: 16^3 probes x 16 x 16 rays against the BVHs, wall time of the whole call (it ends synchronised). The device time
        # is not measured: the call has no timing entry.
        ctx.compute_irradiance_volume((16,) * 3, (lo, hi), 8, 8)
        ts = []
        for i in range(2 + 7):
            t0 = time.perf_counter()
            ctx.compute_irradiance_volume_visibility(16, 16, 5)
            if i >= 2:
                ts.append(1e3 * (time.perf_counter() - t0))
        out["visibility_compute_16x16x16_probes_16x16_rays"] = {"wall_median_ms": round(float(np.median(ts)), 3), "wall_min_ms": round(min(ts), 3), "wall_max_ms": round(max(ts), 3),
                                                                 "runs": len(ts), "warmup": 2, "device_ms": None}
        print("visibility compute, 16^3 probes x 256 rays: wall median %.3f ms (min %.3f, max %.3f)" % (np.median(ts), min(ts), max(ts)), flush=True)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
