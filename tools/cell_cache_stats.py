"""Hit rates of the fused render kernel's per-wave cell cache (csrc/nerf_device.h encode_issue_cached), counted before it was built and
kept to size it again: a library built with -DNGP_EXPERIMENT_CELL_CACHE_STATS runs the shipped kernels WITHOUT the cache, keeps only
the tags such a cache would hold (4, 8 and 16 sets per coarse level; looked up when a pass issues its gathers, filled when they have
landed, as the cache does) and counts lane-lookups and hits per level. One 1080p bench frame per azimuth.

    python tools/cell_cache_stats.py [library] > profiles/cell_cache_hit_rates.txt
builds libngp_hip_cellstats.so (build.py: build(cellstats=True)) if no library is named.
"""
import importlib, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "surface-irradiance-estimation-from-neural-radiance-fields_amd"


def child():
    sys.path.insert(0, ROOT)
    import torch
    import bench

    native, synthetic, scene = (importlib.import_module(PKG + "." + m) for m in ("native", "synthetic", "scene"))
    torch.zeros(1, device="cuda")
    ctx = native.Context(0)
    ctx.set_model(synthetic.make_scene(aabb_scale=1, seed=1234, log2_hashmap_size=19))
    w, h = bench.WIDTH, bench.HEIGHT
    rgba, depth = torch.zeros((h, w, 4), device="cuda"), torch.zeros((h, w), device="cuda")
    n_samples = 0
    for az in bench.AZIMUTHS:
        ctx.render_device(native.make_camera(scene.orbit_camera(az), w, h, scene.focal_from_fov_x(w, bench.FOV_X)), native.make_opts(), rgba.data_ptr(), depth.data_ptr(), 0)
        torch.cuda.synchronize()
        n_samples += ctx.render_stats()["n_samples"]  # (prints the running totals on stderr; the last print is the one that counts)
    print(f"n_samples {n_samples}")
    ctx.close()


def main():
    sys.path.insert(0, ROOT)
    lib = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else importlib.import_module(PKG + ".build").build(cellstats=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, NGP_HIP_LIBRARY=lib), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(r.stdout + r.stderr)
    rows = {}
    for m in re.finditer(r"\[ngp cell cache\] level (\d) lookups (\d+) hits with 4 / 8 / 16 sets (\d+) (\d+) (\d+)", r.stderr):
        rows[int(m.group(1))] = [int(v) for v in m.groups()[1:]]
    if len(rows) != 4 or not all(v[0] for v in rows.values()):
        sys.exit("no counts: is %s built with -DNGP_EXPERIMENT_CELL_CACHE_STATS?\n%s" % (lib, r.stderr[-2000:]))
    n_samples = int(re.search(r"n_samples (\d+)", r.stdout).group(1))
    print(f"# tools/cell_cache_stats.py: 1920x1080, bench model, one frame per azimuth ({n_samples} samples composited); lane-lookups of the coarse level")
    print("# of every network pass (idle lanes of a last pass included, as they gather too) against per-wave direct-mapped tags, cell_cache.h cell_set")
    print("# level  lane-lookups  miss fraction with 4 / 8 / 16 sets per level")
    tot = [0, 0, 0, 0]
    for l in range(4):
        n, hits = rows[l][0], rows[l][1:]
        print(f"  {l}  {n:13d}  " + "  ".join(f"{1.0 - x / n:.4f}" for x in hits))
        tot = [a + b for a, b in zip(tot, rows[l])]
    print("  all  %11d  " % tot[0] + "  ".join(f"{1.0 - x / tot[0]:.4f}" for x in tot[1:]))
    print("# bytes of LDS per wave (64 B line + 4 B tag per set, 4 levels): " + " / ".join(str(4 * s * 68) for s in (4, 8, 16)))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
