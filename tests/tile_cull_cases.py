"""What the tile-cull tests share (tests/test_tile_cull_cpu.py, tests/test_tile_cull_gpu.py): occupancies as 128^3 cell arrays, cameras, and
the CPU model of the cull -- tests/aux/tile_probe_check.cpp, which runs csrc/tile_probe.h on the host for every tile of a pinhole frame and
traverses every ray of a culled tile through the grid in float64."""
import os
import struct
import subprocess

import numpy as np

from conftest import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 128
FOV_BENCH = 0.6911
BENCH_AZIMUTHS = [0.0, 45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0]
NEAR4_WORDS, NEAR2_WORDS = 1024, 8192


def bench_occupancy():
    """occ[x, y, z] of the benchmark's model (synthetic.make_scene(aabb_scale=1): every seed and table size has this density grid)"""
    scene = pkg("scene")
    grid = pkg("synthetic").make_density_grid(1)
    idx = np.arange(G, dtype=np.uint32)
    X, Y, Z = np.meshgrid(idx, idx, idx, indexing="ij")
    return (grid[scene.morton3d(X.ravel(), Y.ravel(), Z.ravel())] > 0.01).reshape(G, G, G)


def structured_occupancies():
    out = {}
    o = np.zeros((G, G, G), bool)
    o[77, 31, 64] = True
    out["single_cell"] = o
    o = np.zeros((G, G, G), bool)
    o[10:118, 63, 20:100] = True  # one cell thick
    out["thin_plate"] = o
    c = (np.indices((G, G, G)).astype(np.float64) + 0.5) / G - 0.5
    r = np.sqrt((c ** 2).sum(0))
    out["shell"] = (r > 0.30) & (r < 0.315)
    o = np.zeros((G, G, G), bool)
    o[0, :, :] = True  # the face whose cells also answer for (-1/128, 0)
    o[:, 127, :] = True
    out["faces"] = o
    return out


def random_occupancy(seed, density):
    return np.random.default_rng(seed).random((G, G, G)) < density


def camera(az, el=30.0, radius=4.03, w=256, h=144, fov_x=FOV_BENCH, look_at=(0.5, 0.5, 0.5), away=False):
    """(3 x 4 matrix, w, h, focal) of an orbit camera around look_at; radius 0.5 puts it inside the unit cube; away: turned by 180 degrees"""
    scene = pkg("scene")
    mat = np.array(scene.orbit_camera(az, el, radius, offset=look_at), np.float32)
    if away:
        mat[:, 0] *= -1.0
        mat[:, 2] *= -1.0
    return mat, w, h, scene.focal_from_fov_x(w, fov_x)


# the frames of tests/test_tile_cull_gpu.py that the CPU model is asked about: name -> camera. Narrow frames have the benchmark's pixel
# footprint (fov_x 0.09 rad over 256 pixels, 0.6911 over 1920) and look past the object's edge, so that some tiles go and some stay.
EDGE = (0.5, 0.2, 0.5)  # (the CPU model: 256 of the 576 tiles of "narrow" go)


def gpu_cameras():
    return {
        "narrow": camera(45.0, w=256, h=144, fov_x=0.09, look_at=EDGE),
        "narrow_odd": camera(45.0, w=250, h=140, fov_x=0.09, look_at=EDGE),
        "inside": camera(20.0, 10.0, 0.5, 256, 144),
        "wide": camera(45.0, 30.0, 0.9, 256, 144, 2.4),  # (8 pixels span more than 4 cells: the bound keeps every tile)
        "away": camera(45.0, w=256, h=144, fov_x=0.09, away=True),
    }


def build_check(tmp_dir, sanitize=True):
    exe = os.path.join(str(tmp_dir), "tile_probe_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I", os.path.join(ROOT, pkg("build").CSRC), os.path.join(ROOT, "tests", "aux", "tile_probe_check.cpp"), "-o", exe])
    return exe


def run_check(exe, tmp_dir, occ, cams, tag="case"):
    """-> (near4 words, near2 words, [(decision bytes per tile, false culls) per camera])"""
    fin, fout = os.path.join(str(tmp_dir), tag + ".in"), os.path.join(str(tmp_dir), tag + ".out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cams)))
        f.write(np.ascontiguousarray(occ.transpose(2, 1, 0)).astype(np.uint8).tobytes())  # x fastest
        for mat, w, h, focal in cams:
            f.write(np.asarray(mat, np.float32).T.astype("<f4").tobytes())  # column by column
            f.write(struct.pack("<iiff", w, h, focal[0], focal[1]))
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    near = np.frombuffer(raw, "<u4", NEAR4_WORDS + NEAR2_WORDS)
    pos = 4 * (NEAR4_WORDS + NEAR2_WORDS)
    res = []
    for _ in cams:
        n_tiles, false_culls = struct.unpack_from("<II", raw, pos)
        res.append((np.frombuffer(raw, np.uint8, n_tiles, pos + 8), false_culls))
        pos += 8 + n_tiles
    assert pos == len(raw)
    os.remove(fin)
    os.remove(fout)
    return near[:NEAR4_WORDS], near[NEAR4_WORDS:], res


def near_bool_numpy(occ, g):
    """dil[bx, by, bz]: some g^3 block in the 3 x 3 x 3 neighbourhood of the block holds an occupied cell"""
    n = G // g
    blocks = occ.reshape(n, g, n, g, n, g).any(axis=(1, 3, 5))
    pad = np.pad(blocks, 1)
    dil = np.zeros_like(blocks)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                dil |= pad[dx:dx + n, dy:dy + n, dz:dz + n]
    return dil


def near_table_numpy(occ, g):
    """the dilated table of tile_probe.h from numpy: words of 32 blocks along x, then y, then z"""
    bits = near_bool_numpy(occ, g).transpose(2, 1, 0).reshape(-1, 32).astype(np.uint64)  # [z][y][x], 32 x a word
    return (bits << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def probe_numpy(occ, cam, band=1e-5):
    """The tile probe restated in float64 numpy, from the text of csrc/tile_probe.h and not from its code, for every tile of a pinhole frame.
    -> (decision per tile as tile_probe_check writes it: 0 kept, 1 no ray reaches the cube, 2 / 4 culled at that granularity;
        ambiguous per tile: some comparison on the way is within `band` of its threshold, or a probe point within `band` of a block face
        decides the lookup -- there fp32 and float64 may disagree, everywhere else they must not).
    band: the header's fp32 quantities (o + d t, the clips, r) carry ~1e-6 for |t| <= 4; 1e-5 is ten times that."""
    mat, W, H, focal = cam
    m = np.asarray(mat, np.float32).astype(np.float64)
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    T = tiles_x * tiles_y
    lane = np.arange(64)
    s4, i16 = lane >> 4, lane & 15
    slot = ((s4 >> 1) * 4 + (i16 >> 2)) * 8 + (s4 & 1) * 4 + (i16 & 3)  # lane -> pixel of the tile, as the kernel deals the four strips
    tile = np.arange(T)[:, None]
    x = (tile % tiles_x) * 8 + (slot & 7)[None, :]
    y = (tile // tiles_x) * 8 + (slot >> 3)[None, :]
    valid = (x < W) & (y < H)
    cx = ((x + 0.5) / W - 0.5) * W / np.float64(np.float32(focal[0]))
    cy = ((y + 0.5) / H - 0.5) * H / np.float64(np.float32(focal[1]))
    d = m[:, 0] * cx[..., None] + m[:, 1] * cy[..., None] + m[:, 2]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(m[:, 3], d.shape)
    amb = np.zeros(T, bool)

    def slab(lo, hi, t_from):
        with np.errstate(divide="ignore", invalid="ignore"):
            a, b = (lo - o) / d, (hi - o) / d
        par = d == 0.0
        inside = (o >= lo) & (o <= hi)
        near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(a, b))
        far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(a, b))
        return np.maximum(near.max(-1), t_from), far.min(-1)

    eps, cell = 1.0 / 1024.0, 1.0 / 128.0
    bn, bf = slab(0.0, 1.0, 0.0)  # the render box: the unit cube
    alive = valid & (bn < bf)
    amb |= (valid & (np.abs(bf - bn) < band)).any(1)
    t0 = bn + 1e-6
    lo, hi = -(cell + eps), 1.0 + eps
    tn, tf = slab(lo, hi, t0)
    inn = alive & (tn <= tf)
    amb |= (alive & (np.abs(tf - tn) < band)).any(1)
    Tn_all, Tf_all = slab(lo - 4 * cell, hi + 4 * cell, 0.0)
    Tn, Tf = Tn_all[:, 15], Tf_all[:, 15]
    decision = np.zeros(T, np.uint8)
    none = ~inn.any(1)
    decision[none] = 1
    live = ~none & inn[:, 15]
    contained = ((tn >= Tn[:, None]) & (tf <= Tf[:, None])) | ~inn
    amb |= live & (inn & (((np.abs(tn - Tn[:, None]) < band) & (Tn[:, None] > 0.0)) | (np.abs(tf - Tf[:, None]) < band))).any(1)  # (T_n = 0 is the clip itself: exact, and every t0 is above it)
    live &= contained.all(1)
    oa, da = o[:, 15], d[:, 15]
    D = np.zeros(T)
    for te in (Tn, Tf):
        te = np.where(live, te, 0.0)
        dev = np.abs((o + d * te[:, None, None]) - (oa + da * te[:, None])[:, None, :]).max(-1)
        D = np.maximum(D, np.where(inn, dev, 0.0).max(1))
    length = np.where(live, Tf - Tn, 0.0)
    r128, r64 = D + length / 256.0 + eps, D + length / 128.0 + eps
    g = np.where(r128 <= 2 * cell, 2, np.where(r128 <= 4 * cell, 4, 0))
    amb |= live & ((np.abs(r128 - 2 * cell) < band) | (np.abs(r128 - 4 * cell) < band))
    n = np.where(r64 <= g * cell, 64, 128)
    amb |= live & (g != 0) & (np.abs(r64 - g * cell) < band)
    live &= g != 0
    k = np.arange(128)[None, :]
    t = np.where(live, Tn, 0.0)[:, None] + (k + 0.5) * (length / n)[:, None]
    q = oa[:, None, :] + da[:, None, :] * t[..., None]  # [tile][point][3]
    used = k < n[:, None]
    sure = np.zeros(T, bool)   # a point is in a set bit wherever within `band` of it one looks
    maybe = np.zeros(T, bool)  # a point is within `band` of a set bit
    for gg in (2, 4):
        dil, side = near_bool_numpy(occ, gg), G // gg
        all_set = np.ones(q.shape[:2], bool)
        any_set = np.zeros(q.shape[:2], bool)
        for sx in (-band, band):
            for sy in (-band, band):
                for sz in (-band, band):
                    b = np.floor((q + np.array([sx, sy, sz])) * side)
                    far = ((b < -2) | (b > side)).any(-1)  # too far from the grid to matter
                    b = np.clip(b, 0, side - 1).astype(np.int64)
                    hit = dil[b[..., 0], b[..., 1], b[..., 2]] & ~far
                    all_set &= hit
                    any_set |= hit
        sel = live & (g == gg)
        sure |= sel & (all_set & used).any(1)
        maybe |= sel & (any_set & used).any(1)
    amb |= live & (sure != maybe)
    decision[live & ~maybe] = g[live & ~maybe]
    return decision, amb
