"""The tile cull's bound on the host (csrc/tile_probe.h through tests/aux/tile_probe_check.cpp, built and run under AddressSanitizer and
UBSan): the dilated tables against numpy, no tile called empty whose rays meet an occupied cell (a condition: the allowed count is 0), and
enough tiles called empty on the benchmark's frames to be worth the test (at least 25 %)."""
import numpy as np
import pytest

import tile_cull_cases as T


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_probe")
    return T.build_check(d), d


@pytest.fixture(scope="module")
def check_fast(tmp_path_factory):
    """the same program without the sanitizers, for the 16.6 M rays of the 1080p frames"""
    d = tmp_path_factory.mktemp("tile_probe_fast")
    return T.build_check(d, sanitize=False), d


def small_cameras():
    """inside and outside the cube, narrow and wide, sizes that are and are not a multiple of 8"""
    return [T.camera(45.0), T.camera(200.0, 10.0, 4.03, 250, 140), T.camera(100.0, 60.0, 2.0, 256, 144, 0.09), T.camera(20.0, 10.0, 0.5, 256, 144),
            T.camera(300.0, -20.0, 0.5, 250, 140, 2.0), T.camera(135.0, 30.0, 1.2, 256, 144, 2.4), T.camera(270.0, 5.0, 8.0, 123, 77, 0.2),
            T.camera(10.0, 85.0, 1.6, 64, 40, 1.0)]


def test_near_tables_match_numpy(check):
    exe, d = check
    for name, occ in (("bench", T.bench_occupancy()), ("random", T.random_occupancy(5, 2e-3)), ("faces", T.structured_occupancies()["faces"])):
        near4, near2, _ = T.run_check(exe, d, occ, [], name)
        assert np.array_equal(near4, T.near_table_numpy(occ, 4)), name
        assert np.array_equal(near2, T.near_table_numpy(occ, 2)), name
        assert near2.any() and (name != "bench" or (near4 == 0).any())  # (tables of something; the benchmark's has empty regions)


def test_no_false_culls_small_frames(check):
    exe, d = check
    occs = dict(T.structured_occupancies(), bench=T.bench_occupancy(), sparse=T.random_occupancy(11, 1e-4), denser=T.random_occupancy(12, 3e-3),
                empty=np.zeros((T.G, T.G, T.G), bool))
    culled_any = kept_any = 0
    for name, occ in occs.items():
        _, _, res = T.run_check(exe, d, occ, small_cameras(), name)
        for k, (dec, false_culls) in enumerate(res):
            print(name, k, "tiles", dec.size, "culled", int((dec != 0).sum()), "false culls", false_culls)
            assert false_culls == 0, (name, k)
            culled_any += int((dec != 0).sum())
            kept_any += int((dec == 0).sum())
            if name == "empty" and k == 2:
                assert (dec != 0).all()  # nothing occupied and tiles narrow enough for the bound: every tile goes
    assert culled_any > 0 and kept_any > 0


def test_bench_frames_no_false_culls_and_cull_power(check_fast):
    """The eight benchmark cameras at 1920 x 1080 on the benchmark's occupancy: 0 false culls, and at least 25 % of the tiles culled."""
    exe, d = check_fast
    cams = [T.camera(az, w=1920, h=1080) for az in T.BENCH_AZIMUTHS]
    _, _, res = T.run_check(exe, d, T.bench_occupancy(), cams, "bench1080")
    total = culled = 0
    for az, (dec, false_culls) in zip(T.BENCH_AZIMUTHS, res):
        assert dec.size == 240 * 135
        share = float((dec != 0).mean())
        print("azimuth %5.1f: culled %.1f %% (g = 2: %d, g = 4: %d, no ray in the cube: %d), false culls %d" % (az, 100 * share, (dec == 2).sum(), (dec == 4).sum(), (dec == 1).sum(), false_culls))
        assert false_culls == 0, az
        assert share >= 0.25, az
        total += dec.size
        culled += int((dec != 0).sum())
    assert culled >= 0.25 * total


def test_probe_decisions_match_float64_numpy(check):
    """The header's per-tile decision (kept, no ray in the cube, culled at 2 or 4 cells) against tile_cull_cases.probe_numpy, a float64
    restatement of the bound as the header's text states it: ray ranges, [T_n, T_f], D, g, N, the clamped lookup. Equal on every tile
    outside the band of 1e-5 (ten times the fp32 error of the header's quantities) around the thresholds and the block faces; the tiles
    inside the band are few (at most 3 % of all), so the comparison is of nearly every tile."""
    exe, d = check
    cams = small_cameras() + list(T.gpu_cameras().values())
    total = inside_band = culled = 0
    for name, occ in (("bench", T.bench_occupancy()), ("sparse", T.random_occupancy(11, 1e-4)), ("shell", T.structured_occupancies()["shell"]),
                      ("faces", T.structured_occupancies()["faces"])):
        _, _, res = T.run_check(exe, d, occ, cams, "np_" + name)
        for k, (cam, (dec, _)) in enumerate(zip(cams, res)):
            with np.errstate(all="ignore"):
                ref, amb = T.probe_numpy(occ, cam)
            diff = dec != ref
            print(name, k, "tiles", dec.size, "culled", int((dec != 0).sum()), int((ref != 0).sum()), "differ", int(diff.sum()), "in the band", int(amb.sum()))
            assert not (diff & ~amb).any(), (name, k, np.nonzero(diff & ~amb)[0][:8])
            total += dec.size
            inside_band += int(amb.sum())
            culled += int(((dec != 0) & ~amb).sum())
    assert inside_band <= 0.03 * total, (inside_band, total)
    assert culled > 0.1 * total  # (both kinds of decision are compared)
