"""Host-side facts that the trimmed network section of the unit render kernels (csrc/nerf_device.h) rests on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trunc_and_fract_equal_floor_and_subtraction(tmp_path):
    """level_cell_in_cube replaces floorf + float->int + (f - floor) by a truncating conversion and the fractional part. For EVERY
    fp32 f in [0, 4096] (1 166 016 513 values; the largest scale * x + 0.5 in use is far below) both give the same integer and the
    same bits (tests/aux/floor_fract_check.c)."""
    exe = tmp_path / "floor_fract_check"
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-ffp-contract=off", "-o", str(exe), os.path.join(ROOT, "tests", "aux", "floor_fract_check.c"), "-lm"])
    out = subprocess.run([str(exe), "1"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr
    assert out.stderr.split()[0] == str(0x45800000 + 1), out.stderr  # every value of the range was visited
