#!/usr/bin/env python3
"""Instruction census of one kernel of csrc/nerf_kernels.hip by section, from the gfx950 ISA.

    tools/isa_census.py [kernel name, default render_nerf_fused_unit_plain] [-D...] > profiles/netsec_census.txt
    tools/isa_census.py -DNGP_NETSEC_V1 > profiles/netsec_census_parent.txt

The file is compiled to assembly with -DNGP_CENSUS, which turns every NGP_SECTION("x") of the source into a comment line
"; SECTION x" in the ISA (no instruction). The kernel's text is cut at those lines, in layout order, and every instruction is
counted under the section that was opened last. The compiler still schedules across the comments and lays basic blocks out as it
likes, so a section's count is what was PLACED there -- good to a few instructions at the seams, exact for the kernel as a whole.
A section that the source enters several times (three network passes are instantiated: two of the paired loop, one of the single
pass) sums all of its instances; `n` is how many there are.

Classes: MFMA; VALU (v_* except MFMA); SALU (s_* except s_waitcnt / s_nop and branches); LDS r/w (ds_read* / ds_write* and other
ds_*); VMEM (buffer_*, global_*, flat_*, scratch_*), of which `gather` = buffer_load_dwordx2; waitcnt; branch (s_cbranch*, s_branch).
"""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surface-irradiance-estimation-from-neural-radiance-fields_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "--cuda-device-only", "-S", "-DNGP_CENSUS"]
COLUMNS = ["n", "VALU", "SALU", "MFMA", "LDS r", "LDS w", "VMEM", "gather", "waitcnt", "branch", "all"]


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return ["MFMA"]
    if op.startswith("v_"):
        return ["VALU"]
    if op.startswith("ds_"):
        return ["LDS w" if "write" in op or "store" in op else "LDS r"]
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return ["VMEM", "gather"] if op == "buffer_load_dwordx2" else ["VMEM"]
    if op == "s_waitcnt":
        return ["waitcnt"]
    if op.startswith(("s_cbranch", "s_branch")):
        return ["branch"]
    if op in ("s_nop", "s_endpgm", "s_code_end"):
        return []
    if op.startswith("s_"):
        return ["SALU"]
    return []


def kernel_text(asm, name):
    start = re.search(r"^(_ZN3ngp\d+%s(?=E)\w*):" % re.escape(name), asm, re.M)
    if not start:
        raise SystemExit("kernel %s not found" % name)
    end = asm.index("s_endpgm", start.end())
    return asm[start.end():end]


def census(text):
    counts = collections.OrderedDict()
    cur = "prologue"
    counts[cur] = collections.Counter(n=1)
    for line in text.splitlines():
        m = re.match(r"\s*; SECTION (\S+)", line)
        if m:
            cur = m.group(1)
            counts.setdefault(cur, collections.Counter())["n"] += 1
            continue
        line = line.split(";")[0].strip()
        if not line or line.endswith(":") or line.startswith("."):
            continue
        op = line.split()[0]
        cls = classify(op)
        if cls:
            counts[cur]["all"] += 1
        for k in cls:
            counts[cur][k] += 1
    return counts


def main():
    defines = [a for a in sys.argv[1:] if a.startswith("-D")]
    names = [a for a in sys.argv[1:] if not a.startswith("-")]
    name = names[0] if names else "render_nerf_fused_unit_plain"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + FLAGS + defines + ["nerf_kernels.hip", "-o", "-"], cwd=CSRC, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit("hipcc failed")
    counts = census(kernel_text(r.stdout, name))
    print("# %s %s: instructions placed per section (all instances of a section summed; n = instances)" % (name, " ".join(defines)))
    print("%-18s" % "section" + "".join("%8s" % c for c in COLUMNS))
    total = collections.Counter()
    for sec, cnt in counts.items():
        print("%-18s" % sec + "".join("%8d" % cnt[c] for c in COLUMNS))
        total.update(cnt)
    print("%-18s" % "kernel" + "".join("%8d" % total[c] for c in COLUMNS))
    res = re.search(r"\.vgpr_count:\s*(\d+)", r.stdout[r.stdout.find(".name:           _ZN3ngp%d%sE" % (len(name), name)):] or "")
    if res:
        print("# VGPRs %s" % res.group(1))


if __name__ == "__main__":
    main()
