#!/bin/bash
# usage: tools/profile_round.sh <tag> [out_dir, default profile_out]   (on an MI355X) -- the evidence bench.py's roofline block cites:
#   1. bench run with --full                     -> <out_dir>/<tag>_bench.json
#   2. rocprofv3 --kernel-trace --stats of a plain run -> <out_dir>/<tag>_kernel_stats.csv
#   3. FETCH_SIZE and WRITE_SIZE in separate --pmc passes (MI355X_MICROARCH.md, HBM section) -> <out_dir>/<tag>_pmc_hbm.json
set -e
tag=$1
out=${2:-profile_out}
export TMPDIR=/tmp && cd "$(dirname "$0")/.."
mkdir -p "$out"
python3 bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err
echo "bench done"
rm -rf $out/prof_$tag && mkdir -p $out/prof_$tag
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -- python3 bench.py > $out/prof_$tag/bench.log 2>&1
cp $out/prof_$tag/*/*kernel_stats.csv $out/${tag}_kernel_stats.csv
echo "kernel trace done"
bash tools/pmc_pass.sh ${tag}_fetch FETCH_SIZE > $out/${tag}_pmc.txt
bash tools/pmc_pass.sh ${tag}_write WRITE_SIZE >> $out/${tag}_pmc.txt
bash tools/pmc_pass.sh ${tag}_compute SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE >> $out/${tag}_pmc.txt
cat $out/${tag}_pmc.txt
python3 - "$tag" "$out" <<'PY'
import json, re, sys
tag, out_dir = sys.argv[1], sys.argv[2]
vals = {}
for line in open(f"{out_dir}/{tag}_pmc.txt"):
    m = re.match(r"\S+ (\w+) mean=([0-9.e+]+) n=(\d+)", line)
    if m:
        vals[m.group(1)] = (float(m.group(2)), int(m.group(3)))
fetch_kb, nf = vals["FETCH_SIZE"]
write_kb, nw = vals["WRITE_SIZE"]
out = {
    "FETCH_SIZE_KB_per_launch": fetch_kb, "FETCH_SIZE_launches": nf,
    "WRITE_SIZE_KB_per_launch": write_kb, "WRITE_SIZE_launches": nw,
    "note": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE in separate passes (bench.py --steps 3 --warmup 1), kernel render_nerf_fused_unit_plain, 1080p. "
            "Counters are in KB; gfx950 reports half of the fetched bytes (MI355X_MICROARCH.md), so read bytes = 2 x FETCH_SIZE. Infinity-Cache hits are included.",
    "traffic_bytes_per_launch_corrected": int((2.0 * fetch_kb + write_kb) * 1024.0),
}
json.dump(out, open(f"{out_dir}/{tag}_pmc_hbm.json", "w"), indent=1)
print(out)
# compute-side utilisation of the same launch: 256 CUs x 4 SIMDs; a wave64 VALU instruction occupies its SIMD for 4 cycles,
# v_mfma_f32_16x16x32_f16 for 16 (SQ_VALU_MFMA_BUSY_CYCLES / SQ_INSTS_MFMA); GRBM_GUI_ACTIVE is summed over the 8 XCDs
if "SQ_INSTS_VALU" in vals:
    cyc = vals["GRBM_GUI_ACTIVE"][0] / 8.0
    simds = 1024.0
    comp = {k: vals[k][0] for k in ("SQ_INSTS_VALU", "SQ_INSTS_MFMA", "SQ_INSTS_SALU", "SQ_INSTS_VMEM_RD", "SQ_INSTS_LDS", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_ACTIVE_INST_VALU", "GRBM_GUI_ACTIVE")}
    comp["kernel_cycles_per_xcd"] = cyc
    comp["valu_issue_utilisation"] = comp["SQ_INSTS_VALU"] * 4.0 / simds / cyc
    comp["mfma_pipe_utilisation"] = comp["SQ_VALU_MFMA_BUSY_CYCLES"] / simds / cyc
    comp["note"] = "per launch of render_nerf_fused_unit_plain at 1080p (bench.py --steps 3 --warmup 1, kernels serialised by the counter collection)"
    json.dump(comp, open(f"{out_dir}/{tag}_pmc_compute.json", "w"), indent=1)
    print(comp)
PY
