#!/bin/bash
# K15 (stage 1) counters at 16384^2 x 7: one SQ pass (instruction counts, VALU activity, waits) with --kernel-trace for the
# durations and register counts, in a run of its own, over profiles/preprocess_bench.py --no-chain (uint8, uint16, float32
# DN).  usage: bash profiles/preprocess_pmc.sh <outdir>   -> <outdir>/preprocess_pmc.json
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "$1" && cd "$1" && pwd)
cd /tmp; export TMPDIR=/tmp
B="python3 $R/profiles/preprocess_bench.py --no-chain --reps 3 --warmup 1"
timeout -k 10 600 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_BUSY_CYCLES \
    --kernel-trace -d $O/sq -o s --output-format csv -- $B > /dev/null 2> $O/sq.err || exit $?
s=$(find $O/sq -name "*counter_collection.csv" | head -1); k=$(find $O/sq -name "*kernel_trace.csv" | head -1)
python3 - "$s" "$k" > $O/preprocess_pmc.json <<'PY'
import collections, csv, json, re, sys
short = lambda n: re.sub(r"\(.*$", "", re.sub(r"^void ", "", n))
cnt = collections.defaultdict(lambda: collections.defaultdict(float))
for r in csv.DictReader(open(sys.argv[1])):
    if "k15_" in r["Kernel_Name"]:
        cnt[short(r["Kernel_Name"])][r["Counter_Name"]] += float(r["Counter_Value"])
dur, launches, vgpr = collections.defaultdict(float), collections.Counter(), {}
for r in csv.DictReader(open(sys.argv[2])):
    k = short(r["Kernel_Name"])
    if "k15_" in k:
        dur[k] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        launches[k] += 1
        vgpr[k] = {c: r[c] for c in r if "VGPR" in c or c in ("LDS_Block_Size", "Scratch_Size", "Workgroup_Size", "Grid_Size")}
out = {"about": "rocprofv3 --pmc over profiles/preprocess_bench.py --no-chain at 16384^2 x 7; times are the kernel-trace "
                "durations of this counter pass; VALU busy = 4 * SQ_ACTIVE_INST_VALU / (ms * 2.4 GHz * 1024 SIMDs), "
                "SQ_ACTIVE_INST_VALU being counted in quad-cycles", "kernels": {}}
for k, c in cnt.items():
    w = max(c.get("SQ_WAVES", 0), 1)
    out["kernels"][k] = {"launches": launches[k], "ms_per_launch": dur[k] / max(launches[k], 1), "counters": dict(c),
                         "valu_insts_per_wave": c.get("SQ_INSTS_VALU", 0) / w, "lds_insts_per_wave": c.get("SQ_INSTS_LDS", 0) / w,
                         "valu_busy": 4 * c.get("SQ_ACTIVE_INST_VALU", 0) / (dur[k] * 1e-3 * 2.4e9 * 1024) if dur[k] else None,
                         "wait_inst_any_per_wave_cycle": c.get("SQ_WAIT_INST_ANY", 0) / max(c.get("SQ_WAVE_CYCLES", 1), 1),
                         "resources": vgpr.get(k)}
print(json.dumps(out, indent=1, sort_keys=True))
PY
rm -rf $O/sq
