#!/bin/bash
# K21 (polynomial warp) counters at 16384^2 x 7: one SQ pass (instruction counts, VALU activity, waits) in a run of its own,
# with no tracing beside it, over one warm and one kept round of profiles/warp_bench.py.  The times are not taken here: VALU
# busy is formed with the medians of an unprofiled profiles/warp_bench.json.
# usage: bash profiles/warp_pmc.sh <outdir> [warp_bench.json]   -> <outdir>/warp_pmc.json
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "$1" && cd "$1" && pwd)
J=${2:-$R/profiles/warp_bench.json}; J=$(cd "$(dirname "$J")" && pwd)/$(basename "$J")
cd /tmp; export TMPDIR=/tmp
B="python3 $R/profiles/warp_bench.py --reps 1 --warm 1 --cpu-size 256"
timeout -k 10 600 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_BUSY_CYCLES \
    -d $O/sq -o s --output-format csv -- $B > /dev/null 2> $O/sq.err || exit $?
s=$(find $O/sq -name "*counter_collection.csv" | head -1)
python3 - "$s" "$J" > $O/warp_pmc.json <<'PY'
import collections, csv, json, re, sys
short = lambda n: re.sub(r"\(.*$", "", re.sub(r"^void ", "", n))
cnt = collections.defaultdict(lambda: collections.defaultdict(float))
seen = collections.defaultdict(set)
for r in csv.DictReader(open(sys.argv[1])):
    if "k21_warp" in r["Kernel_Name"] and int(r["Grid_Size"]) > 4096 * 256:     # the 16384^2 launches, not the small ones at the end
        k = short(r["Kernel_Name"])
        cnt[k][r["Counter_Name"]] += float(r["Counter_Value"])
        seen[k].add(r["Dispatch_Id"])
bench = json.load(open(sys.argv[2]))["warp"]
TYPES = {"unsigned char": "uint8", "float": "float32"}
METHODS = ["nearest", "bilinear", "cubic"]
out = {"about": "rocprofv3 --pmc alone over profiles/warp_bench.py --reps 1 --warm 1 at 16384^2 x 7; counters are per launch (both plans "
                "averaged); VALU busy = 4 * SQ_ACTIVE_INST_VALU / (ms * 2.4 GHz * 1024 SIMDs), SQ_ACTIVE_INST_VALU being counted in "
                "quad-cycles, with ms the median of the unprofiled profiles/warp_bench.json", "kernels": {}}
for k, c in sorted(cnt.items()):
    n = max(len(seen[k]), 1)
    c = {name: v / n for name, v in c.items()}
    m = re.match(r"k21_warp<([^,]+), ([^,]+), (\d)>", k)
    ms = None
    if m and m.group(1) in TYPES:
        rows = [v["median_ms"] for name, v in bench.items() if name.startswith(f"{TYPES[m.group(1)]} {METHODS[int(m.group(3))]} ")]
        ms = sum(rows) / len(rows) if rows else None
    w = max(c.get("SQ_WAVES", 0), 1)
    out["kernels"][k] = {"launches": n, "bench_median_ms": ms, "counters_per_launch": c, "valu_insts_per_wave": c.get("SQ_INSTS_VALU", 0) / w,
                         "vmem_rd_insts_per_wave": c.get("SQ_INSTS_VMEM_RD", 0) / w,
                         "valu_busy": 4 * c.get("SQ_ACTIVE_INST_VALU", 0) / (ms * 1e-3 * 2.4e9 * 1024) if ms else None,
                         "wait_inst_any_per_wave_cycle": c.get("SQ_WAIT_INST_ANY", 0) / max(c.get("SQ_WAVE_CYCLES", 1), 1)}
print(json.dumps(out, indent=1, sort_keys=True))
PY
rc=$?
rm -rf $O/sq
exit $rc
