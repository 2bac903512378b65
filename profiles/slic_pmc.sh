#!/bin/bash
# K23 counters at 16384^2, P = 7, S = 16: one SQ pass (instruction counts, VALU activity, waits) in a run of its own, with no
# tracing beside it, over profiles/slic_bench.py --worker 7 16.  The times come from profiles/slic_bench.json (the library's
# device events in an unprofiled run): VALU busy = 4 * SQ_ACTIVE_INST_VALU / (ms * 2.4 GHz * 1024 SIMDs), the counter being in
# quad-cycles.   usage: bash profiles/slic_pmc.sh <outdir> [bench.json]   -> <outdir>/slic_pmc.json
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); O=$(mkdir -p "$1" && cd "$1" && pwd); J=$(realpath "${2:-$R/profiles/slic_bench.json}")
cd /tmp; export TMPDIR=/tmp
REPS=2; ITERS=3
timeout -k 10 600 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_BUSY_CYCLES \
    -d $O/sq -o s --output-format csv -- python3 $R/profiles/slic_bench.py --worker 7 16 --reps $REPS --iters $ITERS > /dev/null 2> $O/sq.err || exit $?
s=$(find $O/sq -name "*counter_collection.csv" | head -1)
python3 - "$s" "$J" > $O/slic_pmc.json <<'PY'
import collections, csv, json, os, re, sys
short = lambda n: re.sub(r"\(.*$", "", re.sub(r"^void ", "", n))
cnt = collections.defaultdict(lambda: collections.defaultdict(float))
launches = collections.Counter()
for r in csv.DictReader(open(sys.argv[1])):
    if "k23_" in r["Kernel_Name"]:
        k = short(r["Kernel_Name"])
        cnt[k][r["Counter_Name"]] += float(r["Counter_Value"])
        if r["Counter_Name"] == "SQ_WAVES":
            launches[k] += 1
it_ms = None
if os.path.exists(sys.argv[2]):
    for c in json.load(open(sys.argv[2]))["cases"]:
        if c["P"] == 7 and c["S"] == 16:
            it_ms = c["iteration_ms"]
out = {"about": "rocprofv3 --pmc (no tracing) over profiles/slic_bench.py --worker 7 16 at 16384^2; iteration_ms is the unprofiled "
                "time of one assign-and-accumulate iteration from slic_bench.json; VALU busy of the assignment kernel = "
                "4 * SQ_ACTIVE_INST_VALU / (launches * iteration_ms * 2.4 GHz * 1024 SIMDs)", "iteration_ms": it_ms, "kernels": {}}
for k, c in cnt.items():
    w = max(c.get("SQ_WAVES", 0), 1)
    e = {"launches": launches[k], "counters": dict(c), "valu_insts_per_wave": c.get("SQ_INSTS_VALU", 0) / w,
         "lds_insts_per_wave": c.get("SQ_INSTS_LDS", 0) / w,
         "wait_inst_any_per_wave_cycle": c.get("SQ_WAIT_INST_ANY", 0) / max(c.get("SQ_WAVE_CYCLES", 1), 1)}
    if it_ms and "k23_assign" in k and "false" in k:   # the iterations' instantiation, not the INIT one
        e["valu_busy"] = 4 * c.get("SQ_ACTIVE_INST_VALU", 0) / (launches[k] * it_ms * 1e-3 * 2.4e9 * 1024)
    out["kernels"][k] = e
print(json.dumps(out, indent=1, sort_keys=True))
PY
rm -rf $O/sq
