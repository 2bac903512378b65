#!/bin/bash
# usage (on the GPU box): bash profiles/prof_r03.sh <outdir-name>     -> gpurun_out/<outdir-name>/...
# Kernel statistics, HBM traffic (separate FETCH_SIZE / WRITE_SIZE passes), SQ and MFMA counters of the bench command,
# then the plain bench lines.  Counter passes carry --kernel-trace only (no other trace domain).
set -o pipefail
cd /tmp; export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/$1; mkdir -p $O
B="python3 $R/bench.py --no-cpu-baseline --no-extras"
rocprofv3 --kernel-trace --stats -d $O/c3_stats -o c3 --output-format csv -- $B --steps 3 --warmup 1 > $O/c3_stats.json 2> $O/c3_stats.err && echo c3_stats ok
rocprofv3 --kernel-trace --stats -d $O/c3h_stats -o c3h --output-format csv -- $B --steps 2 --warmup 1 --data hard > $O/c3h_stats.json 2> $O/c3h_stats.err && echo c3h_stats ok
rocprofv3 --kernel-trace --stats -d $O/c5_stats -o c5 --output-format csv -- $B --config c5 --steps 2 --warmup 1 > $O/c5_stats.json 2> $O/c5_stats.err && echo c5_stats ok
for cfg in c3 c5; do
  rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/${cfg}_fetch -o f --output-format csv -- $B --config $cfg --steps 1 --warmup 0 > /dev/null 2> $O/${cfg}_fetch.err && echo ${cfg}_fetch ok
  rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/${cfg}_write -o w --output-format csv -- $B --config $cfg --steps 1 --warmup 0 > /dev/null 2> $O/${cfg}_write.err && echo ${cfg}_write ok
  rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES --kernel-trace -d $O/${cfg}_sq -o s --output-format csv -- $B --config $cfg --steps 1 --warmup 0 > /dev/null 2> $O/${cfg}_sq.err && echo ${cfg}_sq ok
done
for cfg in c3 c5; do
  f=$(find $O/${cfg}_fetch -name "*counter_collection.csv" | head -1); w=$(find $O/${cfg}_write -name "*counter_collection.csv" | head -1)
  python3 $R/profiles/summarize_pmc.py $f $w 16384 16384 $O/r03_${cfg}_pmc_traffic && echo ${cfg}_traffic ok
  s=$(find $O/${cfg}_sq -name "*counter_collection.csv" | head -1); k=$(find $O/${cfg}_sq -name "*kernel_trace.csv" | head -1)
  python3 $R/profiles/summarize_sq.py $s $k $O/r03_${cfg}_pmc_sq.md && echo ${cfg}_sq_summary ok
done
cp $(find $O/c3_stats -name "*kernel_stats.csv" | head -1) $O/r03_c3_16384_kernel_stats.csv
cp $(find $O/c3h_stats -name "*kernel_stats.csv" | head -1) $O/r03_c3_hard_16384_kernel_stats.csv
cp $(find $O/c5_stats -name "*kernel_stats.csv" | head -1) $O/r03_c5_16384_kernel_stats.csv
rm -rf $O/c3_stats $O/c3h_stats $O/c5_stats $O/*_fetch $O/*_write $O/*_sq
python3 $R/bench.py --full > $O/r03_bench_c3.json 2> $O/bench_c3.err && echo bench_c3 ok
python3 $R/bench.py --full --data hard --no-extras > $O/r03_bench_c3_hard.json 2> $O/bench_c3h.err && echo bench_c3_hard ok
python3 $R/bench.py --full --config c5 > $O/r03_bench_c5.json 2> $O/bench_c5.err && echo bench_c5 ok
python3 $R/bench.py --full --config c2 > $O/r03_bench_c2.json 2> $O/bench_c2.err && echo bench_c2 ok
ls $O
