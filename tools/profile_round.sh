#!/bin/bash
# usage (on the GPU box, from the repo root): bash tools/profile_round.sh TAG OUTDIR
# bench line (--full), rocprofv3 kernel stats of the same command, PMC traffic passes -> OUTDIR/TAG_*
set -u
T=$1
D=${2:?usage: bash tools/profile_round.sh TAG OUTDIR}
mkdir -p $D
export TMPDIR=/tmp
timeout 600 python -m pytest tests -m gpu -q 2>&1 | tail -4 > $D/${T}_tests.log
timeout 300 python bench.py --full > $D/${T}_bench.json 2> $D/${T}_bench.err
rm -rf $D/${T}_prof
timeout 300 rocprofv3 --kernel-trace --stats -d $D/${T}_prof -o p --output-format csv -- python bench.py --full --steps 500 --warmup 100 --no-cpu-baseline > $D/${T}_bench_rocprof.json 2>/dev/null
cp $D/${T}_prof/p_kernel_stats.csv $D/${T}_kernel_stats.csv
rm -rf $D/${T}_prof
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf $D/pmc_$c
  timeout 300 rocprofv3 --pmc $c --kernel-trace -d $D/pmc_$c -o p --output-format csv -- python bench.py --full --steps 60 --warmup 20 --no-cpu-baseline > /dev/null 2>&1
  rm -f $D/pmc_$c/p_kernel_trace.csv
done
cat $D/${T}_tests.log
python tools/kstats.py $D/${T}_kernel_stats.csv
python tools/pmc.py $D
tail -c 400 $D/${T}_bench.json
