#!/bin/bash
# usage: gpu_bench_profile.sh <tag> [<output dir>]   -- the record run of a round: full bench line, rocprofv3 kernel-trace summary of
# the same command, and the two PMC passes (FETCH_SIZE / WRITE_SIZE) behind roofline.traffic.  Writes the summaries to <output dir>/<tag>_*
# (default: profile_out/ in the repository root).
TAG=${1:-r03}
R=$(cd "$(dirname "$0")/.." && pwd)
O=${2:-$R/profile_out}; mkdir -p $O; O=$(cd $O && pwd)
export TMPDIR=/tmp
cd $R
( time timeout -k 10 600 python bench.py --full --steps 4 --warmup 1 ) > $O/${TAG}_bench_full.log 2>&1 || exit 1
tail -4 $O/${TAG}_bench_full.log | cut -c1-900
cd /tmp
rm -rf $O/prof_$TAG
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG/trace -- python $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-call32 > $O/${TAG}_trace.log 2>&1 || exit 1
timeout -k 10 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/prof_$TAG/pmc_fetch -- python $R/bench.py --steps 1 --warmup 0 --nsteps 400 --no-cpu-baseline --no-call32 > $O/${TAG}_fetch.log 2>&1 || exit 1
timeout -k 10 600 rocprofv3 --kernel-trace --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum --output-format csv -d $O/prof_$TAG/pmc_write -- python $R/bench.py --steps 1 --warmup 0 --nsteps 400 --no-cpu-baseline --no-call32 > $O/${TAG}_write.log 2>&1 || exit 1
cd $R
cp $O/prof_$TAG/trace/*/*kernel_stats.csv $O/${TAG}_bench_kernel_stats.csv
python scripts/pmc_summary.py $O/prof_$TAG/pmc_fetch > $O/${TAG}_bench_pmc_fetch.txt
python scripts/pmc_summary.py $O/prof_$TAG/pmc_write > $O/${TAG}_bench_pmc_write.txt
head -8 $O/${TAG}_bench_kernel_stats.csv | cut -c1-200
head -14 $O/${TAG}_bench_pmc_fetch.txt
# keep the raw kernel trace small enough to merge back: first shot group only
rm -rf $O/prof_$TAG   # raw traces and counter CSVs (tens of MB); the summaries above are what is kept
# the same bench line with the two-launch backward step (option bwd_fuse=2): what the persistent loop is compared with
( timeout -k 10 300 python bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-call32 --option bwd_fuse=2 ) > $O/${TAG}_bench_two_launch.log 2>&1
tail -1 $O/${TAG}_bench_two_launch.log | cut -c1-400
# configs[1] shape, forward only, un-profiled
( timeout -k 10 300 python bench.py --mode fwd --nz 500 --nsteps 2000 --steps 3 --warmup 1 --no-cpu-baseline ) > $O/${TAG}_fwd2000x500_bench.log 2>&1
tail -1 $O/${TAG}_fwd2000x500_bench.log | cut -c1-400
# configs[3]'s per-GPU load in one call: 32 shots per step (one step: 10.8 s)
( timeout -k 10 400 python bench.py --shots-per-step 32 --steps 1 --warmup 0 --no-cpu-baseline --no-call32 ) > $O/${TAG}_bench_32shots.log 2>&1
tail -1 $O/${TAG}_bench_32shots.log | cut -c1-400
