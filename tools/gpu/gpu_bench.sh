# the full benchmark line (CPU baseline + self-check), then its kernel trace and PMC byte counts;
# logs and profiles go to $OUT (default bench_out/); the first step that fails ends the script
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
step() { n=$1; shift; "$@" > $OUT/$n.log 2>&1; r=$?; echo "$n rc=$r" >> $OUT/$n.log; [ $r -eq 0 ] || exit $r; }
step bench timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 3
step prof timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python -u bench.py --steps 10 --warmup 3
python tools/trace_summary.py $OUT/prof/run_kernel_trace.csv 10 $OUT/prof/solve_dispatches.json >> $OUT/prof.log 2>&1
step pmc_fetch timeout -k 10 180 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o run -- python -u bench.py --steps 3 --warmup 1
step pmc_write timeout -k 10 180 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o run -- python -u bench.py --steps 3 --warmup 1
