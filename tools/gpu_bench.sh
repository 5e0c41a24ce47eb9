# Whole bench line (N=1, --full), JSON line + stderr progress into $BENCH_OUT (default bench_out/)
# usage: bash tools/gpu_bench.sh [name] [extra bench args]
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
out=${BENCH_OUT:-bench_out}
mkdir -p $out
name=${1:-r3_bench}
shift
timeout -k 10 1100 python -u bench.py --full "$@" > $out/$name.json 2> $out/$name.err
echo bench_rc=$?
tail -c 6000 $out/$name.json
