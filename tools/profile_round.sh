# Round profile: whole bench line (--full), rocprofv3 kernel stats of a short run, and knn2 PMC passes,
# into $BENCH_OUT (default bench_out/).
# usage: bash tools/profile_round.sh <tag>
set -o pipefail
tag=${1:-v4}
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
out=${BENCH_OUT:-bench_out}
mkdir -p $out
timeout -k 10 900 python3 -u bench.py --full > $out/bench_$tag.log 2>&1 || { echo BENCH_FAILED; tail -20 $out/bench_$tag.log; exit 1; }
tail -1 $out/bench_$tag.log | cut -c1-300
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --pmc off > $out/prof_$tag.log 2>&1 || { echo PROF_FAILED; tail -20 $out/prof_$tag.log; exit 1; }
for ctr in FETCH_SIZE WRITE_SIZE "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES"; do
  name=$(echo $ctr | cut -d' ' -f1)
  timeout -s KILL 300 rocprofv3 --pmc $ctr --output-format csv -d $out/pmc_knn2_${tag}_$name -o run -- python3 bench.py --knn2 only --no-cpu-baseline --knn2-reps 1 > $out/pmc_knn2_${tag}_$name.log 2>&1 || { echo PMC_FAILED $name; tail -5 $out/pmc_knn2_${tag}_$name.log; exit 1; }
done
echo PROFILE_OK
