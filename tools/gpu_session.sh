# One GPU-box session: the -m gpu tests, the headline bench line and the rocprofv3 kernel-trace summary of the same command.
#   [OUT=dir] bash tools/gpu_session.sh TAG [pytest-args...]      (outputs under $OUT/TAG_*, OUT defaults to runs)
TAG=${1:-sess}; shift
R=$PWD
OUT=${OUT:-runs}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
if [ -z "$SKIP_TESTS" ]; then   # (SKIP_TESTS=1: the suite ran in a call of its own -- the whole evidence run does not fit one 40-minute call)
  timeout 1500 python -m pytest tests -m gpu -q -s "$@" > $OUT/${TAG}_pytest.log 2>&1; tail -4 $OUT/${TAG}_pytest.log
fi
DPB_PROFILE_CSV=$OUT/${TAG}_gemm_launches.csv python bench.py --steps 20 --warmup 5 --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; cut -c1-600 $OUT/${TAG}_bench.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_stats -o sd15 -- python $R/bench.py --steps 36 --warmup 12 --profile-run > /dev/null 2>&1
cd $R; python tools/kernel_avgs.py $(ls $OUT/${TAG}_stats/*/*kernel_stats.csv $OUT/${TAG}_stats/*kernel_stats.csv 2>/dev/null | head -1) 48 30 > $OUT/${TAG}_kernel_avgs.txt 2>&1; head -40 $OUT/${TAG}_kernel_avgs.txt
