# Full evidence run of a round: tests, headline bench, kernel-trace stats, PMC passes, config sweep, all under $OUT (default runs):
#   [OUT=dir] bash tools/gpu_final.sh TAG        then   [OUT=dir] python tools/collect_profiles.py TAG rNN
TAG=${1:-rXX}
export OUT=${OUT:-runs}; mkdir -p "$OUT"
bash tools/gpu_session.sh $TAG
bash tools/pmc_mfma.sh $TAG
bash tools/sweep_configs.sh > $OUT/${TAG}_config_sweep.jsonl 2> $OUT/${TAG}_config_sweep.err; cut -c1-200 $OUT/${TAG}_config_sweep.jsonl
