# [OUT=dir] bash tools/refresh_profiles.sh: GPU tests, smoke, the two --full bench lines, kernel trace and PMC passes of the headline (outputs under $OUT/refresh_*, OUT defaults to runs)
R=$PWD
OUT=${OUT:-runs}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
python -m pytest tests -m gpu -q 2>&1 | tail -3 > $OUT/refresh_pytest.txt
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/refresh_smoke.txt 2>&1
DPB_PROFILE_CSV=$OUT/refresh_gemm_launches.csv python bench.py --full 2>/dev/null > $OUT/refresh_bench_sd15.json
python bench.py --workload ddpm256 --dtype fp32 --full 2>/dev/null > $OUT/refresh_bench_ddpm256.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/refresh_stats -o sd15 -- python $R/bench.py --profile-run > /dev/null 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/refresh_pmc_fetch -o f -- python $R/bench.py --steps 12 --warmup 0 --profile-run > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/refresh_pmc_write -o w -- python $R/bench.py --steps 12 --warmup 0 --profile-run > /dev/null 2>&1
cd $R; ls $OUT/refresh_*; cat $OUT/refresh_pytest.txt $OUT/refresh_smoke.txt | tail -5
