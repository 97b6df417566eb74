set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -x -q -m gpu > $OUT/full_gpu.log 2>&1; echo "pytest rc=$?"; tail -3 $OUT/full_gpu.log
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1; tail -1 $OUT/smoke.log
python bench.py --full > $OUT/bench_c4.json 2> $OUT/bench_c4.err; echo "c4 rc=$?"
python bench.py --full --config c3 > $OUT/bench_c3.json 2> $OUT/bench_c3.err; echo "c3 rc=$?"
python bench.py --full --config c5 --steps 3 --warmup 1 > $OUT/bench_c5.json 2> $OUT/bench_c5.err; echo "c5 rc=$?"
python bench.py --full --launcher inlib > $OUT/bench_inlib1.json 2> $OUT/bench_inlib1.err; echo "inlib rc=$?"
bash tools/profile_k1.sh > $OUT/profile.log 2>&1; echo "profile rc=$?"
python tools/tie_sweep.py > $OUT/tie_sweep.log 2>&1
python tools/yeast_time.py > $OUT/yeast.log 2>&1
python tools/n_sweep.py 500 2000 5000 10000 12000 13000 14272 16000 20000 30000 50000 65535 > $OUT/n_sweep.log 2>&1
python tools/na_sweep.py > $OUT/na_sweep.log 2>&1
python tools/host_path_time.py > $OUT/host_path.log 2>&1
echo done
