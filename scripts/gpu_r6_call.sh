# the round's standard GPU call: smoke, the GPU suite, the driver-format bench line (kept as the last form of the scratch script
# that every measurement of LABNOTES round 6 went through; usage: bash scripts/gpu_r6_call.sh OUTDIR)
set -x
cd $GRAFT_REPO_ROOT
OUT="${1:?usage: gpu_r6_call.sh OUTDIR}"; mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1; echo "smoke rc=$?" >> "$OUT/smoke.log"
python -m pytest tests -m gpu -q 2>&1 | tail -6 > "$OUT/gpu_tests.log"
python bench.py --full --steps 20 --warmup 5 > "$OUT/bench_default_run.json" 2> "$OUT/bench_default_run.err"
tail -2 "$OUT/smoke.log"; tail -3 "$OUT/gpu_tests.log"; tail -2 "$OUT/bench_default_run.err"
