#!/bin/bash
# One GPU-box visit: smoke, GPU parity tests, full bench line, rocprofv3 kernel stats.  Logs land in $OUT_DIR (default: round_out/).
set -u
export TMPDIR=/tmp
cd "${GRAFT_REPO_ROOT:-.}"
OUT="${OUT_DIR:-round_out}"
mkdir -p "$OUT"
echo "== rocm-smi" > $OUT/env.log; rocm-smi --showproductname 2>&1 | head -20 >> $OUT/env.log; nproc >> $OUT/env.log; lscpu | grep "Model name" >> $OUT/env.log
echo "== smoke"; timeout 600 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke exit $?" | tee -a $OUT/smoke.log; tail -5 $OUT/smoke.log
echo "== pytest -m gpu"; timeout 1500 python -m pytest tests -m gpu -q --timeout 400 --timeout-method=thread -p no:cacheprovider ${PYTEST_ARGS:-} > $OUT/pytest_gpu.log 2>&1; echo "pytest exit $?" | tee -a $OUT/pytest_gpu.log; tail -40 $OUT/pytest_gpu.log
if [ -n "${DIAG:-}" ]; then echo "== diag"; timeout 1200 python scripts/gpu_diag.py $DIAG > $OUT/diag.log 2>&1; echo "diag exit $?"; cat $OUT/diag.log | tail -40; fi
echo "== bench"; timeout 900 python bench.py --full ${BENCH_ARGS:-} > $OUT/bench.log 2>&1; echo "bench exit $?" | tee -a $OUT/bench.log; tail -3 $OUT/bench.log
if [ "${DO_PROF:-1}" = "1" ]; then
  # two kernel traces of the bench command: whole-device launches (engine option batch_lanes=1, the launch shape bench.py's HIP-event
  # roofline measurement times) and the default 4 concurrent lanes of the timed region
  for lanes in 1 4; do
    echo "== rocprofv3 lanes=$lanes"
    (cd /tmp && HGS_ENGINE_OPTIONS=batch_lanes=$lanes timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OLDPWD/$OUT/prof_lanes$lanes" -o bench -- python "$OLDPWD/bench.py" --steps 2 --warmup 1 --no-cpu-baseline ${BENCH_ARGS:-} > "$OLDPWD/$OUT/prof_lanes$lanes.log" 2>&1); echo "prof exit $?"
    f=$(find $OUT/prof_lanes$lanes -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -12 "$f"
  done
fi
