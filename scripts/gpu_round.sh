#!/bin/bash
# Round-end evidence on one GPU: pytest -m gpu, smoke, bench.py --full (the
# judged line with every other figure beside it), the rocprofv3
# kernel-trace/stats summary of the same bench command,
# and the FETCH_SIZE / WRITE_SIZE PMC passes (one counter per run,
# MI355X_MICROARCH.md HBM section).  Collect with
# `python scripts/collect_profiles.py --round N`.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp
OUT=gpurun_out/round
rm -rf $OUT
mkdir -p $OUT
BARGS="${BENCH_ARGS:-}"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -2 $OUT/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke(); print("smoke ok")' > $OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -2 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full $BARGS > $OUT/bench.json 2> $OUT/bench.err
rc=$?; echo "bench rc=$rc"; cat $OUT/bench.json; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o run -- python3 bench.py --no-cpu --no-single --no-unpadded --no-other --no-host $BARGS > $OUT/trace_bench.json 2> $OUT/trace.err
rc=$?; echo "trace rc=$rc"; cat $OUT/trace_bench.json; [ $rc -eq 0 ] || exit $rc
# per-shape kernel traces of the other workloads (one launch shape per run, so
# no averages mix): C4 x 16 stripes, C2 one stripe and x 16, C5 x 32, C5 repair x 8
for cfg in C4x16 C2 C2x16 C5b32 C5rb8; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_$cfg -o run -- python3 scripts/time_ops.py --configs $cfg --iters 20 > $OUT/trace_$cfg.json 2> $OUT/trace_$cfg.err
  rc=$?; echo "trace $cfg rc=$rc"; [ $rc -eq 0 ] || exit $rc
done
# each rank's launch shape of an N-GPU run (bench.py --slice-of N, default
# bytes-weak layout: rank 0's byte range of N x 256 stripes), and the strong
# layout's 8-rank shape (256 stripes) beside it
for n in 2 4 8; do
  timeout -k 10 300 python bench.py --slice-of $n --no-cpu --no-other --no-host $BARGS > $OUT/slice_$n.json 2> $OUT/slice_$n.err
  rc=$?; echo "slice $n rc=$rc"; [ $rc -eq 0 ] || exit $rc
done
timeout -k 10 300 python bench.py --split bytes --slice-of 8 --no-cpu --no-other --no-host $BARGS > $OUT/slice_8_strong.json 2> $OUT/slice_8_strong.err
rc=$?; echo "slice 8 strong rc=$rc"; [ $rc -eq 0 ] || exit $rc
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_$c -o run -- python3 bench.py --no-cpu --no-single --no-unpadded --no-other --no-host --steps 50 --warmup 5 > $OUT/pmc_$c.json 2> $OUT/pmc_$c.err
  rc=$?; echo "pmc $c rc=$rc"; [ $rc -eq 0 ] || exit $rc
  # the launch shape of each rank of an N-GPU byte-range run (bench.py --slice-of N)
  for n in 2 4 8; do
    timeout -k 10 300 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_${c}_s$n -o run -- python3 bench.py --slice-of $n --no-cpu --no-single --no-unpadded --no-other --no-host --steps 50 --warmup 5 > $OUT/pmc_${c}_s$n.json 2> $OUT/pmc_${c}_s$n.err
    rc=$?; echo "pmc $c slice $n rc=$rc"; [ $rc -eq 0 ] || exit $rc
  done
done
exit 0
