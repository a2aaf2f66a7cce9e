#!/bin/bash
# Row-layout dev loop on the GPU box: parity tests, stage split, bench (verified).
set -o pipefail
mkdir -p bench_out; export TMPDIR=/tmp
B=${B:-4}
timeout -k 10 600 python -m pytest tests/test_aes_rows.py tests/test_gpu_parity.py -x -q -m gpu > bench_out/pytest_rows.log 2>&1 && echo tests ok \
&& timeout -k 10 300 python tools/round_stages.py rows $B > bench_out/stages_rows.log 2>&1 && cat bench_out/stages_rows.log \
&& timeout -k 10 300 python bench.py --full --check --no-cpu-baseline --batch $B > bench_out/bench_rows.json 2>&1 && cat bench_out/bench_rows.json
rc=$?; tail -3 bench_out/pytest_rows.log; exit $rc
