#!/bin/bash
# GPU check used during development: full GPU suite, dense factor across
# sizes, C3 bench with its phase and roofline figures but without the tracker
# legs.  Logs go to the directory given as the first argument.
#   bash tools/gpu_check.sh OUT_DIR
set -o pipefail
O=${1:?usage: gpu_check.sh OUT_DIR}
mkdir -p "$O"
timeout -k 10 120 python tools/chol_scale.py > "$O/chol_scale.txt" 2>&1 && \
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > "$O/gpu_tests.log" 2>&1 && \
timeout -k 10 300 python bench.py --full --no-tracker --no-cpu-baseline --no-oneshot > "$O/bench.json" 2> "$O/bench.err"
