#!/bin/bash
# the whole -m gpu suite with durations, then the default bench line with --full (run on the GPU box from the repo root; logs under $LOG_DIR)
T=${1:-full}
L=${LOG_DIR:-bench_logs}; mkdir -p "$L"
python3 -m pytest tests -q -m gpu --durations=30 -x > "$L/r03_${T}_gpu_tests.log" 2>&1; echo "pytest rc=$?" >> "$L/r03_${T}_gpu_tests.log"
tail -45 "$L/r03_${T}_gpu_tests.log"
python3 bench.py --full > "$L/r03_${T}_bench.log" 2>&1; tail -c 400 "$L/r03_${T}_bench.log"
