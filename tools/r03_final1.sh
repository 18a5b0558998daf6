#!/bin/bash
# final pass 1 (GPU box): the whole -m gpu suite with durations, smoke(), the driver's bench command with --full; logs under $LOG_DIR
L=${LOG_DIR:-bench_logs}; mkdir -p "$L"
python3 -m pytest tests -q -m gpu --durations=15 > "$L/r03_final_gpu_tests.log" 2>&1; echo "pytest rc=$?" >> "$L/r03_final_gpu_tests.log"
tail -22 "$L/r03_final_gpu_tests.log"
python3 -c "import __graft_entry__ as g; g.smoke()" > "$L/r03_final_smoke.log" 2>&1; tail -2 "$L/r03_final_smoke.log"
python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > "$L/r03_final_bench_c3.log" 2>&1; tail -c 300 "$L/r03_final_bench_c3.log"
