#!/bin/bash
# final pass 3 (GPU box): the table at 1 Gb (k = 47, 3 colours, ~1.05e9 records) on the final build, with --full (log under $LOG_DIR); then the
# GPU seed sweep for what time is left
L=${LOG_DIR:-bench_logs}; mkdir -p "$L"
python3 bench.py --full --genome-len 1000000000 --repeat-families 170000 --steps 5 --warmup 2 --cpu-seconds 15 > "$L/r03_final_bench_c3_1Gb.log" 2>&1; tail -c 400 "$L/r03_final_bench_c3_1Gb.log"; echo
rm -f /tmp/ldbg_bench/c3_L1000000000*
echo pass3 done
