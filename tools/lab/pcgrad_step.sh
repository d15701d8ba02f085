#!/bin/bash
# ms per step of the "total" and the "per_task" step, then the kernel stats of the new kernels in a run of their own,
# then profiles/pcgrad_mmoe_ae30_b65536.txt.  Every GPU step under its own time limit; a failed step ends the script.
set -o pipefail
out=${1:-build/pcgrad_lab}
mkdir -p $out
timeout -k 10 300 python3 tools/lab/pcgrad_step.py --mode time --out $out > $out/time.log 2>&1 || { tail -20 $out/time.log; exit 1; }
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -- python3 tools/lab/pcgrad_step.py --mode profile --steps 20 --out $out > $out/prof.log 2>&1 || { tail -20 $out/prof.log; exit 1; }
python3 tools/lab/pcgrad_step.py --mode report --out $out
