#!/bin/bash
# usage: tools/final_pass.sh <output dir>   (empty <output dir>/traffic and <output dir>/prof_serial first: new files
# would land next to old ones)
# End-of-round evidence pass on the GPU box: smoke, PMC traffic, serial kernel stats, the full bench line, secondary
# workloads.  Everything lands in <output dir>; tools/update_profiles.py copies the judged pieces into profiles/.
out=${1:?usage: tools/final_pass.sh <output dir>}
mkdir -p "$out"
python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -1
bash tools/pmc_traffic.sh $out/traffic > $out/pmc.log 2>&1; tail -2 $out/pmc.log
bash tools/prof_serial.sh $out/prof_serial > $out/prof_serial.log 2>&1; tail -4 $out/prof_serial.log
python3 bench.py --full > $out/bench_default.json 2> $out/bench_default.err; tail -1 $out/bench_default.json | cut -c1-300
bash tools/bench_secondary.sh $out 2>&1 | tail -14
python3 tools/bench_rows.py --graph > $out/rows.jsonl 2> $out/rows.err; cat $out/rows.jsonl
MMLREC_BENCH_FORCE_SHARD=1 python3 bench.py --full --gpus 2 --no-cpu-baseline --no-configs --no-lazy > $out/bench_forced_shard.json 2> $out/bench_forced_shard.err; tail -1 $out/bench_forced_shard.json | cut -c1-200
