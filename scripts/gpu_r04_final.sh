#!/bin/bash
# Round-4 evidence for profiles/ at the commit that ships: the driver's command twice, the default bench, rocprofv3 kernel statistics of the three
# workloads, the PMC passes (traffic), the bf16 benches, then the whole GPU suite.  Usage (repo root, GPU box): bash scripts/gpu_r04_final.sh [tag]
TAG=${1:-r04final}
OUT=$PWD/gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp HSA_ENABLE_IPC_MODE_LEGACY=0
for i in 1 2; do python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/driver_$i.json 2> $OUT/driver_$i.err; echo "driver cmd $i rc=$? $(python3 -c "import json; d=json.load(open('$OUT/driver_$i.json')); print(d['ms_per_step'], d['ms_per_step_resident'], d['inference']['ms_per_call'], d['roofline']['frac'])")"; done
bash scripts/gpu_profile.sh $TAG
for W in mlp stress; do
  timeout 300 python bench.py --full --workload $W --steps 200 --warmup 30 > $OUT/bench_$W.json 2>> $OUT/bench.err; echo "$W: $(cut -c1-200 $OUT/bench_$W.json)"
  ( cd /tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$W -o trace -- python $OLDPWD/bench.py --full --workload $W --steps 30 --warmup 10 --no-cpu-baseline > $OUT/rocprof_$W.log 2>&1 )
  for f in $(find $OUT/prof_$W -name "*kernel_stats.csv"); do cp $f $OUT/kernel_stats_$W.csv; cut -c1-150 $f | head -8; done
  find $OUT/prof_$W -name "*kernel_trace.csv" -delete; find $OUT/prof_$W -name "*.db" -delete
done
timeout 300 python bench.py --full --workload stress --precision bf16 --steps 200 --warmup 30 --no-cpu-baseline > $OUT/bench_stress_bf16.json 2>> $OUT/bench.err
timeout 300 python bench.py --full --precision bf16 --steps 200 --warmup 30 --no-cpu-baseline > $OUT/bench_hash_bf16.json 2>> $OUT/bench.err
cat $OUT/../../.git_commit 2>/dev/null > $OUT/commit.txt
timeout 600 python -m pytest tests -m gpu -q > $OUT/pytest.log 2>&1; echo "pytest rc=$?"; grep -E "passed|failed|error" $OUT/pytest.log | tail -2
echo done
