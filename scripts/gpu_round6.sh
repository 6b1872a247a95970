#!/bin/bash
# Round-6 measurement set (results under gpurun_out/, copied to profiles/ by
# hand), each step under its own time limit (scripts/gpu_steps.sh).
#   usage: scripts/gpu_round6.sh 1|2|3|4
cd "${GRAFT_REPO_ROOT:-/root/repo}"
R="$PWD"
P="rocprofv3 --kernel-trace --stats --output-format csv -o run -d"
case "$1" in
1) scripts/gpu_steps.sh \
  "500 gputest python -u -m pytest tests -m gpu -v --timeout 150 --timeout-method thread" \
  "150 smoke python -c 'import __graft_entry__ as g; g.smoke()'" \
  "300 b3 python -u bench.py --full" \
  "300 b3t0 python -u bench.py --full --ts-order 0 --no-cpu" \
  "300 s3 cd /tmp && $P $R/gpurun_out/s3 -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu --no-parity" \
  "300 s3t0 cd /tmp && $P $R/gpurun_out/s3t0 -- python3 $R/bench.py --ts-order 0 --steps 3 --warmup 1 --no-cpu --no-parity" ;;
2) scripts/gpu_steps.sh \
  "400 pmc3 bash scripts/gpu_pmc.sh r06_pmc_config3.json" \
  "400 pmc3t0 env BENCH_ARGS='--ts-order 0' bash scripts/gpu_pmc.sh r06_pmc_config3_ts_order0.json" ;;
3) scripts/gpu_steps.sh \
  "300 b2 python -u bench.py --full --workload filter" \
  "300 bz python -u bench.py --full --keys-dist zipf --no-cpu" \
  "300 bzt0 python -u bench.py --full --keys-dist zipf --ts-order 0 --no-cpu" \
  "300 b5 python -u bench.py --full --workload config5" \
  "200 bdo python -u bench.py --deliver --ordered --no-cpu --no-parity" \
  "200 bh python -u bench.py --ingest host --no-cpu --no-parity" \
  "200 s5 cd /tmp && $P $R/gpurun_out/s5 -- python3 $R/bench.py --workload config5 --steps 3 --warmup 1 --no-cpu --no-parity" \
  "200 s2 cd /tmp && $P $R/gpurun_out/s2 -- python3 $R/bench.py --workload filter --steps 3 --warmup 1 --no-cpu --no-parity" ;;
4) scripts/gpu_steps.sh \
  "300 pmc2 env BENCH_ARGS='--workload filter' PMC_EVENTS=100000000 bash scripts/gpu_pmc.sh r06_pmc_filter.json" \
  "300 pmc5 env BENCH_ARGS='--workload config5' PMC_EVENTS=16777216 bash scripts/gpu_pmc.sh r06_pmc_config5.json" \
  "300 pmcz env BENCH_ARGS='--keys-dist zipf' bash scripts/gpu_pmc.sh r06_pmc_zipf.json" \
  "200 rank2 env CEP_DIST_BACKEND=gloo python3 bench.py --gpus 2 --steps 3 --warmup 2 --no-cpu" ;;
esac
