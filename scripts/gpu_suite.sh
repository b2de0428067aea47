# A change's visit to the GPU. check: smoke, the -m gpu suite (-x) and a C2 bench line. full: the
# same, then the bench line with every workload (results/TAG_bench.json, full records in
# results/TAG_bench_full.json) and its summary, C3 with warm-up 5 (warm-up independence) and the
# torchrun/RCCL path at world size 1. Every step runs under a time limit of its own; the first step
# that fails prints the end of its output and ends the script. Nothing is tried twice.
# Usage: [LOGDIR=DIR] bash scripts/gpu_suite.sh check|full TAG [-k EXPR]
# Logs go to DIR/TAG_* (DIR relative to the repository root; default results/).
set -u
MODE=${1:-} TAG=${2:-}
case "$MODE:$TAG" in check:?*|full:?*) ;; *) echo "usage: gpu_suite.sh check|full TAG [-k EXPR]"; exit 2 ;; esac
K=(); [ "${3:-}" = -k ] && K=(-k "$4")
LOGDIR=${LOGDIR:-results}
cd "$(dirname "$0")/.." && mkdir -p "$LOGDIR" results || exit 1
O=$LOGDIR/$TAG B=results/${TAG}_bench

step() {    # step NAME SECONDS OUT COMMAND...: stdout to OUT, stderr to OUT.err
  local name=$1 secs=$2 out=$3; shift 3
  timeout -k 10 "$secs" "$@" > "$out" 2> "$out.err" || { echo "$name failed ($?)"; tail -30 "$out" "$out.err"; exit 1; }
  echo "$name ok"
}

step smoke 300 ${O}_smoke.txt python -c "import __graft_entry__ as g; g.smoke()"
step "gpu tests" 1000 ${O}_gpu_tests.txt python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread "${K[@]}"
tail -2 ${O}_gpu_tests.txt
step "bench c2" 300 ${O}_bench_c2.json python bench.py --workload c2 --no-cpu-baseline
python -c "import json; d=json.load(open('${O}_bench_c2.json')); r=d['roofline']; print('c2', d['value'], d['ms_per_step'], d['wall_ms_per_step'], r['avg_launch_ms'], r['frac'], 'traffic', r.get('traffic'), 'frac_measured', r.get('frac_measured'))"
[ "$MODE" = full ] || exit 0
step "bench --full" 600 $B.json python bench.py --full --full-json ${B}_full.json
wc -c $B.json
python scripts/bench_summary.py $B.json
step "bench c3 warm-up 5" 300 ${O}_bench_c3w5.json python bench.py --workload c3 --warmup 5 --no-cpu-baseline
step "torchrun bench" 300 results/${TAG}_bench_dist.log python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --gpus 1 --steps 5 --warmup 1 --full
