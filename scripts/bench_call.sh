# The bench line with every workload into results/TAG_bench.json (+ _full.json) and its summary
cd "$(dirname "$0")/.." && mkdir -p results && timeout -k 10 600 python bench.py --full --full-json results/$1_bench_full.json > results/$1_bench.json 2> results/$1_bench.err; rc=$?; python scripts/bench_summary.py results/$1_bench.json; exit $rc
