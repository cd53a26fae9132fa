export TMPDIR=/tmp
OUT=${OUT:-$PWD/check_out}
mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -m gpu -x -q > "$OUT/gpu_tests.log" 2>&1 &&
timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" &&
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_trace" -o run -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/prof_trace.log" 2>&1 &&
timeout -k 10 600 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/prof_fetch" -o run -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/prof_fetch.log" 2>&1 &&
timeout -k 10 600 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/prof_write" -o run -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$OUT/prof_write.log" 2>&1
