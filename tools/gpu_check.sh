#!/bin/bash
# One GPU-box pass: hardware microbench, smoke, GPU parity tests, bench.  Outputs -> $GPU_CHECK_OUT (gpu_check_out/)
cd "${GRAFT_REPO_ROOT:-.}" || exit 1
R=$(pwd); O="$R/${GPU_CHECK_OUT:-gpu_check_out}"
mkdir -p "$O"
export TMPDIR=/tmp
what="${1:-all}"
if [[ "$what" == all || "$what" == micro ]]; then
  hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize tools/microbench.hip -o /tmp/microbench 2>/dev/null \
    && timeout 300 /tmp/microbench > "$O/microbench.txt" 2>&1
  cat "$O/microbench.txt"
fi
if [[ "$what" == all || "$what" == smoke ]]; then
  timeout 600 python __graft_entry__.py smoke > "$O/smoke.txt" 2>&1; echo "smoke rc=$?"; tail -5 "$O/smoke.txt"
fi
if [[ "$what" == all || "$what" == test ]]; then
  timeout 1500 python -m pytest tests -m gpu -q --timeout 600 > "$O/pytest_gpu.txt" 2>&1; echo "pytest rc=$?"
  tail -40 "$O/pytest_gpu.txt"
fi
if [[ "$what" == all || "$what" == bench ]]; then
  timeout 900 python bench.py --full --steps 10 --warmup 3 > "$O/bench.txt" 2> "$O/bench.err"; echo "bench rc=$?"
  tail -3 "$O/bench.err"; cat "$O/bench.txt"
fi
if [[ "$what" == micro2 || "$what" == all2 ]]; then
  hipcc --offload-arch=gfx950 -O3 -fno-slp-vectorize tools/microbench2.hip -o /tmp/microbench2 2>/dev/null \
    && timeout 300 /tmp/microbench2 > "$O/microbench2.txt" 2>&1
  cat "$O/microbench2.txt"
fi
if [[ "$what" == prof || "$what" == all2 ]]; then
  rm -rf "$O/prof"; cd /tmp
  timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o bench -- python "$R/bench.py" --full --steps 10 --warmup 3 --no-cpu-baseline > "$O/prof_bench.txt" 2>&1
  cd "$R"; find "$O/prof" -name "*stats*" | head; f=$(find "$O/prof" -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -12 "$f"
fi
