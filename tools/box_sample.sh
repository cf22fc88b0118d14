#!/bin/bash
# samples the box kind: short step timing; on a fast-kind box (step < 8.95 ms) also the full bench line
# usage: bash tools/box_sample.sh OUTDIR
O=$(realpath -m "${1:?usage: bash tools/box_sample.sh OUTDIR}"); mkdir -p "$O"
cd "$(dirname "$0")/.."
python tools/dec_quick.py --time-only 2>&1 | grep -v amdgpu.ids | head -3 > "$O"/box_sample.txt
cat "$O"/box_sample.txt
S=$(grep -o "S1: [0-9.]*" "$O"/box_sample.txt | cut -d' ' -f2)
if python -c "import sys; sys.exit(0 if float('$S') < 8.95 else 1)"; then
  python bench.py --full > "$O"/r04_bench_fastbox.json 2> "$O"/r04_bench_fastbox.err
  python tools/family_trace.py 2>&1 | grep -v amdgpu.ids > "$O"/r04_family_trace_fastbox.txt
  tail -c 300 "$O"/r04_bench_fastbox.json
fi
