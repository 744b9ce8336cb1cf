#!/bin/bash
# Run ON THE GPU BOX (through gpurun) once the kernels are final: every record under profiles/ that carries the device sources'
# hash, in one go (about ten minutes).  Then HERE:
#   python tools/summarize_rocprof.py <round>; python tools/summarize_shapes.py --phase-shares-headline '{...}';
#   python tools/summarize_queue_prof.py <tag> after; cp <log directory>/<round>_bench_default.log profiles/
# usage: tools/record_round.sh <round tag, e.g. r03> [log directory, default records_out/ at the repository root]
# (the log directory holds this script's own logs; the profiler passes write their raw output where profile_*.sh put it)
R=$GRAFT_REPO_ROOT; TAG=${1:-rxx}
OUT=$(realpath -m "${2:-$R/records_out}"); mkdir -p "$OUT"
$R/tools/profile_round.sh > "$OUT/prof_round.log" 2>&1
$R/tools/profile_shapes.sh > "$OUT/prof_shapes.log" 2>&1
$R/tools/profile_queue_mode.sh ${TAG}q > "$OUT/prof_queue.log" 2>&1
cd $R
python3 bench.py --full > "$OUT/${TAG}_bench_default.log" 2> "$OUT/${TAG}_bench_default.err"
tools/sweep_round.sh 2>&1 | grep "^|" > "$OUT/${TAG}_sweep.log"
if [ -f radiosaber_amd/libradiosaber_hip_stamps.so ]; then
  export RS_HIP_LIB=radiosaber_amd/libradiosaber_hip_stamps.so
  (RS_JIT_EXTRA="-DRS_STAMPS" python3 tools/phase_stamps.py --jit --ttis 400
   RS_JIT_EXTRA="-DRS_STAMPS -DRS_STAMPS_HOLD" python3 tools/phase_stamps.py --jit --hold --ttis 400 | grep "hold:"
   RS_JIT_EXTRA="-DRS_STAMPS" python3 tools/phase_stamps.py --jit --ttis 400 --sched 8
   RS_JIT_EXTRA="-DRS_STAMPS" python3 tools/phase_stamps.py --jit --ttis 400 --rbgs 64 --rbg-size 8) 2>&1 | grep -v "^    -" > "$OUT/${TAG}_stamps_final.log"
fi
cut -c1-150 "$OUT/${TAG}_bench_default.log"
