# Build diagnostic kernel variants for scripts/ab_probe.py and the other probes:
# build/libraftsim_<name>.so with extra -D flags (csrc/device.hpp lists the switches). Every variant
# is a RS_DIAG_BUILD: tagged "diag", refused by raftsim.check_build, loaded through RAFTSIM_LIB.
# Usage: bash scripts/build_variants.sh name1 "-DFLAG=1 ..." name2 "..." ...
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/raft-simulation_amd/csrc
mkdir -p "$R/raft-simulation_amd/build"
JOBS=16          # concurrent compiles at most
pids=()
rc=0
reap() { wait "$1" || rc=1; }     # a failed variant fails the script
while [ $# -ge 2 ]; do
  if [ ${#pids[@]} -ge $JOBS ]; then
    reap "${pids[0]}"
    pids=("${pids[@]:1}")
  fi
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -DRS_DIAG_BUILD $2 \
    -o "$R/raft-simulation_amd/build/libraftsim_$1.so" $C/tick_kernel.hip $C/steady_kernel.hip $C/storm_kernel.hip $C/violations_kernel.hip $C/census_kernel.hip $C/audit_kernel.hip $C/raftsim.hip &
  pids+=($!)
  shift 2
done
for p in "${pids[@]}"; do reap "$p"; done
exit $rc
