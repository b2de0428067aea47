"""First launches of a workload with the storm ticks on the lane-per-cluster storm kernel or on the
lane-per-node STORM body (diagnostic): launch times, the storm kernel's leftover count, and whether
both paths give the same state. The product library takes no override of that choice: this needs a
diagnostic variant (scripts/build_variants.sh, e.g. `build_variants.sh diag ""`), loaded through
RAFTSIM_LIB, which reads RAFTSIM_STORM_MIN_CLUSTERS.
Usage: RAFTSIM_LIB=raft-simulation_amd/build/libraftsim_diag.so \\
       python scripts/storm_probe.py WORKLOAD CLUSTERS"""
import ctypes
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "raft-simulation_amd"), str(ROOT)]
import bench  # noqa: E402
import raftsim  # noqa: E402

_lib = ctypes.CDLL(str(raftsim.LIB_PATH))            # (loads without a GPU call)
_lib.raftsim_src_hash.restype = ctypes.c_char_p
if _lib.raftsim_src_hash().decode() != "diag":
    sys.exit(f"storm_probe: {raftsim.LIB_PATH} is not a diagnostic build, so it ignores "
             "RAFTSIM_STORM_MIN_CLUSTERS: build a variant with scripts/build_variants.sh and "
             "pass it through RAFTSIM_LIB")

wl, c = sys.argv[1], int(sys.argv[2])
cfg = bench.WORKLOADS[wl]["cfg"]
digests = []
for mode in ("body", "kernel"):
    os.environ["RAFTSIM_STORM_MIN_CLUSTERS"] = "4000000000" if mode == "body" else "1"
    sim = raftsim.Simulator(n_clusters=c, **cfg)
    for i in range(3):
        sim.step(10000)
        ms, nl = sim.last_step_timing()
        print(f"{wl} {c} storm-{mode:6s} step {i} launches {nl} avg ms {ms:.3f} span ms "
              f"{sim.last_span():.3f} storm bails {sim.diag_storm_bails()}", flush=True)
    digests.append(sim.digest())
    sim.close()
print("same state:", bool((digests[0] == digests[1]).all()))
