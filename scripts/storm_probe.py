"""First launches of a workload with the storm ticks on the lane-per-cluster storm kernel or on the
lane-per-node STORM body (diagnostic): launch times, the storm kernel's leftover count, and whether
both paths give the same state. The product library takes no override of that choice: this needs a
diagnostic variant (scripts/build_variants.sh, e.g. `build_variants.sh diag ""`), loaded through
RAFTSIM_LIB, which reads RAFTSIM_STORM_MIN_CLUSTERS.
Usage: RAFTSIM_LIB=raft-simulation_amd/build/libraftsim_diag.so \\
       python scripts/storm_probe.py WORKLOAD CLUSTERS"""
import os

import probe


def main(argv=None):
    p = probe.parser(__doc__)
    p.add_argument("workload", choices=list(probe.bench.WORKLOADS))
    p.add_argument("clusters", type=int)
    args = p.parse_args(argv)
    wl, c = args.workload, args.clusters
    probe.require_diag(probe.raftsim.LIB_PATH, "storm_probe", "ignores RAFTSIM_STORM_MIN_CLUSTERS")
    digests = []
    for mode in ("body", "kernel"):
        os.environ["RAFTSIM_STORM_MIN_CLUSTERS"] = "4000000000" if mode == "body" else "1"
        sim = probe.open_sim(**probe.workload(wl, c))
        for i in range(3):
            (r,) = probe.launches(sim, 1)
            print(f"{wl} {c} storm-{mode:6s} step {i} launches {r.launches} avg ms {r.ms:.3f} "
                  f"span ms {r.span:.3f} storm bails {sim.diag_storm_bails()}", flush=True)
        digests.append(sim.digest())
        sim.close()
    print("same state:", bool((digests[0] == digests[1]).all()))


if __name__ == "__main__":
    main()
