"""Per-launch kernel time of a workload's first launches at several cluster counts (diagnostic):
whether the general kernel is bound by its waves' dependent chains (time flat in the cluster
count while the chip has room) or by issue (time proportional to it); with the launches' device
spans, and on any build (--lib), also the single launches from init-node that a PMC pass runs.
Usage: python scripts/scale_probe.py WORKLOAD C1 C2 ... [--lib LIB] [--steps K]   (K = 6)"""
import probe


def main(argv=None):
    p = probe.parser(__doc__)
    p.add_argument("workload", choices=list(probe.bench.WORKLOADS))
    p.add_argument("clusters", nargs="+", type=int, metavar="C")
    p.add_argument("--lib", help="default: the product library")
    p.add_argument("--steps", type=int, default=6)
    args = p.parse_args(argv)
    for c in args.clusters:
        sim = probe.open_sim(args.lib, **probe.workload(args.workload, c))
        recs = probe.launches(sim, args.steps)
        print(f"{args.workload} clusters {c:7d} launch ms " + " ".join(f"{r.ms:7.3f}" for r in recs)
              + "  step span ms " + " ".join(f"{r.span:7.3f}" for r in recs)
              + f"  ({recs[-1].launches} launches per step)", flush=True)
        sim.close()


if __name__ == "__main__":
    main()
