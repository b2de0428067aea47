"""Per-launch burst-engine diagnostics of a -DRS_BURST_DIAG=1 build (scripts/build_variants.sh, a
diagnostic build: wrong counters, timing only): engine ticks, engine entries, yields and tick-loop
trips per launch.
Usage: python scripts/burst_diag.py LIB c4_n9 [c4_n7 ...] [--clusters C] [--steps K]"""
import probe

FIELDS = ("dropped", "duplicated", "partitioned", "payload_evicted", "ev_cs")


def main(argv=None):
    p = probe.parser(__doc__)
    p.add_argument("lib", metavar="LIB")
    p.add_argument("workloads", nargs="+", choices=list(probe.bench.WORKLOADS))
    p.add_argument("--clusters", type=int, help="default: the workload's at one GPU")
    p.add_argument("--steps", type=int, default=20)
    args = p.parse_args(argv)
    probe.require_diag(args.lib, "burst_diag", "counts no engine ticks")
    for wname in args.workloads:
        s = probe.open_sim(args.lib, **probe.workload(wname, args.clusters))
        prev = dict.fromkeys(FIELDS, 0)
        for step in range(args.steps):
            (r,) = probe.launches(s, 1)
            c = s.counters()
            d = {k: c[k] - prev[k] for k in FIELDS}
            prev = {k: c[k] for k in FIELDS}
            print(f"{wname} launch {step:2d} {r.ms:8.3f} ms  engine_ticks {d['dropped']:9d} "
                  f"entries {d['duplicated']:8d} yields {d['partitioned']:8d} trips "
                  f"{d['payload_evicted']:9d} ev_cs {d['ev_cs']:9d}", flush=True)
        s.close()


if __name__ == "__main__":
    main()
