"""Quick throughput probe over several configs (one GPU call). Prints one line per config. The
configs are bench.py's workloads at one GPU's size with the differences below: they are older than
the bursty, redirect-following client, so apart from c2 none is the bench workload of its name.
Usage: perf_probe.py [NAME ...] [--check]   (--check: then tests/cases.py's c3_faults against the
oracle)"""
import time

import probe

STEADY_CLIENT = dict(client_period=0, client_burst=0, client_redirects=0)   # no bursts, no redirects
PROBES = {
    # C2 whose election timers never fire: the cost of ticks in which nothing happens
    "idle": lambda: probe.workload("c2", el_base=10 ** 8),
    # C2 as the bench has it (the one probe that is a bench workload)
    "c2": lambda: probe.workload("c2"),
    # C2 with four-slot inboxes: the queue capacity's share of the launch
    "c2_q4": lambda: probe.workload("c2", inbox_cap=4),
    # C3's faults under a steady client at an eighth of the bench's rate, not its bursts
    "c3": lambda: probe.workload("c3", client_ppm=10000, **STEADY_CLIENT),
    # ... at 200 ppm: almost no client work, the faults alone
    "c3_lowclient": lambda: probe.workload("c3", client_ppm=200, **STEADY_CLIENT),
    # C2 with one client-set per million ticks: a client at all takes the launch off the LITE path
    "c2_client1": lambda: probe.workload("c2", client_ppm=1),
    # C3's faults with no client: what the faults cost without log growth
    "c3_noclient": lambda: probe.workload("c3", client_ppm=0, **STEADY_CLIENT),
    # C4-N9's logs under a steady client at half the bench's burst rate: no 1000-entry batches
    "c4_n9": lambda: probe.workload("c4_n9", client_ppm=250000, **STEADY_CLIENT),
}


def main(argv=None):
    p = probe.parser(__doc__)
    p.add_argument("names", nargs="*", metavar="NAME", help=", ".join(PROBES) + " (default: all)")
    p.add_argument("--check", action="store_true")
    args = p.parse_args(argv)
    if set(args.names) - set(PROBES):
        p.error(f"unknown probe in {args.names}: one of {', '.join(PROBES)}")
    for name in args.names or PROBES:
        cfg = PROBES[name]()
        sim = probe.open_sim(**cfg)
        sim.step(probe.TICKS)
        t0 = time.perf_counter()
        ms = probe.launches(sim, 2)[-1].ms
        dt = (time.perf_counter() - t0) / 2
        nt = cfg["n_clusters"] * cfg["nodes"] * probe.TICKS
        c = sim.counters()
        ev = sum(c[k] for k in c if k.startswith("ev_")) / max(1, c["node_ticks"])
        print(f"{name:14s} wall {dt*1e3:8.2f} ms/10k ticks  kernel {ms:8.2f} ms  "
              f"{nt/dt:.3e} node-ticks/s  events/node-tick {ev:.2e}", flush=True)
        sim.close()
    if args.check:
        import cases
        import pairing
        try:
            with pairing.pair(cases.CASES["c3_faults"]) as (g, r):
                pairing.step(g, r, 20000, "perf_probe --check", counters=True)
            print("parity check: OK", flush=True)
        except AssertionError as e:
            print(e)
            print("parity check: MISMATCH", flush=True)


if __name__ == "__main__":
    main()
