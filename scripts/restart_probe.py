"""Cost of restarting halted nodes on the device ("Node restarts").

  python scripts/restart_probe.py [clusters] [ticks] [--out FILE]
      C3 shape, `clusters` x 5 (default 131,072) stepped to `ticks` (default 40,000): its crash
      storm has then halted nodes in most clusters. FILE (default profiles/restart_cost.txt)
      receives the JSON lines that are also printed.

Measured on that handle, each from the same state (a snapshot taken after the storm is cloned back
before every call, outside the timed window): restart_where over the whole handle; the list form
for the same nodes, the list being select()'s records made before; the round trip
restart(select(any=halted)), i.e. the query, its records' copy, the list conversion and the
restart; and restart_where when nothing matches (the scan alone). Per measurement: kernel ms
(raftsim_diag_restart_ms; plus raftsim_diag_census_ms for the round trip) and wall ms around the
call, each the best of the last three of four calls, and the nodes restarted."""
import time
from pathlib import Path

import numpy as np

from probe import ROOT, emit, open_sim, parser, workload
import raftsim  # noqa: E402  (on the path once probe is imported)


def main(argv=None):
    p = parser(__doc__)
    p.add_argument("clusters", nargs="?", type=int, help="default: one GPU's shard of C3")
    p.add_argument("ticks", nargs="?", type=int, default=40000)
    p.add_argument("--out", default=str(ROOT / "profiles" / "restart_cost.txt"))
    args = p.parse_args(argv)
    cfg = workload("c3", args.clusters)
    sim = open_sim(**cfg)
    for _ in range(args.ticks // 10000):
        sim.step_async(10000)
    sim.sync()
    lines = []

    def report(rec):
        lines.append(rec)
        emit(rec)

    total, recs = sim.select(any=["halted"])
    nodes = sum(len(r["halted"]) for r in recs)
    census = sim.census()
    report({"what": "handle", "clusters": cfg["n_clusters"], "nodes": cfg["nodes"], "tick": sim.tick,
            "halted_clusters": total, "halted_nodes": nodes,
            "fault_nodes": census["fault_nodes"]})
    snap = raftsim.snapshot(sim)
    want = None

    def measure(what, call, expect):
        nonlocal want
        out = []
        for _ in range(4):
            raftsim.rollback(sim, snap)
            t0 = time.perf_counter()
            n, kernel = call()
            out.append((kernel, (time.perf_counter() - t0) * 1e3))
            assert n == expect, (what, n, expect)
            d = sim.digest()
            if want is None:
                want = d
            assert np.array_equal(d, want), what          # every form leaves the same state
        report({"what": what, "nodes_restarted": expect,
                "kernel_ms": round(min(k for k, _ in out[-3:]), 4),
                "wall_ms": round(min(w for _, w in out[-3:]), 3)})

    measure("restart_where over the whole handle",
            lambda: (sim.restart_where(), sim.last_restart_ms()), nodes)
    measure("the list form for the same nodes (select()'s records made before)",
            lambda: (sim.restart(recs), sim.last_restart_ms()), nodes)

    def round_trip():
        n = sim.restart(sim.select(any=["halted"])[1])
        return n, sim.last_census_ms() + sim.last_restart_ms()

    measure("restart(select(any=halted)): query, copy, list and restart", round_trip, nodes)
    out = []
    for _ in range(4):                                    # nothing is halted any more
        t0 = time.perf_counter()
        assert sim.restart_where() == 0
        out.append((sim.last_restart_ms(), (time.perf_counter() - t0) * 1e3))
    report({"what": "restart_where when nothing matches (the scan alone)", "nodes_restarted": 0,
            "kernel_ms": round(min(k for k, _ in out[-3:]), 4),
            "wall_ms": round(min(w for _, w in out[-3:]), 3)})
    snap.close()
    sim.close()
    import json
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
