"""BASELINE configs 3-5 on one MI355X next to the CPU oracle (one GPU call; a JSON line per result).

c3      one GPU's shard of config 3 (131,072 of the 1,048,576 five-node clusters): drop 10 %, dup 1 %,
        delay U[1,50], partitions (p 0.1 per 1000-tick epoch), bursty client (SIM_SPEC D14/D15) at
        one client-set per 100 ticks on average. bench.py times the whole 1M clusters.
c4_n7, c4_n9   config 4: 16,384 clusters of 7 / 9 nodes with 4096-entry logs and a bursty client
        (500,000 ppm in 2048 of every 8192 ticks, redirects followed) run for 110k ticks: log
        growth, 1000+-entry AppendEntries batches, OVERFLOW halts; kernel time per 10k-tick step.
c4_spec_n9     the same on the Spec-Raft control (majority commit through the sorting network).
c5      config 5: config 3's faults and client with the vote granted without the log check, on the
        faithful model (flag 1) and on the Spec-Raft control (flags 3); ticks until the first safety
        violation anywhere in the shard, GPU wall time next to the CPU oracle's on the same
        clusters (all host threads, idle-tick skipping), bit-exactness, and the Spec-Raft control
        (flag 2) run for as many ticks: leaders, commits, violations.
GPU rates are node-ticks/s over steps of 10k ticks after a warm-up (state resident in HBM)."""
import time

import numpy as np

import probe
from probe import emit
import helpers  # noqa: E402  (tests/: on the path once probe is imported)
import pairing  # noqa: E402


def cpu_oracle(cfg, clusters, ticks_list):
    r = pairing.oracle(dict(cfg, n_clusters=clusters), idle_skip=True)
    dts = []
    for t in ticks_list:
        t0 = time.perf_counter()
        r.step(t)
        dts.append(time.perf_counter() - t0)
    return r, dts


def node_census(sim):
    import ctypes
    raw = sim.read_nodes_raw()
    b = np.frombuffer(raw, dtype=np.uint8).reshape(len(raw), ctypes.sizeof(raw[0]))
    log_len = b[:, 20:24].copy().view(np.uint32).ravel()
    return {"leaders_running": int(((b[:, 0] == 2) & (b[:, 3] == 0)).sum()),
            "halted_nodes": int((b[:, 3] != 0).sum()), "max_log_len": int(log_len.max())}


def c3_shard():
    C3 = probe.workload("c3")
    n, clusters = C3["nodes"], C3["n_clusters"]
    g = probe.open_sim(**C3)
    g.step(20000)
    t0 = time.perf_counter()
    for _ in range(4):
        g.step(10000)
    gdt = time.perf_counter() - t0
    _, dts = cpu_oracle(C3, 8192, [20000, 40000])
    emit({"config": "c3_shard", "gpu_clusters": clusters,
          "gpu_node_ticks_per_s": clusters * n * 40000 / gdt,
          "cpu_clusters": 8192, "cpu_threads": helpers.cpu_threads(),
          "cpu_node_ticks_per_s": 8192 * n * 40000 / dts[1],
          "gpu_counters": {k: v for k, v in g.counters().items() if v}, **node_census(g)})


def c4(name, workload, total=110000):
    cfg = probe.workload(workload)
    nodes, clusters, variant = cfg["nodes"], cfg["n_clusters"], cfg.setdefault("variant_flags", 0)
    g = probe.open_sim(**cfg)
    t_all = time.perf_counter()
    kms = [launch.ms for launch in probe.launches(g, total // probe.TICKS)]
    gdt = time.perf_counter() - t_all
    cpu_n = 512
    r, dts = cpu_oracle(cfg, cpu_n, [total])
    same = bool((g.digest(0, cpu_n) == r.digest()).all())
    emit({"config": name, "variant_flags": variant, "clusters": clusters, "ticks": total,
          "gpu_node_ticks_per_s": clusters * nodes * total / gdt,
          "kernel_ms_per_10k_ticks": [round(x, 3) for x in kms],
          "cpu_clusters": cpu_n, "cpu_threads": helpers.cpu_threads(),
          "cpu_node_ticks_per_s": cpu_n * nodes * total / dts[0], "first_clusters_bit_exact": same,
          "gpu_counters": {k: v for k, v in g.counters().items() if v}, **node_census(g)})


def first_violation(sim, chunk, max_ticks):
    t0 = time.perf_counter()
    done = 0
    while done < max_ticks:
        sim.step(chunk)
        done += chunk
        fv = sim.counters()["first_violation_tick"]
        if fv is not None:
            return fv, done, time.perf_counter() - t0
    return None, done, time.perf_counter() - t0


def time_to_violation(name, flags, chunk=1000, max_ticks=200000):
    cfg = probe.workload("c3", variant_flags=flags)
    clusters = cfg["n_clusters"]
    g = probe.open_sim(**cfg)
    gfv, gdone, gdt = first_violation(g, chunk, max_ticks)
    r = pairing.oracle(cfg, idle_skip=True)
    cfv, cdone, cdt = first_violation(r, chunk, gdone)
    emit({"config": name, "variant_flags": flags, "clusters": clusters,
          "first_violation_tick": gfv, "ticks_simulated": gdone, "gpu_wall_s": gdt,
          "cpu_first_violation_tick": cfv, "cpu_wall_s": cdt, "cpu_threads": helpers.cpu_threads(),
          "bit_exact": bool(gfv == cfv and cdone == gdone and (g.digest() == r.digest()).all()),
          "gpu_counters": {k: v for k, v in g.counters().items() if v}})
    return gdone


def main(argv=None):
    p = probe.parser(__doc__)
    p.add_argument("names", nargs="*", metavar="CONFIG", help="of c3, c4, c5 (default: all)")
    names = p.parse_args(argv).names or ["c3", "c4", "c5"]
    if "c3" in names:
        c3_shard()
    if "c4" in names:
        c4("c4_n7", "c4_n7")
        c4("c4_n9", "c4_n9")
        c4("c4_spec_n9", "c4_spec")
    if "c5" in names:
        ticks = time_to_violation("c5_faithful_nolog", 1)
        ticks = max(ticks, time_to_violation("c5_spec_nolog", 3))
        ctl = probe.open_sim(**probe.workload("c3", variant_flags=2))
        t0 = time.perf_counter()
        ctl.step(ticks)
        c = ctl.counters()
        emit({"config": "c5_spec_control", "variant_flags": 2, "clusters": ctl.C,
              "ticks_simulated": ticks, "gpu_wall_s": time.perf_counter() - t0,
              "first_violation_tick": c["first_violation_tick"], "leaders": c["leaders"],
              "entries_applied": c["entries_applied"],
              "violations": c["viol_election"] + c["viol_log"] + c["viol_complete"],
              **node_census(ctl)})


if __name__ == "__main__":
    main()
