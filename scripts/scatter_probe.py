"""Cost of raft_scatter_write against the per-node write loop ("Scatter").

  python scripts/scatter_probe.py c3      C3 shape, 131,072 x 5 at tick 200k: the first 4,096
                                          clusters of audit_select(any=("diverged",)), every
                                          required part, scattered back into the handle at their
                                          own ids; then one record to all 131,072 clusters
  python scripts/scatter_probe.py c4_n9   C4-N9, 1,024 x 9 at tick 110k: all 1,024 clusters

Per measurement: kernel ms (raftsim_diag_scatter_ms) and wall ms around scatter(), best of the
last three of four calls, and GB/s of pack bytes; the same for the gather that makes the pack
(raftsim_diag_gather_ms). The baseline is the loop a user writes without
the scatter for the same clusters -- restore_cluster's call sequence (set_tick, write_nodes,
write_clusters, N x write_arena, 2N x write_queue, N x write_commit_stream) as bare ctypes calls
on views of the pack's bytes made beforehand, so that no Python conversion is timed. One JSON line
per measurement. One process per handle."""
import ctypes as C
import time

import numpy as np

from probe import best, emit, open_sim, parser, workload
from raftsim import _abi  # noqa: E402  (on the path once probe is imported)

PARTS = ("cluster", "nodes", "queues", "arenas", "streams")


def scatter_cost(name, sim, pack, clusters, records=None):
    def call():
        sim.scatter(pack, clusters, records)
        return sim.last_scatter_ms()

    kernel, wall = best(call)
    n = len(clusters)
    mb = n * pack.layout["stride"] / 1e6
    emit({"what": name, "targets": n, "records": len(pack), "stride": pack.layout["stride"],
          "written_MB": round(mb, 1), "kernel_ms": round(kernel, 4),
          "kernel_GBps": round(mb / kernel, 1), "wall_ms": round(wall, 3),
          "wall_GBps": round(mb / wall, 2)})
    return wall


def gather_cost(name, sim, ids, parts):
    """The gather of the same pack: kernel ms (raftsim_diag_gather_ms) and wall ms, as above."""
    packs = []

    def call():
        packs[:] = [sim.gather(ids, parts=parts)]
        return sim.last_gather_ms()

    kernel, wall = best(call)
    mb = len(ids) * packs[0].layout["stride"] / 1e6
    emit({"what": name, "records": len(ids), "stride": packs[0].layout["stride"],
          "read_MB": round(mb, 1), "kernel_ms": round(kernel, 4),
          "kernel_GBps": round(mb / kernel, 1), "wall_ms": round(wall, 3)})
    return packs[0]


def write_loop(sim, pack):
    """restore_cluster's calls for every cluster of the pack, into the cluster it came from."""
    f, h, N, Q, A, SC = sim._fns, sim._h, pack.N, pack.Q, pack.A, pack.SC
    views = []
    for i, c in enumerate(pack.clusters):
        q = pack.part(i, "queues")
        ar = pack.part(i, "arenas")
        st = pack.part(i, "streams") if SC else None
        nodes = pack.nodes[i]
        views.append((
            c, nodes, _abi.Cluster.from_buffer(pack.part(i, "cluster")),
            [(_abi.Entry * A).from_buffer(ar, k * A * 8) for k in range(N)],
            [((_abi.Msg * Q).from_buffer(q, (k * 2 + w) * Q * 32),
              nodes[k].res_count if w else nodes[k].req_count) for k in range(N) for w in (0, 1)],
            [((C.c_uint32 * SC).from_buffer(st, k * SC * 4), min(nodes[k].commit_count, SC))
             for k in range(N)] if SC else []))
    calls = 0
    t0 = time.perf_counter()
    for c, nodes, cl, arenas, queues, streams in views:
        rc = f["set_tick"](h, pack.tick)
        rc |= f["write_nodes"](h, c, 1, nodes)
        rc |= f["write_clusters"](h, c, 1, C.byref(cl))
        for k, a in enumerate(arenas):
            rc |= f["write_arena"](h, c, k + 1, a, A)
        for j, (m, cnt) in enumerate(queues):
            rc |= f["write_queue"](h, c, j // 2 + 1, j % 2, m, cnt)
        for k, (s, cnt) in enumerate(streams):
            rc |= f["write_commit_stream"](h, c, k + 1, s, cnt)
        assert rc == 0, (c, f["last_error"]())
        calls += 3 + len(arenas) + len(queues) + len(streams)
    return calls, (time.perf_counter() - t0) * 1e3


def main(argv=None):
    p = parser(__doc__)
    p.add_argument("which", nargs="?", default="c3", choices=("c3", "c4_n9"))
    which = p.parse_args(argv).which
    if which == "c3":
        sim = open_sim(**workload("c3"))
        ticks, take = 200000, 4096
    else:
        sim = open_sim(**workload("c4_n9", 1024))
        ticks, take = 110000, 1024
    for _ in range(ticks // 10000):
        sim.step_async(10000)
    sim.sync()
    total, recs = sim.audit_select(any=("diverged",), limit=take)
    ids = [r["cluster"] for r in recs]
    ids += [c for c in range(sim.C) if c not in set(ids)][:take - len(ids)]   # (fewer diverged)
    emit({"what": f"{which}: handle", "tick": sim.tick, "diverged": total, "clusters": len(ids)})
    parts = [p for p in PARTS if p != "streams" or sim.config.commit_stream_cap]
    pack = gather_cost(f"{which}: the gather of these {take} clusters", sim, ids, parts)
    want = sim.digest()
    wall = scatter_cost(f"{which}: {take} clusters back to their ids", sim, pack, ids)
    assert np.array_equal(sim.digest(), want)
    calls, loop_ms = write_loop(sim, pack)
    assert np.array_equal(sim.digest(), want)
    emit({"what": f"{which}: the write loop for the same clusters", "calls": calls,
          "wall_ms": round(loop_ms, 1), "us_per_call": round(loop_ms * 1e3 / calls, 1),
          "loop_over_scatter": round(loop_ms / wall, 1)})
    if which == "c3":
        n = sim.C
        scatter_cost("c3: one record to 131,072 clusters", sim, pack, np.arange(n),
                     np.zeros(n, dtype=np.int64))
        assert (sim.digest() == want[ids[0]]).all()
    sim.close()


if __name__ == "__main__":
    main()
