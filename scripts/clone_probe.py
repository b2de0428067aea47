"""Cost of raft_clone_write against the host path it replaces ("Clone").

  python scripts/clone_probe.py [clusters] [ticks]    C3 shape, `clusters` x 5 (default 131,072)
                                                      stepped to `ticks` (default 20,000)

Measured on that handle: the respawn (the first half of the clusters cloned onto the second half
in place), one cluster cloned onto every other, a snapshot's fill (every cluster cloned into a
second handle), and for the first 4,096 pairs of the respawn the host path, scatter(gather(...)).
Per measurement: kernel ms (raftsim_diag_clone_ms; the gather's plus the scatter's for the host
path) and wall ms around the call, best of the last three of four calls, and GB/s of state written
(the stride of the record a scatter needs, per target). One JSON line per measurement."""
import time

import numpy as np

from probe import best, emit, open_sim, parser, workload
import raftsim  # noqa: E402  (on the path once probe is imported)
from raftsim import _abi  # noqa: E402


def report(what, n, stride, kernel, wall):
    mb = n * stride / 1e6
    emit({"what": what, "pairs": n, "stride": stride, "written_MB": round(mb, 1),
          "kernel_ms": round(kernel, 4), "kernel_GBps": round(mb / kernel, 1),
          "wall_ms": round(wall, 3), "wall_GBps": round(mb / wall, 2)})


def clone_cost(what, dst, sources, targets, stride, source=None):
    def call():
        dst.clone(sources, targets, source=source)
        return dst.last_clone_ms()

    report(what, len(targets), stride, *best(call))


def main(argv=None):
    p = parser(__doc__)
    p.add_argument("clusters", nargs="?", type=int, help="default: one GPU's shard of C3")
    p.add_argument("ticks", nargs="?", type=int, default=20000)
    args = p.parse_args(argv)
    cfg = workload("c3", args.clusters)
    clusters, ticks = cfg["n_clusters"], args.ticks
    sim = open_sim(**cfg)
    for _ in range(ticks // 10000):
        sim.step_async(10000)
    sim.sync()
    parts = [p for p in _abi.SCATTER_PARTS] + (["streams"] if sim.config.commit_stream_cap else [])
    stride = sim.gather_layout(parts)["stride"]
    half = clusters // 2
    lo, hi = np.arange(half), np.arange(half, 2 * half)
    emit({"what": "handle", "clusters": clusters, "tick": sim.tick, "stride": stride})
    before = sim.digest()
    clone_cost("respawn: the first half onto the second", sim, lo, hi, stride)
    now = sim.digest()
    assert np.array_equal(now[hi], before[lo]) and np.array_equal(now[lo], before[lo])
    take = min(4096, half)

    def host_path():
        pack = sim.gather(lo[:take], parts=parts)
        sim.scatter(pack, hi[:take])
        return sim.last_gather_ms() + sim.last_scatter_ms()

    report(f"the host path for {take} of these pairs: scatter(gather(...))", take, stride,
           *best(host_path))
    clone_cost(f"the same {take} pairs cloned", sim, lo[:take], hi[:take], stride)
    assert np.array_equal(sim.digest(), now)
    clone_cost("one cluster onto every other", sim, np.zeros(clusters - 1, dtype=np.int64),
               np.arange(1, clusters), stride)
    assert (sim.digest() == before[0]).all()
    t0 = time.perf_counter()
    snap = raftsim.snapshot(sim)
    emit({"what": "snapshot(): create and fill a second handle",
          "wall_ms": round((time.perf_counter() - t0) * 1e3, 1)})
    clone_cost("the snapshot's fill: every cluster into the second handle", snap,
               np.arange(clusters), np.arange(clusters), stride, source=sim)
    assert np.array_equal(snap.digest(), sim.digest())
    clone_cost("rollback's copy: every cluster back", sim, np.arange(clusters), np.arange(clusters),
               stride, source=snap)
    snap.close()
    sim.close()


if __name__ == "__main__":
    main()
