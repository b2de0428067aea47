"""The N>1 path on the GPU: two ranks (one process each, both on the box's one MI355X, gloo for the
host-side reduction -- RCCL needs one GPU per rank) each run their contiguous cluster shard through
libraftsim.so and all-reduce the counters exactly as bench.py does; digests and reduced counters
must equal one handle simulating every cluster (Philox is keyed by the global cluster id)."""
from pathlib import Path

import numpy as np
import pytest

import gloo
import helpers

pytestmark = pytest.mark.gpu

CFG = dict(nodes=5, seed=17, client_ppm=80000, client_period=16384, client_burst=2048,
           client_redirects=4, drop_ppm=100000, dup_ppm=10000, dmin=1, dmax=50,
           part_ppm=100000, log_cap=256)
TOTAL, STEPS = 20000, 3


def _worker(rank, world, out):
    import raftsim
    from raftsim import dist as rdist

    off, cnt = rdist.shard(TOTAL, rank, world)
    with raftsim.Simulator(n_clusters=cnt, cluster_offset=off, **CFG) as sim:
        for _ in range(STEPS):
            sim.step(10000)
        np.save(Path(out) / f"digest_{rank}.npy", sim.digest())
        return rdist.reduce_counters(sim.counters())


def test_gpu_two_ranks_equal_one_handle(tmp_path):
    got = gloo.spawn(_worker, 2, tmp_path / "counters.json", str(tmp_path))
    whole = helpers.gpu(n_clusters=TOTAL, **CFG)
    for _ in range(STEPS):
        whole.step(10000)
    dg = np.concatenate([np.load(tmp_path / f"digest_{r}.npy") for r in range(2)])
    assert np.array_equal(dg, whole.digest())
    assert got == whole.counters() and got["client_injected"] > 0
