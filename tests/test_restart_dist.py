"""dist.reduce_restarts on CPU: gloo, world_size 2 and 1. Each rank restarts the halted nodes of
its cluster shard on the oracle backend (raftsim.restart_by_writes) and the ranks all-reduce the
count; the result must equal the count of one process holding every cluster."""
import gloo
import pairing
import raftsim
from cases import cfg_of

TOTAL, TICKS = 48, 20000


def _restarted(off, cnt):
    cfg = dict(cfg_of("crash_storm_clients", cnt), cluster_offset=off)
    with pairing.closing(pairing.oracle(cfg, threads=2, ticks=TICKS)) as (h,):
        halted = {}
        for i, r in enumerate(h.read_nodes()):
            if r["fault"]:
                halted.setdefault(i // h.N, []).append(i % h.N + 1)
        return sum(raftsim.restart_by_writes(h, c, ids) for c, ids in halted.items())


def _worker(rank, world):
    from raftsim import dist as rdist

    mine = _restarted(*rdist.shard(TOTAL, rank, world))
    return {"mine": mine, "reduced": rdist.reduce_restarts(mine)}


def test_sharded_restart_count_equals_single_process(tmp_path):
    whole = _restarted(0, TOTAL)
    assert whole > 0
    for world in (2, 1):
        got = gloo.spawn(_worker, world, tmp_path / f"r{world}.json")
        assert got["reduced"] == whole, world
        assert (got["mine"] < whole) == (world == 2)
