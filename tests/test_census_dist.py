"""dist.reduce_census on CPU: gloo, world_size 2 and 1. Each rank takes the census of its cluster
shard (tests/census_oracle.py on the oracle backend, the dict Simulator.census returns) and the
ranks all-reduce it; the result must equal the census of one process holding every cluster."""
import census_oracle as co
import gloo
from cases import CASES

# few clusters with every kind of node: halts, leaders, candidates, queued messages
CFG = dict(CASES["arena_odd"])
TOTAL, TICKS = 61, 1500


def _shard_census(off, cnt):
    return co.oracle_at(dict(CFG, n_clusters=cnt, cluster_offset=off), (TICKS,))[0][0]


def _worker(rank, world):
    from raftsim import dist as rdist

    mine = _shard_census(*rdist.shard(TOTAL, rank, world))
    red = rdist.reduce_census(mine)
    return {"reduced": red, "keys": [list(mine), list(red)]}


def test_sharded_census_equals_single_process(tmp_path):
    whole = _shard_census(0, TOTAL)
    # the run has something in every kind of field, so a field reduced with the wrong operator
    # (a maximum summed, the minimum taken as a maximum) shows
    assert whole["by_class"]["halted"] and whole["by_class"]["one_leader"]
    assert whole["term_min"] < whole["term_max"] and whole["req_queued"] and whole["hwm_max"]
    for world in (2, 1):
        got = gloo.spawn(_worker, world, tmp_path / f"r{world}.json")
        assert got["reduced"] == whole, world
        assert got["keys"][0] == got["keys"][1] == list(whole)       # the dict keeps its order
    halves = [_shard_census(0, 30), _shard_census(30, 31)]
    assert whole["term_sum"] == sum(h["term_sum"] for h in halves)
    assert whole["term_max"] == max(h["term_max"] for h in halves) != sum(
        h["term_max"] for h in halves)
