"""dist.reduce_audit on CPU: gloo, world_size 2 and 1. Each rank takes the audit of its cluster
shard (tests/audit_oracle.py on the oracle backend, the dict Simulator.audit returns) and the
ranks all-reduce it; the result must equal the audit of one process holding every cluster."""
import audit_oracle as ao
import gloo
from cases import CASES

# few clusters with diverged and identical logs and common prefixes of several lengths
CFG = dict(CASES["spec_arena_odd"])
TOTAL, TICKS = 61, 1500


def _shard_audit(off, cnt):
    return ao.oracle_at(dict(CFG, n_clusters=cnt, cluster_offset=off), (TICKS,))[0][0]


def _worker(rank, world):
    from raftsim import dist as rdist

    mine = _shard_audit(*rdist.shard(TOTAL, rank, world))
    red = rdist.reduce_audit(mine)
    return {"reduced": red, "keys": [list(mine), list(red)]}


def test_sharded_audit_equals_single_process(tmp_path):
    whole = _shard_audit(0, TOTAL)
    # the run has something in every kind of field, so a field reduced with the wrong operator
    # (a maximum summed, a minimum taken as a maximum) shows
    halves = [_shard_audit(0, 30), _shard_audit(30, 31)]
    assert whole["by_class"]["diverged"] and whole["by_class"]["identical"]
    assert whole["agree_min"] < whole["agree_max"] and whole["diverge_index_min"] is not None
    assert whole["commit_diverge_index_min"] is None           # a minimum nobody has stays None
    assert any(h[k] != whole[k] for h in halves for k in ("agree_max", "agree_min"))
    for world in (2, 1):
        got = gloo.spawn(_worker, world, tmp_path / f"r{world}.json")
        assert got["reduced"] == whole, world
        assert got["keys"][0] == got["keys"][1] == list(whole)       # the dict keeps its order
    assert whole["entries"] == sum(h["entries"] for h in halves)
    assert whole["agree_max"] == max(h["agree_max"] for h in halves)
    assert whole["clusters"] == TOTAL
