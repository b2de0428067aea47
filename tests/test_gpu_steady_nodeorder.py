"""The line-0 body in node order (steady_kernel.hip, NodeOrder): a wave under strong certificates
keeps its clusters' hashes and deadlines by node, not by follower slot, and what the followers share
as one value each (rs::run_launch and rs::rounds run on it as on FixedPoint). A wrong node/slot mapping shows only for some leader positions, so the configs
here are checked to put a leader in every position. Everything compares the GPU with the C oracle
after every launch: digests, counters, every node record."""
import numpy as np
import pytest

import pairing
from cases import cut_cfg
from steady_pair import elected, step

pytestmark = pytest.mark.gpu


def leaders_by_position(r):
    """How many clusters each node position leads, from the oracle's node records."""
    nodes = r.read_nodes()
    N = r.N
    n = np.zeros(N, dtype=np.int64)
    for c in range(r.C):
        for k in range(N):
            n[k] += nodes[c * N + k]["role"] == 2
    return n


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("nodes", [2, 3, 4, 5])
def test_every_leader_position_every_phase(nodes, d):
    """Every leader position through every phase of a round, entering and leaving cut: P + 2
    launches of P + 1 ticks (the phase at the start moves by one tick each launch; every launch
    holds whole rounds and is cut at both ends), then P + 2 launches of 2P - 1 ticks (the phase moves
    the other way, and K takes both values of the band within a wave)."""
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, threads=1) as (g, r):
        elected(g, r, P)
        lead = leaders_by_position(r)
        print("clusters led by each node position:", lead.tolist())
        assert lead.sum() == r.C and (lead >= 20).all(), lead
        for nt in (P + 1, 2 * P - 1):
            for i in range(P + 2):
                step(g, r, nt, f"launch {i} of {nt} ticks")
                assert g.diag_last_bails() >= 0, (nt, i)


@pytest.mark.parametrize("nodes,d", [(5, 1), (2, 2)])
def test_no_append_entries_in_the_launch(nodes, d):
    """2P single-tick launches, most of which deliver no append-entries: the followers' deadlines
    go back as loaded. Half way, clusters 0 and 198 are written with their own records: their
    waves leave the line-0 body for a launch and come back to it."""
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, threads=1) as (g, r):
        elected(g, r, P)
        for i in range(2 * P):
            if i == P:
                for be in (g, r):
                    for c in (0, 198):
                        be.write_nodes(c, be.read_nodes_raw(c, 1))
            step(g, r, 1, f"single tick {i}")
            assert g.diag_last_bails() >= 0, i


def test_default_timers_small():
    """The headline's own stream, 256 clusters: five launches of 10,000 ticks, no bail at the end."""
    cfg = dict(n_clusters=256, nodes=5, seed=42)
    with pairing.pair(cfg, idle_skip=True) as (g, r):
        for i in range(5):
            step(g, r, 10000, f"step {i}")
        assert g.diag_last_bails() == 0
