"""The steady kernel's line-0 path (steady_kernel.hip, device.hpp "strong certificate"): a cluster
the certified path left on the fixed point's schedule is run from the first 128-B line of its
block alone. Everything here compares the GPU with the C oracle after every step: digests,
counters, and the node records of every cluster. Fault-free, client-free configs."""
import numpy as np
import pytest

import helpers
import pairing
from cases import C_CUT, cut_cfg
from raftsim import _abi
from steady_pair import elected, step

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("nodes", [2, 3, 4, 5])
def test_every_cut_phase(nodes, d):
    """Launch ends in every phase of a round, entering and leaving a launch: no round in progress,
    append-entries in flight, each count of responses cut. 3P single-tick launches, then launches
    of P - 1, P, P + 1 and 7P + 3 ticks. Every launch takes the steady kernel."""
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, threads=1) as (g, r):
        elected(g, r, P)
        for i in range(3 * P):
            step(g, r, 1, f"single tick {i}")
            assert g.diag_last_bails() >= 0, i
        for nt in (P - 1, P, P + 1, 7 * P + 3):
            step(g, r, nt, f"launch of {nt}")
            assert g.diag_last_bails() >= 0, nt


def test_default_timers():
    """The headline's shape at 1/16 size: default timers, six 10,000-tick steps, three of 1,000."""
    cfg = dict(n_clusters=4096, nodes=5, seed=42)
    with pairing.pair(cfg, idle_skip=True) as (g, r):
        for i, nt in enumerate([10000] * 6 + [1000] * 3):
            step(g, r, nt, f"step {i} of {nt}")
        assert g.diag_last_bails() == 0


def _leader(be, c):
    return next(i for i, n in enumerate(be.read_nodes(c, 1)) if n["role"] == 2)


def _op_nodes_same(be, c):
    be.write_nodes(c, be.read_nodes_raw(c, 1))


def _op_nodes_deadline(be, c):
    raw = be.read_nodes_raw(c, 1)
    lead = next(i for i in range(be.N) if raw[i].role == 2)
    raw[(lead + 1) % be.N].deadline = be.tick + 1       # a follower about to time out
    be.write_nodes(c, raw)


def _op_queue(be, c):
    """One more empty append-entries from the leader into a follower's REQ ring."""
    lead = _leader(be, c)
    fol = (lead + 1) % be.N
    term = be.read_nodes(c, 1)[lead]["current_term"]
    q = [list(m) for m in be.read_queue(c, fol + 1, 0)]
    arr = max([be.tick] + [m[0] for m in q])
    be.write_queue(c, fol + 1, 0, q + [[arr, 2 | (lead + 1) << 3, term, 0, 0, 0, 0, 0]])


def _op_cluster(be, c):
    be.write_clusters(c, be.read_clusters(c, 1))


def _op_set_tick(be, c):
    be.set_tick(be.tick + 5)


OPS = dict(nodes_same=_op_nodes_same, nodes_deadline=_op_nodes_deadline, queue=_op_queue,
           cluster=_op_cluster, set_tick=_op_set_tick)


@pytest.mark.parametrize("general_first", [False, True])
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("nodes,d", [(5, 2), (4, 1)])
def test_certificate_cleared(nodes, d, op, general_first):
    """Host writes between steady launches clear the certificate (both forms live in one word): the
    written cluster runs through the general tick body, the rest of its wave through the two-line
    paths, and the GPU stays the oracle's at every phase of the round. general_first: the write
    follows a launch of the general kernel (auto mode's cool-down after many bails, provoked by
    timing out a follower in each of 20 clusters), whose write-back clears certificates too."""
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, threads=1) as (g, r):
        elected(g, r, P)
        if general_first:
            for be in (g, r):
                for c in range(20, 40):
                    _op_nodes_deadline(be, c)
            seen = False
            for i in range(10):
                step(g, r, 1, f"cool-down {i}")
                if g.diag_last_bails() < 0:
                    seen = True
                    break
            assert seen, "no launch took the general kernel"
        for phase in range(P + 1):
            c = (37 * phase + 5) % C_CUT
            for be in (g, r):
                OPS[op](be, c)
            step(g, r, 1, f"{op} at phase {phase}")
        for i in range(2 * P):
            step(g, r, 1, f"after {i}")
        step(g, r, 3 * P + 1, "long launch after")


@pytest.mark.parametrize("nodes,d", [(5, 1), (5, 3), (4, 2)])
def test_mixed_waves(nodes, d):
    """One host-written cluster in each wave before a step: the wave leaves the line-0 path, and its
    other 63 clusters come out as the oracle's."""
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, threads=1) as (g, r):
        elected(g, r, P)
        for phase in range(P + 2):
            for be in (g, r):
                for c in (7, 64 + 63, 128, C_CUT - 1):
                    _op_nodes_same(be, c)
            step(g, r, 1 if phase % 3 else P + 1, f"phase {phase}")
        step(g, r, 5 * P, "after")


def _reserved(be):
    arr = (_abi.Cluster * be.C)()
    be._check(be._fns["read_clusters"](be._h, 0, be.C, arr))
    return np.array([list(x.reserved) for x in arr], dtype=np.uint32)


def test_reserved_words_invisible():
    """The certificate and the leader's term live in the cluster's reserved words: reads return
    them as zero, and the digest does not depend on how the ticks were cut into launches."""
    cfg = dict(n_clusters=1024, nodes=5, seed=9)
    a = helpers.gpu(**cfg, ticks_per_launch=30000)
    b = helpers.gpu(**cfg, ticks_per_launch=1000)
    r = pairing.oracle(cfg, idle_skip=True)
    with pairing.closing(a, b, r):
        a.step(30000)
        for _ in range(30):
            b.step(1000)
        r.step(30000)
        assert a.diag_last_bails() >= 0 and b.diag_last_bails() == 0
        assert not _reserved(a).any() and not _reserved(b).any()
        assert (a.digest() == b.digest()).all()
        pairing.same(a, r, "one launch of 30000")
        assert b.counters() == pairing.same_counters(a, r)
    cfg2, P = cut_cfg(4, 1)
    with pairing.pair(cfg2, threads=1) as (g, r2):
        elected(g, r2, P)
        for i in range(P):
            step(g, r2, 1, f"tick {i}")
            assert not _reserved(g).any()
