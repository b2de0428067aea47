"""The steady kernel (steady_kernel.hip) on the exact thresholds of its fast paths: the configs
of steady_edges.edge_cfg put every inequality of the certified paths' and the closed-form init
election's guards at equality, or one below it. Everything here compares the GPU with the C
oracle after every launch (steady_pair.same: digests, counters and the raw node
records of every cluster). test_steady_edge_witness.py shows on the oracle alone that these runs
contain the ties the thresholds are about. Fault-free, client-free configs of 199 clusters."""
import pytest

import pairing
import steady_edges as se
from steady_pair import launch

pytestmark = pytest.mark.gpu

TPL = 16384         # ticks_per_launch: every step below is one launch (the longest is 300P)


def set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("RAFTSIM_STEADY", raising=False)
    else:
        monkeypatch.setenv("RAFTSIM_STEADY", mode)


SCHEDULE = [(n, d, "corner", m) for n in (2, 3, 4, 5) for d in (1, 2, 3) for m in ("always", "never")]
SCHEDULE += [(n, d, v, "always") for v in se.VARIANTS if v != "corner"
             for n in (2, 3, 4, 5) for d in (1, 2)]
SCHEDULE += [(n, d, v, "auto") for v in ("corner", "hb=2d") for n, d in ((5, 1), (4, 2))]
SCHEDULE += [(n, 2, v, None) for v in ("corner", "hb=2d", "el-1") for n in (6, 9)]


@pytest.mark.parametrize("nodes,d,variant,mode", SCHEDULE)
def test_threshold_schedule(nodes, d, variant, mode, monkeypatch):
    """From init-node: one launch of 300P ticks (the elections), 2P + 2 single-tick launches (every
    phase of a round starts and ends a launch, and every tie lands on a launch's first and on its
    last tick), then launches of P - 1, P, P + 1, 2P - 1, 7P + 3 and 200P + 1 ticks. mode None:
    N = 6 and 9 have no steady kernel; the general LITE instance meets the same ties.

    At `corner` a settled cluster holds every certificate condition at equality, so the steady
    kernel owes it the certified path: the last launch's bails may not exceed the clusters the
    oracle shows unsettled before it by more than auto mode's own tolerance of 1/16 of the
    clusters. More bails mean a certificate test is off by one on its conservative side, which no
    state comparison can see. Observed on the MI355X: bails == unsettled + steady_edges.deposed in
    every case (0 in nine of the twelve (nodes, d); 1 at (3, 3), 4 at (4, 1), 3 at (5, 1)): no
    settled cluster bails for a threshold."""
    set_mode(monkeypatch, mode)
    cfg, P = se.edge_cfg(nodes, d, variant)
    with pairing.pair(cfg, dict(ticks_per_launch=TPL)) as (g, r):
        launch(g, r, 300 * P, "election launch", mode)
        for i in range(2 * P + 2):
            launch(g, r, 1, f"single tick {i}", mode)
        unsettled = 0
        for nt in (P - 1, P, P + 1, 2 * P - 1, 7 * P + 3, 200 * P + 1):
            unsettled = se.settled(r)[0]
            launch(g, r, nt, f"launch of {nt}", mode)
        if variant == "corner" and mode is not None:
            bails = g.diag_last_bails()
            print(f"N={nodes} d={d} corner {mode}: last launch bails {bails}, oracle unsettled "
                  f"{unsettled} before it, {se.settled(r)[0]} after, deposed leaders with "
                  f"leader-state in {se.deposed(r)} settled clusters")
            assert bails <= unsettled + se.C_EDGE // 16


@pytest.mark.parametrize("nodes,d", [(5, 1), (4, 2), (2, 3)])
def test_host_written_ties(nodes, d, monkeypatch):
    """Deadlines written by the host onto the thresholds' ties, at `corner`, in one cluster of
    each wave: a follower's on the arrival of its next append-entries (P1: the message wins) and
    one tick before it (the timer wins); the leader's on the next tick to run and the one after.
    Each write is followed once by a 1-tick launch and once by one of P + 1 ticks, then by 3P
    single ticks. The write clears the cluster's certificate, so its wave leaves the line-0 path
    with 63 certified clusters in it."""
    set_mode(monkeypatch, "always")
    cfg, P = se.edge_cfg(nodes, d, "corner")
    for name, write in se.WRITES.items():
        for nt in (1, P + 1):
            what = f"{name}, launch of {nt}"
            with pairing.pair(cfg, dict(ticks_per_launch=TPL), threads=1) as (g, r):
                launch(g, r, 300 * P, f"{what}: election launch", "always")
                for i in range(6):
                    launch(g, r, 1, f"{what}: settle {i}", "always")
                for c in se.WRITTEN:
                    assert write(g, c) == write(r, c), (what, c)
                launch(g, r, nt, what, "always")
                for i in range(3 * P):
                    launch(g, r, 1, f"{what}: tick {i} after", "always")


REWRITTEN = (0, 64, 128, 192)      # the first cluster of each wave of the 199


@pytest.mark.parametrize("nodes", [2, 5])
def test_general_path_round_in_progress(nodes, monkeypatch):
    """The general path's fixed-point branch with a round in progress at t0 (append-entries in
    flight, responses cut), at `corner` with d = 1. Before every launch the host rewrites one
    settled cluster of each wave with the node records just read from it: the write changes nothing
    the oracle can see and clears the cluster's certificate, so every wave loads all its lines and
    takes the general path, where the rewritten cluster is at the fixed point in whatever phase of
    its round the launch starts. (A read resolves a deferred draw and the write stores the exact
    deadline: test_gpu_steady_line0's nodes_same, the same state to the oracle.) After the
    elections and a launch of 2P ticks: 2P + 2 single-tick launches, then launches of P - 1, P + 1
    and 3P + 1 ticks. No launch may bail more clusters than the oracle shows unsettled before it,
    within the corner bound of test_threshold_schedule: a rewritten cluster that bailed for a
    threshold of this branch would still compare equal."""
    set_mode(monkeypatch, "always")
    cfg, P = se.edge_cfg(nodes, 1, "corner")
    with pairing.pair(cfg, dict(ticks_per_launch=TPL), threads=1) as (g, r):
        launch(g, r, 300 * P, "election launch", "always")
        launch(g, r, 2 * P, f"launch of {2 * P}", "always")
        for i, nt in enumerate([1] * (2 * P + 2) + [P - 1, P + 1, 3 * P + 1]):
            unsettled = se.settled(r)[0]
            for c in REWRITTEN:
                se.leader_of(r, c)                   # settled: at the fixed point, in some phase
                for be in (g, r):
                    be.write_nodes(c, be.read_nodes_raw(c, 1))
            launch(g, r, nt, f"launch {i} of {nt}", "always")
            bails = g.diag_last_bails()
            print(f"N={nodes} launch {i} of {nt}: bails {bails}, oracle unsettled {unsettled} "
                  "before it")
            assert bails <= unsettled + se.C_EDGE // 16, (i, nt)


@pytest.mark.parametrize("variant", ["Q2F", "Q2F-1"])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("nodes", [2, 3, 4, 5])
def test_first_launch_cuts_the_election(nodes, d, variant, monkeypatch):
    """The closed-form init election, cut by the first launch's end at every event: the initial
    deadlines lie in [P, 2P) and an election's script ends at most 4d + 2F ticks after the first
    timer, so first launches of every length nt in [P, 2P + 4d + 2F + 3) end before, inside and
    after it for some cluster (tlast < tend at equality), with the ring condition Q >= 2F at
    equality (Q2F) and one below it (Q2F-1). A fresh pair of handles per nt: one launch of nt
    ticks, one of 3P. Every nt is run, for d = 2 as well (the longest case takes 0.2 s on the
    MI355X). A loop, not parameters: a failure names the first nt that fails.

    The second launch is where this test found a bug: an election that the first launch's end
    cut leaves the new leader's responses queued, the first round after an election runs a tick
    late at N = 4 and 5 with d = 1
    (test_steady_edge_witness.test_first_round_after_election_runs_late), and the steady kernel's
    general path, having drained those responses, continued the cluster from the fixed point past
    a follower's timeout."""
    set_mode(monkeypatch, "always")
    cfg, P = se.edge_cfg(nodes, d, variant)
    F = nodes - 1
    for nt in range(P, 2 * P + 4 * d + 2 * F + 3):
        with pairing.pair(cfg, dict(ticks_per_launch=TPL), threads=1) as (g, r):
            launch(g, r, nt, f"first launch of {nt}", "always")
            launch(g, r, 3 * P, f"launch of {3 * P} after a first one of {nt}", "always")
