"""CPU witness for test_gpu_steady_edges.py: on the C oracle alone, the threshold configs of
steady_edges.edge_cfg reach the states the GPU tests claim to compare -- settled clusters led from
every node position, followers whose election deadline ties with the arrival of an append-entries,
leaders whose heartbeat deadline ties with the arrival of a response, the chaotic side one below
el_base's threshold, and both init-election classes the closed form handles. A change of a seed
or a timer that moves a config off its ties fails here, without a GPU.

The floors asserted are conditions the GPU tests need, not measurements. Measured on the oracle
(199 clusters, a 300P step, then 2P single ticks; ranges over nodes 2..5 x d 1..3):
  corner   0..1 unsettled, the least-used leader position leads >= 23, 35..136 follower ties,
           no leader tie
  hb=2d    0 unsettled, 398 leader ties everywhere
  hb-1     0..2 unsettled
  el-1     15..198 unsettled
  init     single 102..166; tie 31..36 at d = 1, N >= 3

The GPU is only ever compared with the C oracle, so the oracle is compared here with the
independent Python restatement (oracle/pyref.py) on the same edges.
"""
import pytest

import helpers
import pairing
import pyref
import steady_edges as se

GRID = [(n, d) for n in (2, 3, 4, 5) for d in (1, 2, 3)]


def run_witness(nodes, d, variant):
    """(unsettled, led, follower_ties, leader_ties): a 300P step, then 2P single ticks with the
    ties summed before each."""
    cfg, P = se.edge_cfg(nodes, d, variant)
    with pairing.oracle(cfg) as r:
        r.step(300 * P)
        unsettled, led = se.settled(r)
        fol = lead = 0
        for _ in range(2 * P):
            f, l = se.ties(r)
            fol += f
            lead += l
            r.step(1)
    print(f"N={nodes} d={d} {variant}: unsettled {unsettled} led {led} follower ties {fol} "
          f"leader ties {lead}")
    return unsettled, led, fol, lead


@pytest.mark.parametrize("nodes,d", GRID)
def test_corner_reaches_follower_ties(nodes, d):
    unsettled, led, fol, _ = run_witness(nodes, d, "corner")
    assert unsettled <= 4
    assert min(led) >= 15, led
    assert fol >= 20


@pytest.mark.parametrize("nodes,d", GRID)
def test_hb_2d_reaches_leader_ties(nodes, d):
    unsettled, _, _, lead = run_witness(nodes, d, "hb=2d")
    assert unsettled <= 4
    assert lead >= 390          # two rounds in almost every cluster


@pytest.mark.parametrize("nodes,d", GRID)
def test_hb_below_threshold_settles(nodes, d):
    assert run_witness(nodes, d, "hb-1")[0] <= 4


@pytest.mark.parametrize("nodes,d", GRID)
def test_el_base_below_threshold_is_chaotic(nodes, d):
    """Halts and re-elections that the catch-up body must run."""
    assert run_witness(nodes, d, "el-1")[0] >= 10


@pytest.mark.parametrize("nodes,d", GRID)
def test_init_election_classes(nodes, d):
    cfg, _ = se.edge_cfg(nodes, d, "corner")
    with helpers.oracle(**cfg) as r:
        k = se.init_classes(r)
    print(f"N={nodes} d={d}: {k}")
    assert sum(k.values()) == se.C_EDGE
    assert k["single"] >= 50
    if d == 1 and nodes >= 3:
        assert k["tie"] >= 20


@pytest.mark.parametrize("nodes,d", [(4, 1), (5, 1)])
def test_first_round_after_election_runs_late(nodes, d):
    """test_gpu_steady_edges.test_first_launch_cuts_the_election: with el_base == P the first
    round after init-node's election runs one tick late at N = 4 and 5 with d = 1, and a follower
    with draw 0 times out one tick before its append-entries. The steady kernel's general path
    once continued such a cluster from the fixed point and missed that timer; these are the
    clusters that showed it. Measured: 60 clusters at N = 4, 54 at N = 5 (none at N = 2, 3 or
    d = 2); the floor asserted is what keeps the GPU test from passing without them."""
    cfg, P = se.edge_cfg(nodes, d, "Q2F")
    hit = set()
    with helpers.oracle(**cfg) as r:
        for _ in range(4 * P):
            hit.update(se.late_round_timeouts(r))
            r.step(1)
    print(f"N={nodes} d={d}: {len(hit)} clusters with a follower's timeout in a late round")
    assert len(hit) >= 20


@pytest.mark.parametrize("nodes,d", [(5, 1), (4, 2), (2, 3)])
def test_host_written_clusters_are_settled_and_tie(nodes, d):
    """test_gpu_steady_edges.test_host_written_ties: the four written clusters are settled when
    they are written, and the written follower deadline is a tie (P1: the message wins) in some of
    them -- where the leader takes no response between the write and its next heartbeat."""
    cfg, P = se.edge_cfg(nodes, d, "corner")
    with helpers.oracle(**cfg) as r:
        r.step(300 * P + 6)
        want = {c: se.write_follower_tie(r, c) for c in se.WRITTEN}
        met = 0
        for _ in range(P + 2 * d + 1):
            t = r.tick
            for c, arr in want.items():
                if arr != t:
                    continue
                fol, now = se.next_ae_arrival(r, c)
                n = r.read_nodes(c, 1)[fol]
                met += now == t and n["deadline"] == t and n["req_count"] > 0
            r.step(1)
    print(f"N={nodes} d={d}: {met} of {len(se.WRITTEN)} written deadlines met their append-entries")
    assert met >= 1


@pytest.mark.parametrize("cluster_offset", [0, 57, 198])
@pytest.mark.parametrize("variant", [v for v in se.VARIANTS if v != "Q2F"])
@pytest.mark.parametrize("nodes,d", GRID)
def test_oracle_equals_python_restatement_on_edges(nodes, d, variant, cluster_offset):
    cfg, P = se.edge_cfg(nodes, d, variant, clusters=1)
    be = helpers.oracle(cluster_offset=cluster_offset, **cfg)
    pc = pyref.PyCluster(helpers.py_config(**cfg), cluster_offset)
    for chunk in range(4):
        for t in range(chunk * 15 * P, (chunk + 1) * 15 * P):
            pc.step(t)
        be.step(15 * P)
        helpers.compare_py_backend(pc, be, 0)
    c = be.counters()
    for k, v in pc.cnt.items():
        assert c[k] == v, (k, c[k], v)
    assert c["first_violation_tick"] == pc.first_violation
    be.close()
