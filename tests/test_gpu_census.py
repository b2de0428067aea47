"""The state census on the GPU: Simulator.census and Simulator.select (csrc/census_kernel.hip)
held to tests/census_oracle.py run on the oracle's records, which tests/test_census_abi.py checks
against hand-written clusters and pins the class populations of (every class occurs in the runs
below; the figures are asserted there and in the tests here that name them)."""
import socket

import numpy as np
import pytest

import census_oracle as co
import helpers
import pairing
from cases import CASES, PARITY, cfg_of
from raftsim import _abi, dist

pytestmark = pytest.mark.gpu

def check_identities(c):
    assert sum(c["leaders_hist"]) == sum(c["live_hist"]) == c["clusters"]
    b = c["by_class"]
    assert b["no_leader"] + b["one_leader"] + b["multi_leader"] == c["clusters"]
    assert sum(c["fault_nodes"]) == c["nodes"]
    assert sum(c["role_nodes"]) == c["nodes"] - sum(c["fault_nodes"][1:])
    assert len(c["leaders_hist"]) == len(c["live_hist"]) == c["nodes"] // c["clusters"] + 1


@pytest.mark.parametrize("name,n,ticks", PARITY, ids=[f"{p[0]}-{p[1]}" for p in PARITY])
def test_census_and_selection_equal_the_oracles(name, n, ticks):
    """Every N = 2..9: census() field by field and select() over every cluster."""
    cfg = cfg_of(name, n)
    assert n % (64 // cfg["nodes"]) or name == "burst_variant_mid_n8"
    want = co.oracle_at(cfg, ticks)
    g = helpers.gpu(**cfg)
    for t, (cen, recs) in zip(ticks, want):
        g.step(t - g.tick)
        got = g.census()
        for k in cen:
            assert got[k] == cen[k], (name, t, k)
        assert list(got) == list(cen)
        check_identities(got)
        total, sel = g.select()
        assert total == n and sel == recs, (name, t)
        # the census agrees with the selection it summarises
        for k, bit in _abi.CLUSTER_CLASSES.items():
            assert g.select(any=(k,), limit=0) == (cen["by_class"][k], []), (name, t, k)
    g.close()


def test_compaction_dense():
    """4,133 clusters (no multiple of the wave's 12, of the workgroup's 48 or of the chunk's 768;
    six chunks), every class populated: the full list, each class alone, all / none / combined
    predicates, limits below, at and above the total, the count alone, an empty answer."""
    cfg = cfg_of("arena_odd", 4133)
    ticks = (750, 1500)
    want = co.oracle_at(cfg, ticks)
    assert co.population(want[0][0]) == [489, 3617, 27, 1025, 525, 1, 1, 556, 3480]
    assert co.population(want[1][0]) == [1566, 2557, 10, 2957, 2320, 0, 322, 1586, 2497]
    g = helpers.gpu(**cfg)
    for t, (cen, recs) in zip(ticks, want):
        g.step(t - g.tick)
        assert g.census() == cen, t
        assert g.select() == (4133, recs), t
        for k in co.CLASSES:
            exp = co.select_of(recs, any=(k,))
            assert exp[0] == cen["by_class"][k]
            assert g.select(any=(k,)) == exp, (t, k)
        for pred in (dict(all=("one_leader", "halted")), dict(none=("settled",)),
                     dict(any=("no_leader", "candidate"), all=("halted",),
                          none=("no_quorum", "log_full")),
                     dict(any=("multi_leader", "log_full"), none=("candidate",))):
            exp = co.select_of(recs, **pred)
            assert 0 < exp[0] < 4133, (t, pred)
            assert g.select(**pred) == exp, (t, pred)
        total, sub = co.select_of(recs, any=("halted",))
        for limit in (1, 100, total - 1, total, total + 1, 5000):
            assert g.select(any=("halted",), limit=limit) == (total, sub[:limit]), (t, limit)
        assert g.select(any=("halted",), limit=0) == (total, [])
        # nobody matches: a settled cluster has one leader
        assert g.select(all=("settled", "no_leader")) == (0, [])
        assert g.select(all=("settled",), none=("one_leader",), limit=10) == (0, [])
    g.close()


def test_compaction_sparse_and_shards():
    """3,001 clusters; at tick 9000 four of them hold two leaders (in one term each): one shard
    against three on the same device give the same census and the same lists, rebased to the
    handle; a limit that cuts inside the second shard. At tick 4500 nothing is elected yet."""
    cfg = cfg_of("c5_variant", 3001)
    ticks = (4500, 9000)
    want = co.oracle_at(cfg, ticks)
    (cen0, recs0), (cen1, recs1) = want
    assert co.population(cen0) == [3001, 0, 0, 0, 0, 0, 0, 0, 0]
    assert co.population(cen1) == [701, 2296, 4, 0, 0, 4, 0, 160, 1601]
    multi = co.select_of(recs1, any=("multi_leader",))
    lo = [3001 * d // 3 for d in range(4)]
    cand = co.select_of(recs1, any=("candidate",))
    in_first = sum(r["cluster"] < lo[1] for r in cand[1])
    in_second = sum(lo[1] <= r["cluster"] < lo[2] for r in cand[1])
    assert in_first and in_second > 1 and in_first + in_second < cand[0]
    seen = []
    for nd in (1, 3):
        g = helpers.gpu(n_devices=nd, **cfg)
        g.step(4500)
        assert g.census() == cen0, nd
        assert g.select(any=("no_leader",), limit=0) == (3001, []), nd
        assert g.select(none=("no_leader",)) == (0, []), nd
        assert g.select() == (3001, recs0), nd
        g.step(4500)
        assert g.census() == cen1, nd
        assert multi[0] == 4 and g.select(any=("multi_leader",)) == multi, nd
        assert g.select(all=("same_term_leaders",)) == multi, nd
        assert g.select() == (3001, recs1), nd
        cut = in_first + in_second // 2 + 1              # inside the second shard
        assert g.select(any=("candidate",), limit=cut) == (cand[0], cand[1][:cut]), nd
        assert g.select(any=("candidate",), limit=in_first) == (cand[0], cand[1][:in_first]), nd
        seen.append((g.census(), g.select(none=("settled",))))
        g.close()
    assert seen[0] == seen[1]
    # the same job's clusters 1000.. as a handle of their own: cluster rebased, global ids kept
    part = [dict(r, cluster=r["cluster"] - 1000) for r in multi[1] if r["cluster"] >= 1000]
    g = helpers.gpu(**dict(cfg, n_clusters=2001, cluster_offset=1000, n_devices=2))
    g.step(9000)
    assert part and g.select(any=("multi_leader",)) == (len(part), part)
    g.close()


@pytest.mark.parametrize("name,ticks,mode", [("lite_n3", 30000, None), ("lite_n4", 30000, None),
                                             ("lite_elections", 30000, "always")])
def test_steady_path_is_read_as_it_stands(name, ticks, mode, monkeypatch):
    """Handles the steady kernel runs (certified blocks after the first launches): the census is
    the oracle's, the query changes no digest, and a further step still matches the oracle: the
    query wrote nothing and the certificates stand. lite_elections keeps electing, which sends the
    default path choice to the general kernel now and then: there every launch is held on the
    steady kernel, as test_gpu_parity's forced runs do."""
    if mode:
        monkeypatch.setenv("RAFTSIM_STEADY", mode)
    cfg = dict(CASES[name])
    assert 1000 <= cfg["n_clusters"] <= 1200
    r = pairing.oracle(cfg)
    g = helpers.gpu(**cfg)
    for _ in range(ticks // 10000):
        g.step(10000)
    r.step(ticks)
    assert g.diag_last_bails() >= 0                    # the last launch took the steady path
    before = g.digest()
    cen, recs = co.of_backend(r)
    assert g.census() == cen
    assert g.select() == (cfg["n_clusters"], recs)
    assert g.select(any=("settled",), limit=0)[0] == cen["by_class"]["settled"] > 0
    assert np.array_equal(g.digest(), before) and np.array_equal(before, r.digest())
    g.step(10000)
    r.step(10000)
    assert g.diag_last_bails() >= 0
    pairing.same(g, r, "the step after the queries")
    assert g.census() == co.of_backend(r)[0]
    pairing.same_counters(g, r)
    g.close()


def test_queries_are_stream_ordered():
    """step_async several times with no sync: the queries wait for the steps."""
    cfg = cfg_of("fast_timers", 333)
    cen, recs = co.oracle_at(cfg, (1000, 2000))[1]
    assert co.population(cen) == [306, 26, 1, 238, 113, 1, 0, 319, 10]
    for extra in (dict(), dict(ticks_per_launch=37, schedule=1)):
        g = helpers.gpu(**cfg, **extra)
        for _ in range(4):
            g.step_async(500)
        assert g.census() == cen, extra
        assert g.select() == (333, recs), extra
        g.sync()
        assert g.census() == cen and g.last_census_ms() > 0
        g.close()
    g = helpers.gpu(**cfg)
    for _ in range(4):
        g.step_async(500)
    assert g.select(any=("halted",)) == co.select_of(recs, any=("halted",))
    g.close()


# -- host-written states ---------------------------------------------------------------------------

LOG_CAP = 8


def patterns(N, quorum):
    """name -> ({node index: fields}, the classes the cluster is in), on a base of live followers
    at term 1 that name no leader. One cluster per class bit, and the edges: a halted leader is no
    leader, a halted candidate no candidate, a full log counts on a halted node."""
    halt_to_lose = N - quorum + 1
    last = N - 1
    return {
        "no_leader": ({}, ("no_leader",)),
        "one_leader": ({0: dict(role=2, current_term=3, leader_id=1),
                        **{k: dict(current_term=2, leader_id=1) for k in range(1, N)}},
                       ("one_leader",)),
        "multi_leader": ({0: dict(role=2, current_term=3), 1: dict(role=2, current_term=4)},
                         ("multi_leader",)),
        "halted_leader": ({last: dict(role=2, current_term=5, fault=1)},
                          ("no_leader", "halted") + (("no_quorum",) if N - 1 < quorum else ())),
        "no_quorum": ({k: dict(fault=1 + k % 4) for k in range(halt_to_lose)},
                      ("no_leader", "halted", "no_quorum")),
        "same_term_leaders": ({0: dict(role=2, current_term=6), last: dict(role=2, current_term=6)},
                              ("multi_leader", "same_term_leaders")),
        "log_full_on_halted": ({last: dict(fault=4, log_len=LOG_CAP, arena_frontier=LOG_CAP)},
                               ("no_leader", "halted")
                               + (("no_quorum",) if N - 1 < quorum else ()) + ("log_full",)),
        "candidate": ({last: dict(role=1, current_term=2)}, ("no_leader", "candidate")),
        "halted_candidate": ({0: dict(role=1, current_term=2, fault=2)},
                             ("no_leader", "halted") + (("no_quorum",) if N - 1 < quorum else ())),
        "settled": ({k: dict(role=2 if k == 1 else 0, current_term=9, leader_id=2)
                     for k in range(N)}, ("one_leader", "settled")),
    }


def write_pattern(g, cluster, mods):
    N = g.N
    raw = list(g.read_nodes_raw(cluster, 1))
    every = ((1 << (N + 1)) - 1) & ~1
    for k, node in enumerate(raw):
        node.role, node.current_term, node.leader_id, node.fault = 0, 1, 0, 0
        node.log_len = node.arena_base = node.arena_frontier = 0
        node.ls_present = node.ls_keys = 0
        for f, v in mods.get(k, {}).items():
            setattr(node, f, v)
        if node.role == 2:                       # a leader record carries its leader-state
            node.ls_present, node.ls_keys = 1, every & ~(1 << (k + 1))
    g.write_nodes(cluster, raw)


@pytest.mark.parametrize("nodes,variant", [(2, 0), (9, 0), (2, 2), (8, 2)])
def test_host_written_states(nodes, variant):
    """One cluster per class bit written through write_nodes at the first and the last cluster of
    handles of 1, floor(64/N) and floor(64/N) + 1 clusters (a lone cluster, a full wave, a wave
    and one): against the helper on the handle's own read_nodes, and against the classes written
    down here. variant 2 (Spec-Raft) at even N: the stricter quorum N/2 + 1."""
    quorum = co.quorum(nodes, variant)
    assert quorum == (nodes // 2 + 1 if variant else (nodes + 1) // 2)
    cpw = 64 // nodes
    for nc in (1, cpw, cpw + 1):
        g = helpers.gpu(n_clusters=nc, nodes=nodes, log_cap=LOG_CAP, variant_flags=variant, seed=5)
        for pname, (mods, want) in patterns(nodes, quorum).items():
            want = tuple(k for k in co.CLASSES if k in want)
            for c in {0, nc - 1}:
                write_pattern(g, c, mods)
            cen, recs = co.of_backend(g)
            assert g.census() == cen, (nc, pname)
            total, sel = g.select()
            assert (total, sel) == (nc, recs), (nc, pname)
            for c in {0, nc - 1}:
                assert sel[c]["classes"] == want, (nc, pname, c)
            mask_rest = tuple(k for k in co.CLASSES if k not in want)
            exact = g.select(all=want, none=mask_rest)
            assert {0, nc - 1} <= {r["cluster"] for r in exact[1]} and exact[0] == len(exact[1])
            if pname == "halted_leader":
                assert sel[0]["leaders"] == [] and sel[0]["halted"] == [nodes]
                assert cen["role_nodes"][2] == 0 and cen["fault_nodes"][1] == len({0, nc - 1})
            if pname == "same_term_leaders":
                assert sel[nc - 1]["leaders"] == [1, nodes] and sel[nc - 1]["term_max"] == 6
                assert sel[nc - 1]["term_min"] == (1 if nodes > 2 else 6)
            if pname == "log_full_on_halted":
                assert sel[0]["len_max"] == LOG_CAP and cen["len_max"] == LOG_CAP
            if pname == "no_quorum":
                assert sel[0]["halted"] == list(range(1, nodes - quorum + 2))
        check_identities(g.census())
        g.close()
    if variant:     # the same written state under the faithful quorum: one halt of two is survived
        with helpers.gpu(n_clusters=1, nodes=nodes, log_cap=LOG_CAP, seed=5) as f:
            mods = {k: dict(fault=1) for k in range(nodes - quorum + 1)}
            write_pattern(f, 0, mods)
            assert "no_quorum" not in f.select()[1][0]["classes"]
            assert f.census()["by_class"]["no_quorum"] == 0


def test_large_handle_takes_the_strided_and_tiled_paths():
    """115,138 nine-node clusters, the smallest size past both thresholds the runs above stay
    below: the census grid is capped (1,024 workgroups stride over 16,449 wave groups, four or five
    each) and the selection has 258 chunks of 448 clusters, more than the scan's one tile of 256.
    A handle fresh from init-node with settled clusters written at the chunk and tile edges; the
    expectation is the helper's census of one untouched and one written cluster, scaled."""
    N, chunk = 9, 4 * 16 * (64 // 9)
    C = 256 * chunk + 450
    assert chunk == 448 and C == 115138 and -(-C // chunk) == 258 and -(-C // 7) > 4 * 1024
    where = [0, chunk - 1, chunk, 100 * chunk + 7, 256 * chunk - 1, 256 * chunk, C - 1]
    g = helpers.gpu(n_clusters=C, nodes=N, log_cap=LOG_CAP, inbox_cap=1, seed=5)
    mods = patterns(N, co.quorum(N, 0))["settled"][0]
    for c in where:
        write_pattern(g, c, mods)

    def one(c):
        nodes, cl = g.read_nodes(c, 1), g.read_clusters(c, 1)
        return (co.census_of(nodes, cl, N, LOG_CAP, 0),
                dict(co.records_of(nodes, N, LOG_CAP, 0)[0], cluster=c, global_id=c))
    (init, irec), (wrote, wrec) = one(1), one(where[3])
    assert irec["classes"] == ("no_leader",) and wrec["classes"] == ("one_leader", "settled")
    a, b = C - len(where), len(where)
    want = {}
    for k, v in init.items():
        w = wrote[k]
        if k == "by_class":
            want[k] = {x: a * v[x] + b * w[x] for x in v}
        elif isinstance(v, list):
            want[k] = [a * x + b * y for x, y in zip(v, w)]
        elif k.endswith("_max"):
            want[k] = max(v, w)
        elif k == "term_min":
            want[k] = min(v, w)
        else:
            want[k] = a * v + b * w
    assert want["clusters"] == C and want["by_class"]["settled"] == b
    assert want["term_sum"] == 9 * a + 81 * b          # init-node's term is 1, the written one 9
    assert g.census() == want
    recs = [dict(wrec, cluster=c, global_id=c) for c in where]
    assert g.select(any=("one_leader",)) == (b, recs)
    assert g.select(all=("settled",), limit=5) == (b, recs[:5])
    rest = [c for c in range(C) if c not in where]
    assert g.select(none=("settled",), limit=0) == (a, [])
    total, head = g.select(any=("no_leader",), limit=chunk + 3)
    assert total == a and head == [dict(irec, cluster=c, global_id=c) for c in rest[:chunk + 3]]
    g.close()


# -- identities, arguments, reduction --------------------------------------------------------------

def test_reduce_census_of_one_rank_is_the_identity():
    import torch.distributed as tdist

    cfg = cfg_of("fast_timers", 333)
    g = helpers.gpu(**cfg)
    g.step(2000)
    c = g.census()
    check_identities(c)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    tdist.init_process_group("gloo", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{port}")
    try:
        red = dist.reduce_census(c)
    finally:
        tdist.destroy_process_group()
    assert red == c and list(red) == list(c)
    assert c == co.oracle_at(cfg, (1000, 2000))[1][0]
    g.close()


def test_bad_arguments():
    g = helpers.gpu(**cfg_of("fast_timers", 4))
    sel = g._census["select"]
    buf = (_abi.ClusterState * 4)()
    for any_, all_, none_, out, cap in ((512, 0, 0, buf, 4), (0, 1024, 0, buf, 4),
                                        (0, 0, 2 ** 31, buf, 4), (0, 3, 2, buf, 4),
                                        (1, 0, 0, None, 4)):
        assert sel(g._h, any_, all_, none_, out, cap) == -22, (any_, all_, none_, cap)
        assert g._fns["last_error"]()
    assert g._census["read"](g._h, None) == -22
    assert sel(g._h, 0, 0, 0, None, 0) == 4            # count only, no output
    assert sel(g._h, 511, 0, 0, buf, 4) == 4
    assert [b.cluster for b in buf] == [0, 1, 2, 3] and all(b.classes == 1 for b in buf)
    with pytest.raises(ValueError):
        g.select(any=("leaderless",))
    with pytest.raises(helpers.RaftSimError):
        g.select(all=("halted",), none=("halted",))
    assert g.select(limit=2) == (4, g.select()[1][:2])
    g.close()
