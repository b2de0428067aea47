"""The log audit on the GPU: Simulator.audit and Simulator.audit_select (csrc/audit_kernel.hip) held
to tests/audit_oracle.py -- run on the oracle's records and logs for the parity cases, and on the
GPU handle's own read-back for host-written logs (long ones, ones that cross an arena's end: no run
reaches them). tests/test_audit_abi.py checks the mirror against hand-written logs and pins the
populations of the runs below; every class occurs in them."""
import socket

import numpy as np
import pytest

import audit_oracle as ao
import audit_shapes
import helpers
from cases import CASES, PARITY, cfg_of
from raftsim import _abi, dist

pytestmark = pytest.mark.gpu


def check_identities(s):
    b = s["by_class"]
    assert b["commit_diverged"] <= b["diverged"] and b["match_broken"] <= b["diverged"]
    assert b["diverged"] + b["identical"] <= s["clusters"]
    assert s["diverged_nodes"] >= 2 * b["diverged"]
    assert (s["diverge_index_min"] is None) == (b["diverged"] == 0)
    assert (s["commit_diverge_index_min"] is None) == (b["commit_diverged"] == 0)
    assert s["agree_min"] <= s["agree_max"] and s["agree_sum"] <= s["entries"]


def check_against(g, summary, recs, where):
    """audit(), the full record list and every class's count against the mirror's."""
    got = g.audit()
    for k in summary:
        assert got[k] == summary[k], (where, k)
    assert list(got) == list(summary)
    check_identities(got)
    total, sel = g.audit_select()
    assert total == len(recs), where
    for a, b in zip(sel, recs):
        assert a == b, (where, b["cluster"])
    for k in _abi.AUDIT_CLASSES:
        assert g.audit_select(any=(k,), limit=0) == (summary["by_class"][k], []), (where, k)


@pytest.mark.parametrize("name,n,ticks", PARITY, ids=[f"{p[0]}-{p[1]}" for p in PARITY])
def test_audit_and_selection_equal_the_mirror_on_the_oracle(name, n, ticks):
    """Every N = 2..9 (333 and 96 clusters: no multiple of a wave's 4 clusters at 333, whole waves
    at 96): audit() field by field, audit_select() over every cluster, the class counts."""
    cfg = cfg_of(name, n)
    want = ao.oracle_at(cfg, ticks)
    g = helpers.gpu(**cfg)
    for t, (summary, recs) in zip(ticks, want):
        g.step(t - g.tick)
        check_against(g, summary, recs, (name, t))
    assert want[0][0] != want[1][0], "the two checkpoints differ"
    g.close()


# -- host-written logs -----------------------------------------------------------------------------

def write_shapes(g, shapes, A, where=None):
    """One cluster per shape (shape i at cluster where[i], or i): the arenas (poison outside the
    logs), then the node records."""
    N = g.N
    for c, sh in zip(where or range(len(shapes)), shapes):
        bases = audit_shapes.bases(N, A, c, sh)
        raw = list(g.read_nodes_raw(c, 1))
        for k, node in enumerate(raw):
            log = sh["logs"][k]
            g.write_arena(c, k + 1, audit_shapes.arena_of(log, bases[k], A, k))
            node.log_len, node.commit_index = len(log), sh["commits"][k]
            node.arena_base, node.arena_frontier = bases[k], bases[k] + len(log)
        g.write_nodes(c, raw)


def host_written(nodes, odd):
    log_cap, A = (24, 51) if odd else (256, 1024)
    shapes = audit_shapes.shapes(nodes, log_cap)
    g = helpers.gpu(n_clusters=len(shapes), nodes=nodes, log_cap=log_cap, arena_cap=A, seed=3)
    write_shapes(g, shapes, A)
    return g, shapes


@pytest.mark.parametrize("nodes,odd,width", [(2, False, 16), (5, False, 16), (9, False, 16),
                                             (5, True, 16), (2, False, 64), (5, False, 64),
                                             (9, False, 64), (5, True, 64)])
def test_host_written_logs(nodes, odd, width, monkeypatch):
    """tests/audit_shapes.py's clusters (lengths 0 .. log_cap around both group widths' step
    boundaries, single differences in term or val between the first, a middle and the last pair of
    the pair mask, short logs that end around the difference, equal terms after a difference,
    inversions, commits on both sides of a difference), every log at an arena_base of its own so
    that it crosses the arena's end at another position, poison in every slot outside the logs:
    against the mirror on the handle's own read-back and against the classes written down with the
    shapes, with either group width."""
    monkeypatch.setenv("RAFTSIM_AUDIT_WIDTH", str(width))
    g, shapes = host_written(nodes, odd)
    assert len(shapes) % 4
    summary, recs = ao.of_backend(g)
    for rec, sh in zip(recs, shapes):
        assert rec["classes"] == tuple(k for k in ao.CLASSES if k in sh["want"]), sh["name"]
    # nothing passes on an empty set
    assert all(summary["by_class"].values())
    for f in ("diverge_index", "commit_diverge_index", "order_index"):
        assert any(r[f] is None for r in recs) and any(r[f] is not None for r in recs), f
    check_against(g, summary, recs, (nodes, odd, width))
    assert g.audit_select(all=("term_order", "identical")) == \
        ao.select_of(recs, all=("term_order", "identical"))
    assert g.last_audit_ms() > 0
    g.close()


def test_records_stay_valid_until_a_log_or_commit_changes():
    """audit() leaves the records on the device; a write of an arena, of a node record and a step
    each make the next query walk the logs again."""
    g, shapes = host_written(5, False)
    summary, recs = ao.of_backend(g)
    assert g.audit() == summary
    assert g.audit_select() == (len(recs), recs)             # from the records audit() left
    # one entry of an identical cluster rewritten
    c = next(i for i, s in enumerate(shapes) if s["name"] == "identical_65")
    assert recs[c]["classes"] == ("identical",)
    node = g.read_nodes(c, 1)[2]
    arena = g.read_arena(c, 3)
    slot = (node["arena_base"] + 40) % len(arena)
    arena[slot] = (arena[slot][0], arena[slot][1] + 1)
    g.write_arena(c, 3, arena)
    total, sel = g.audit_select(any=("diverged",))
    hit = [r for r in sel if r["cluster"] == c]
    assert hit and hit[0]["classes"] == ("diverged", "commit_diverged", "match_broken")
    assert hit[0]["diverge_index"] == 40 and hit[0]["diverged"] == [1, 2, 3, 4, 5]
    assert total == summary["by_class"]["diverged"] + 1
    assert g.audit() == ao.of_backend(g)[0]
    # a commit index lowered: bit 2 goes, bit 1 stays
    raw = list(g.read_nodes_raw(c, 1))
    for node in raw:
        node.commit_index = 40
    g.write_nodes(c, raw)
    after = g.audit_select(any=("diverged",))[1]
    hit = [r for r in after if r["cluster"] == c]
    assert hit[0]["classes"] == ("diverged", "match_broken")
    assert hit[0]["commit_diverge_index"] is None and hit[0]["diverge_index"] == 40
    assert g.audit_select() == (len(recs), ao.of_backend(g)[1])
    g.close()
    # a step: the summary becomes the next checkpoint's
    cfg = cfg_of("fast_timers", 333)
    (s0, r0), (s1, r1) = ao.oracle_at(cfg, (1000, 2000))
    assert ao.population(s0) == [75, 26, 33, 0, 190] and ao.population(s1) == [104, 38, 47, 0, 132]
    g = helpers.gpu(**cfg)
    g.step(1000)
    assert g.audit() == s0 and g.audit_select() == (333, r0)
    g.step(1000)
    assert g.audit_select() == (333, r1) and g.audit() == s1
    g.close()


# -- the capped grid -------------------------------------------------------------------------------

def capped_handle(width, C):
    """A handle past the pass's grid cap at `width` lanes per cluster (2,048 workgroups of four
    waves: 8,192 groups of 64 / width clusters a trip), N = 3, fresh from init-node, with four
    written clusters: at cluster 0, at the last cluster of the first trip, at the first of the
    second and at C - 1. Returns (handle, their clusters, the expected audit(), the expected
    records of the written clusters): the mirror on the read-back of the written clusters and of
    one untouched cluster, that one scaled by the number of untouched clusters."""
    N, log_cap, A = 3, 24, 51
    trip = 2048 * 4 * (64 // width)
    assert trip < C < 2 * trip
    where = [0, trip - 1, trip, C - 1]
    by_name = {s["name"]: s for s in audit_shapes.shapes(N, log_cap)}
    shapes = [by_name[k] for k in ("diff_term_0", "order_one_15", "match_step16", "identical_17")]
    assert "commit_diverged" in shapes[0]["want"] and "term_order" in shapes[1]["want"]
    assert shapes[2]["want"] == ("diverged", "match_broken") and shapes[3]["want"] == ("identical",)
    g = helpers.gpu(n_clusters=C, nodes=N, log_cap=log_cap, arena_cap=A, seed=3)
    write_shapes(g, shapes, A, where)

    def one(c):
        nodes = g.read_nodes(c, 1)
        logs = [g.log(c, k + 1) if r["log_len"] else [] for k, r in enumerate(nodes)]
        rec = ao.records_of(logs, [r["commit_index"] for r in nodes], N)[0]
        rec = dict(rec, cluster=c, global_id=c)
        return ao.summary_of([rec], logs), rec
    (init, irec), wrote = one(1), [one(c) for c in where]
    assert irec["classes"] == ("identical",) and init["entries"] == 0
    for (_, rec), sh in zip(wrote, shapes):
        assert rec["classes"] == tuple(k for k in ao.CLASSES if k in sh["want"]), sh["name"]
    a, parts = C - len(where), [s for s, _ in wrote]
    want = {}
    for k, v in init.items():
        ws = [s[k] for s in parts]
        if k == "by_class":
            want[k] = {x: a * v[x] + sum(w[x] for w in ws) for x in v}
        elif k.endswith("_min") or k.endswith("_max"):
            have = [x for x in [v] + ws if x is not None]
            want[k] = (min if k.endswith("_min") else max)(have) if have else None
        else:
            want[k] = a * v + sum(ws)
    assert want["clusters"] == C and want["by_class"]["identical"] == a + 1
    assert want["agree_min"] == 0 and want["agree_max"] == 17 and want["diverge_index_min"] == 0
    return g, where, want, [rec for _, rec in wrote]


@pytest.mark.parametrize("width,C", [(64, 8197), (16, 32789)])
def test_capped_grid_strides_to_a_second_trip(width, C, monkeypatch):
    """The smallest shapes at which the pass's grid is capped. Width 64: 8,197 groups over 8,192
    waves, so groups 8,192 .. 8,196 are a second trip, spread over two workgroups. Width 16: 8,198
    groups of four clusters, the last holding one cluster. Either way the fold kernel sees 2,048
    partial summaries. Written clusters stand on both sides of the trip's edge and at both ends."""
    monkeypatch.setenv("RAFTSIM_AUDIT_WIDTH", str(width))
    g, where, want, recs = capped_handle(width, C)
    got = g.audit()
    assert got == want and list(got) == list(want)
    check_identities(got)
    assert g.audit_select(none=("identical",)) == (3, recs[:3])
    assert [r["cluster"] for r in recs[:3]] == where[:3]
    assert g.audit_select(limit=0) == (C, [])
    assert g.audit_select(any=("identical",), limit=0) == (C - 3, [])
    g.close()


def test_one_handle_serves_both_widths(monkeypatch):
    """The scratch a handle allocates at its first query serves either width: on the 8,197-cluster
    handle a query at width 16, then (a node record written back unchanged makes the next query
    walk the logs again) at 64, at 64 again and at 16 give the same answers. The wide grid there
    is 2,048 workgroups, the narrow one 513."""
    monkeypatch.setenv("RAFTSIM_AUDIT_WIDTH", "16")
    g, _, want, recs = capped_handle(64, 8197)
    answers = []
    for width in (16, 64, 64, 16):
        monkeypatch.setenv("RAFTSIM_AUDIT_WIDTH", str(width))
        g.write_nodes(0, list(g.read_nodes_raw(0, 1)))
        answers.append((g.audit(), g.audit_select(none=("identical",))))
    assert answers == [(want, (3, recs[:3]))] * 4
    g.close()


# -- compaction and shards -------------------------------------------------------------------------

def test_compaction_dense():
    """4,133 clusters (five chunks of 1,024, no multiple of anything), every class populated: each
    class alone, combined predicates, limits below, at and above the total, the count alone, an
    empty answer."""
    cfg = cfg_of("arena_odd", 4133)
    (summary, recs), = ao.oracle_at(cfg, (1500,))
    assert ao.population(summary) == [3841, 2607, 2776, 26, 47]
    g = helpers.gpu(**cfg)
    g.step(1500)
    assert g.audit() == summary
    assert g.audit_select() == (4133, recs)
    for k in ao.CLASSES:
        exp = ao.select_of(recs, any=(k,))
        assert exp[0] == summary["by_class"][k] > 0
        assert g.audit_select(any=(k,)) == exp, k
    for pred in (dict(all=("diverged",), none=("commit_diverged",)),
                 dict(any=("term_order", "identical"), none=("match_broken",)),
                 dict(all=("commit_diverged", "match_broken"), none=("term_order",))):
        exp = ao.select_of(recs, **pred)
        assert 0 < exp[0] < 4133, pred
        assert g.audit_select(**pred) == exp, pred
    total, sub = ao.select_of(recs, any=("commit_diverged",))
    for limit in (1, total - 1, total, total + 1):
        assert g.audit_select(any=("commit_diverged",), limit=limit) == (total, sub[:limit]), limit
    assert g.audit_select(any=("commit_diverged",), limit=0) == (total, [])
    # nobody matches: identical logs do not diverge
    assert g.audit_select(all=("identical", "diverged")) == (0, [])
    assert g.audit_select(all=("identical", "diverged"), limit=10) == (0, [])
    g.close()


def test_shards():
    """3,001 clusters, most of them still identical at tick 9000 and six diverged: one shard
    against three on the same device give the same summary and the same lists, rebased to the
    handle; a limit that cuts inside the second shard; the shards as handles of their own."""
    cfg = cfg_of("c5_variant", 3001)
    (summary, recs), = ao.oracle_at(cfg, (9000,))
    assert ao.population(summary) == [6, 0, 6, 0, 2136]
    lo = [3001 * d // 3 for d in range(4)]
    rest = ao.select_of(recs, none=("identical",))
    in_first = sum(r["cluster"] < lo[1] for r in rest[1])
    in_second = sum(lo[1] <= r["cluster"] < lo[2] for r in rest[1])
    assert in_first and in_second > 1 and in_first + in_second < rest[0] == 865
    seen = []
    for nd in (1, 3):
        g = helpers.gpu(n_devices=nd, **cfg)
        g.step(9000)
        assert g.audit() == summary, nd
        assert g.audit_select() == (3001, recs), nd
        assert g.audit_select(any=("diverged",)) == ao.select_of(recs, any=("diverged",)), nd
        cut = in_first + in_second // 2 + 1              # inside the second shard
        assert g.audit_select(none=("identical",), limit=cut) == (rest[0], rest[1][:cut]), nd
        assert g.audit_select(none=("identical",), limit=in_first) == \
            (rest[0], rest[1][:in_first]), nd
        seen.append((g.audit(), g.audit_select(any=("match_broken",))))
        g.close()
    assert seen[0] == seen[1]
    # the same job's clusters 1000.. as a handle of their own: cluster rebased, global ids kept
    part = [dict(r, cluster=r["cluster"] - 1000) for r in rest[1] if r["cluster"] >= 1000]
    g = helpers.gpu(**dict(cfg, n_clusters=2001, cluster_offset=1000, n_devices=2))
    g.step(9000)
    assert part and g.audit_select(none=("identical",)) == (len(part), part)
    g.close()


def test_reduce_audit_of_one_rank_is_the_identity():
    import torch.distributed as tdist

    cfg = cfg_of("fast_timers", 333)
    g = helpers.gpu(**cfg)
    g.step(2000)
    a = g.audit()
    check_identities(a)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    tdist.init_process_group("gloo", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{port}")
    try:
        red = dist.reduce_audit(a)
    finally:
        tdist.destroy_process_group()
    assert red == a and list(red) == list(a)
    assert a == ao.oracle_at(cfg, (1000, 2000))[1][0]
    g.close()


# -- read-only, stream order, arguments ------------------------------------------------------------

def test_queries_read_only_and_stream_ordered():
    cfg = cfg_of("fast_timers", 333)
    summary, recs = ao.oracle_at(cfg, (1000, 2000))[1]
    g = helpers.gpu(**cfg)
    g.step(2000)
    before = g.digest(), g.counters(), g.violations(limit=0)
    assert g.audit() == summary and g.audit_select() == (333, recs)
    after = g.digest(), g.counters(), g.violations(limit=0)
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    assert g.audit() == g.audit()                          # bitwise the same answer
    g.close()
    # step_async several times with no sync: the queries wait for the steps
    for extra in (dict(), dict(ticks_per_launch=37, schedule=1)):
        g = helpers.gpu(**cfg, **extra)
        for _ in range(4):
            g.step_async(500)
        assert g.audit() == summary, extra
        assert g.audit_select() == (333, recs), extra
        g.sync()
        assert g.audit() == summary
        g.close()
    g = helpers.gpu(**cfg)
    for _ in range(4):
        g.step_async(500)
    assert g.audit_select(any=("diverged",)) == ao.select_of(recs, any=("diverged",))
    g.close()


def test_steady_certificates_stay_and_empty_logs_load_nothing():
    """The config-2 shape: five warm-up launches, audit(), one more launch; the steady kernel bails
    what a twin handle without the audit bails, so the certificates stood. Every log is empty: all
    identical, no entries."""
    cfg = dict(CASES["c2_small"])
    g, twin = helpers.gpu(**cfg), helpers.gpu(**cfg)
    for h in (g, twin):
        for _ in range(5):
            h.step(10000)
    a = g.audit()
    n = cfg["n_clusters"]
    assert a == dict(clusters=n, by_class=dict(diverged=0, commit_diverged=0, match_broken=0,
                                               term_order=0, identical=n),
                     entries=0, agree_sum=0, agree_min=0, agree_max=0, diverged_nodes=0,
                     commit_diverged_nodes=0, diverge_index_min=None,
                     commit_diverge_index_min=None)
    assert g.audit_select(none=("identical",)) == (0, [])
    for h in (g, twin):
        h.step(10000)
    assert g.diag_last_bails() == twin.diag_last_bails() >= 0
    assert np.array_equal(g.digest(), twin.digest()) and g.counters() == twin.counters()
    g.close()
    twin.close()


def test_bad_arguments():
    g = helpers.gpu(**cfg_of("fast_timers", 4))
    sel = g._audit["select"]
    buf = (_abi.AuditRecord * 4)()
    for any_, all_, none_, out, cap in ((32, 0, 0, buf, 4), (0, 64, 0, buf, 4),
                                        (0, 0, 2 ** 31, buf, 4), (0, 3, 2, buf, 4),
                                        (1, 0, 0, None, 4)):
        assert sel(g._h, any_, all_, none_, out, cap) == -22, (any_, all_, none_, cap)
        assert g._fns["last_error"]()
    assert g._audit["read"](g._h, None) == -22
    assert sel(g._h, 0, 0, 0, None, 0) == 4            # count only, no output
    assert sel(g._h, 31, 0, 0, buf, 4) == 4
    assert [b.cluster for b in buf] == [0, 1, 2, 3] and all(b.classes == 16 for b in buf)
    assert all(b.diverge_index == 2 ** 32 - 1 and b.len_min == 0 for b in buf)
    with pytest.raises(ValueError):
        g.audit_select(any=("forked",))
    with pytest.raises(helpers.RaftSimError):
        g.audit_select(all=("diverged",), none=("diverged",))
    assert g.audit_select(limit=2) == (4, g.audit_select()[1][:2])
    g.close()
