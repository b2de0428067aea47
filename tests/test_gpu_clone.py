"""Cluster state cloned on the GPU (include/raftsim.h, raft_clone_write): cluster s of one handle
becomes cluster t of the same or of another handle without a pack in host memory, and the target is
bit for bit what scatter(gather(...)) leaves.

The expected state comes from code that is not under test, in two ways: (a) the host path
scatter(gather(...)) on a twin handle, and (b) the C oracle, in which the same clone is
pack = gather_mirror.pack_of(ref, sources) followed by ref.restore_cluster(pack, i,
cluster=targets[i]). The in-handle cases are tests/test_gather_abi.py's GPU_CASES (odd arena_cap,
N = 2 and N = 9, a record large enough for more than one workgroup, wrapped commit-stream rings).
Every handle compared by digest has trace_cap 0."""
import ctypes

import numpy as np
import pytest

import gather_mirror as gm
import helpers
import pairing
import raftsim
from cases import CASES, GPU_CASES, ROUNDTRIP
from raftsim import _abi

pytestmark = pytest.mark.gpu

SUMS = ["node_ticks"] + _abi.COUNTER_NAMES
STEADY = dict(n_clusters=1024, nodes=5, hb=300, el_base=500, el_span=500)


def oracle_clone(ref, sources, targets):
    """The clone in an oracle handle: the mirror's pack of the distinct sources, restored into the
    targets through the write_* calls."""
    distinct = sorted(set(sources))
    pack = gm.pack_of(ref, distinct)
    at = {c: i for i, c in enumerate(distinct)}
    for s, t in zip(sources, targets):
        ref.restore_cluster(pack, at[s], cluster=t)


def raw_clone(dst, targets, src, sources, n=None):
    """raft_clone_write as the C ABI has it: (return code, message)."""
    t = (ctypes.c_uint32 * max(1, len(targets)))(*targets)
    s = (ctypes.c_uint32 * max(1, len(sources)))(*sources)
    rc = dst._clone["write"](dst._h, t, src._h, s, len(targets) if n is None else n)
    return rc, dst._fns["last_error"]().decode()


def deltas(after, before):
    return {k: after[k] - before[k] for k in SUMS}


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_in_handle(name):
    cfg, ticks = GPU_CASES[name]
    C = cfg["n_clusters"]
    third = C // 3
    # the first third onto the last third reversed and onto the middle third in order: with an odd
    # arena_cap the arenas go even -> odd, odd -> even and between equal parities
    sources = list(range(third)) * 2
    targets = list(range(C - 1, C - 1 - third, -1)) + list(range(third, 2 * third))
    rest = np.setdiff1d(np.arange(C), targets)
    g, ref = helpers.gpu(**cfg), pairing.oracle(cfg, threads=8)
    g.step(ticks)
    ref.step(ticks)
    if name == "c4_n9":                                  # more than one workgroup per pair
        stride = g.gather_layout(_abi.SCATTER_PARTS)["stride"]
        assert stride // 32768 >= 2, stride
    if cfg.get("arena_cap", 0) % 2:                      # (source, target) parities of the arenas
        N, A = cfg["nodes"], cfg["arena_cap"]
        met = {(s * N * A % 2, t * N * A % 2) for s, t in zip(sources, targets)}
        assert met >= {(0, 1), (1, 0)}
        if third % 2 == 0:                               # arena_odd: equal parities too
            assert met == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if name == "arena_odd":
        assert third % 2 == 0
    before = g.digest()
    assert np.array_equal(before, ref.digest())
    assert g.clone(sources, targets) == len(targets)
    assert g.host_written and g.last_clone_ms() > 0
    now = g.digest()
    assert np.array_equal(now[targets], before[sources])
    assert np.array_equal(now[rest], before[rest]), "untouched clusters"
    got = g.gather(targets)
    assert np.array_equal(got.data, g.gather(sources).data), "a gather of the targets, every part"
    assert np.array_equal(gm.pack_bytes(g, targets), got.data), "the targets' per-node reads"
    oracle_clone(ref, sources, targets)
    assert np.array_equal(now, ref.digest())
    g0, r0 = g.counters(), ref.counters()
    pairing.step(g, ref, 4000, "after the clone")
    assert deltas(g.counters(), g0) == deltas(ref.counters(), r0)
    for h in (g, ref):
        h.close()


def test_one_source_to_many():
    cfg = dict(CASES["n2"], n_clusters=4200)
    g = helpers.gpu(**cfg)
    g.step(6000)
    c = 5
    targets = [t for t in range(4200) if t != c][:4097]  # more pairs than workgroups in flight
    pack = g.gather([c])
    before = g.digest()
    want = before[c]
    assert g.clone([c] * len(targets), targets) == 4097
    d = g.digest()
    assert (d[targets] == want).all() and d[c] == want
    assert np.array_equal(d[4098:], before[4098:]), "untouched clusters"
    picks = (targets[0], targets[2048], targets[-1])
    refs = []
    for j in picks:                                      # the same state under another global id
        one = helpers.oracle(**dict(cfg, n_clusters=1, cluster_offset=j))
        one.restore_cluster(pack, 0)
        one.step(8000)
        refs.append(one.digest()[0])
        one.close()
    g.step(8000)
    d = g.digest()
    assert [d[j] for j in picks] == refs
    assert len(np.unique(d[targets])) >= 2, "the futures differ"
    g.close()


def test_owed_draws_and_certificates():
    """tests/test_gpu_scatter.py's test_steady_path_is_earned_again handle: after three steady
    launches certificates are set and the followers' draws are owed. A clone that resolved a draw
    with the target's id, passed FL_DRAW through or copied the certificate would differ from the
    host path and from the oracle, at once or a step later."""
    g, twin, ref = helpers.gpu(**STEADY), helpers.gpu(**STEADY), pairing.oracle(STEADY, threads=8)
    for _ in range(3):
        for h in (g, twin):
            h.step(10000)
    ref.step(30000)
    assert g.diag_last_bails() >= 0                      # the steady path ran
    sources, targets = list(range(512)), list(range(1023, 511, -1))
    assert g.clone(sources, targets) == 512
    assert twin.scatter(twin.gather(sources), targets) == 512
    oracle_clone(ref, sources, targets)
    for step in range(3):
        if step:
            for h in (g, twin, ref):
                h.step(10000)
        d = g.digest()
        assert np.array_equal(d, twin.digest()), step
        assert np.array_equal(d, ref.digest()), step
    assert g.diag_last_bails() >= 0
    for h in (g, twin, ref):
        h.close()


def test_cross_handle_a_queued_client_set_ends_lite():
    cfg = dict(n_clusters=64, nodes=5, hb=300, el_base=500, el_span=500)
    src, ref = helpers.gpu(**cfg), pairing.oracle(cfg, threads=8)
    for h in (src, ref):
        h.step(3000)
        for c, node in ((2, 1), (40, 3)):
            helpers.client_set_into(h, c, node, 700 + c)
    tgt = helpers.gpu(**cfg)                             # a LITE handle until the clone
    tgt.set_tick(3000)
    assert tgt.clone(range(64), range(64), source=src) == 64
    assert np.array_equal(tgt.digest(), src.digest())
    pairing.step(tgt, ref, 3000, "the clone's target")
    assert tgt.counters()["ev_cs"] >= 2                  # the two client-sets were handled
    for h in (src, ref, tgt):
        h.close()


def test_shards():
    cfg = dict(CASES["fast_timers"], n_clusters=3001)
    one, three = helpers.gpu(**cfg), helpers.gpu(**cfg, n_devices=3)
    for h in (one, three):
        h.step(2000)
    # shards [0, 1000), [1000, 2000), [2000, 3001): sources on every shard (multiples of 4), each
    # cloned a shard further (targets = 1 mod 4), then pairs inside each shard and the last cluster
    sources = list(range(0, 3000, 4))
    targets = [(s + 1001) % 3000 for s in sources]
    sources += [2, 1002, 2002, 3000]
    targets += [7, 1007, 2007, 999]
    shard = lambda c: min(c // 1000, 2)  # noqa: E731
    assert {(shard(s), shard(t)) for s, t in zip(sources, targets)} >= \
        {(0, 1), (1, 2), (2, 0), (0, 0), (1, 1), (2, 2)}
    assert len(set(targets)) == len(targets) and not set(targets) & set(sources)
    before = one.digest()
    for h in (one, three):
        assert h.clone(sources, targets) == len(targets)
    d = one.digest()
    assert np.array_equal(d[targets], before[sources]) and (d[targets] != before[targets]).all()
    assert np.array_equal(three.digest(), d)
    assert np.array_equal(one.gather(range(3001)).data, three.gather(range(3001)).data)
    # from the 1-shard handle into the 3-shard one, permuted over the shards, and back
    perm = [(c * 7 + 13) % 3001 for c in range(3001)]
    assert three.clone(range(3001), perm, source=one) == 3001
    assert np.array_equal(three.digest()[perm], d)
    one.step(500)
    assert (one.digest() != d).any()
    assert one.clone(perm, range(3001), source=three) == 3001
    assert np.array_equal(one.digest(), d)
    for h in (one, three):
        h.close()


def test_snapshot_rollback_split():
    sim = helpers.gpu(**ROUNDTRIP)
    sim.step(10000)
    snap = raftsim.snapshot(sim)
    assert (snap.tick, snap.C, snap.config.seed) == (10000, sim.C, sim.config.seed)
    at_snap = sim.digest()
    assert np.array_equal(snap.digest(), at_snap)
    c0 = sim.counters()
    sim.step(5000)
    d1, c1 = sim.digest(), sim.counters()
    assert (d1 != at_snap).any()
    raftsim.rollback(sim, snap)
    assert sim.tick == 10000 and np.array_equal(sim.digest(), at_snap)
    assert np.array_equal(snap.digest(), at_snap)
    sim.step(5000)
    assert np.array_equal(sim.digest(), d1)
    assert deltas(sim.counters(), c1) == deltas(c1, c0)
    snap.step(5000)                                      # the snapshot is a continuation too
    assert np.array_equal(snap.digest(), d1)
    snap.close()
    # split: the clusters in an interesting class over eight others
    total, recs = sim.select(any=("multi_leader", "no_leader"), limit=16)
    survivors = recs if total else list(range(8))
    alive = {r["cluster"] if isinstance(r, dict) else r for r in survivors}
    victims = [c for c in range(sim.C - 1, -1, -1) if c not in alive][:8]
    before = sim.digest()
    plan = raftsim.split(sim, survivors, victims)
    assert plan == raftsim.split_plan(survivors, victims) and plan[1] == victims
    assert set(plan[0]) <= alive and len(plan[0]) == 8
    now = sim.digest()
    rest = np.setdiff1d(np.arange(sim.C), victims)
    assert np.array_equal(now[victims], before[plan[0]])
    assert np.array_equal(now[rest], before[rest])
    sim.close()


def test_stream_order():
    cfg = dict(CASES["fast_timers"], n_clusters=600)
    g, twin = helpers.gpu(**cfg), helpers.gpu(**cfg)
    sources, targets = list(range(0, 300)), list(range(599, 299, -1))
    for h in (g, twin):
        h.step(1000)
    g.step_async(3000)
    assert g.clone(sources, targets) == 300              # no sync in between
    twin.step(3000)
    assert twin.clone(sources, targets) == 300
    d = g.digest()
    assert np.array_equal(d, twin.digest())
    assert np.array_equal(d[targets], d[sources])
    for h in (g, twin):
        h.close()


def test_refusals():
    cfg = dict(CASES["fast_timers"], n_clusters=8)
    g, t = helpers.gpu(**cfg), helpers.gpu(**cfg)
    g.step(500)
    t.step(100)
    before = g.digest(), t.digest()
    for dst, src in ((g, g), (t, g)):
        rc, msg = raw_clone(dst, [4, 5], src, [0, 8])
        assert rc == -22 and "sources[1] = 8" in msg
        rc, msg = raw_clone(dst, [4, 5, 8, 9], src, [0, 1, 2, 8])
        assert rc == -22 and "targets[2] = 8" in msg     # the first offending position
        rc, msg = raw_clone(dst, [4, 5, 6, 5, 4], src, [0, 0, 0, 0, 0])
        assert rc == -22 and "targets[3] = 5" in msg and "twice" in msg
        assert raw_clone(dst, [], src, []) == (0, raw_clone(dst, [], src, [])[1])
        assert dst.clone([], [], source=src) == 0
    # inside one handle no cluster is both read and written
    # (the first position either of whose clusters stands on the other side too)
    rc, msg = raw_clone(g, [4, 5, 0], g, [0, 1, 2])
    assert rc == -22 and "sources[0] = 0" in msg and "both a source and a target" in msg
    rc, msg = raw_clone(g, [4, 0, 6], g, [1, 2, 0])
    assert rc == -22 and "targets[1] = 0" in msg and "both a source and a target" in msg
    rc, msg = raw_clone(g, [4, 5, 6], g, [0, 5, 4])
    assert rc == -22 and "targets[0] = 4" in msg
    rc, msg = raw_clone(g, [7, 5, 6], g, [0, 6, 2])
    assert rc == -22 and "sources[1] = 6" in msg
    rc, msg = raw_clone(g, [3], g, [3])
    assert rc == -22 and "both" in msg
    # handles of another shape: the field is named
    with helpers.gpu(**dict(cfg, log_cap=64)) as other:
        rc, msg = raw_clone(other, [0], g, [0])
        assert rc == -22 and "log_cap" in msg
        with pytest.raises(ValueError, match="differ in log_cap"):
            other.clone([0], [0], source=g)
        assert not other.host_written
    # through Python: ranges and lengths
    with pytest.raises(ValueError, match=r"targets\[1\] = 8"):
        g.clone([0, 1], [4, 8])
    with pytest.raises(ValueError, match=r"sources\[0\] = -1"):
        g.clone([-1], [4])
    with pytest.raises(ValueError, match="2 sources for 1 targets"):
        t.clone([1, 2], [0], source=g)
    with pytest.raises(helpers.RaftSimError, match="both a source and a target"):
        g.clone([0, 1], [1, 2])
    assert np.array_equal(g.digest(), before[0]) and np.array_equal(t.digest(), before[1]), \
        "a refused clone wrote nothing"
    # between two handles a cluster id may stand on both sides
    assert t.clone([3, 3], [3, 0], source=g) == 2
    assert (t.digest()[[3, 0]] == before[0][3]).all()
    g.close()
    t.close()


def test_what_a_clone_leaves_alone():
    cfg = dict(CASES["fast_timers"], n_clusters=333)
    g, src, twin = helpers.gpu(**cfg), helpers.gpu(**cfg), helpers.gpu(**cfg)
    g.step(2000)
    for h in (src, twin):
        h.step(3000)
    a0 = g.audit()                                       # the audit's records are valid now
    before = g.violations(), g.counters()
    assert before[0][0] > 0 and a0 != src.audit()
    s_before = (src.violations(), src.counters(), src.audit(), src.audit_select(limit=50),
                src.digest().tolist(), src.tick)
    assert g.clone(range(333), range(333), source=src) == 333
    assert (g.violations(), g.counters()) == before
    assert g.audit() == src.audit(), "the clone dropped the target's audit records"
    assert np.array_equal(g.digest(), src.digest()) and g.tick == 2000
    assert (src.violations(), src.counters(), src.audit(), src.audit_select(limit=50),
            src.digest().tolist(), src.tick) == s_before
    # in-handle: the targets' violation records stay those of the clusters they were
    viol = src.violations()
    assert src.clone(range(100), range(332, 232, -1)) == 100
    assert src.violations() == viol
    twin.clone(range(100), range(332, 232, -1))
    for h in (src, twin):                                # the source's next step is what it was
        h.step(1000)
    assert np.array_equal(src.digest(), twin.digest())
    assert deltas(src.counters(), s_before[1]) == deltas(twin.counters(), s_before[1])
    for h in (g, src, twin):
        h.close()
