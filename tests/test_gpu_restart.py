"""Node restarts on the GPU (include/raftsim.h, raft_restart_write / raft_restart_where; SIM_SPEC
§4a): a halted or a live node's process started again on the device, AMNESIA (the reference's JVM
started again) or DURABLE (Raft's Figure 2).

The expected state comes from code that is not under test: the C oracle handle of the same config
gets raftsim.restart_by_writes (read_nodes, the pure raftsim.restart_record, write_nodes, two empty
write_queue, write_clusters) for the same nodes. Compared at once are every cluster's digest, a
gather of every part of the restarted clusters against the mirror of the oracle's per-node reads
(tests/gather_mirror.py) and against the GPU handle's own per-node reads; both handles then step
15,000 ticks (past T + el_base + el_span) and are compared again by digests and counter deltas.
Every handle compared by digest has trace_cap 0, except where the trace rings are the subject.

The storm (`crash_storm_clients`, 2048 clusters, the case table's seed) was looked at on the oracle
before the assertions were written: at tick 20,000 it has IOOBE, NPE and OVERFLOW halts in 1,835
clusters and 19 clusters with four nodes halted, and up to tick 80,000 no cluster with all five
halted (the last live node of a faithful cluster never wins an election and nothing halts it). The
storm test therefore halts the fifth node of one four-halted cluster by the same write_nodes on
both handles, so that a mask naming every node of a cluster is restarted too."""
import ctypes

import numpy as np
import pytest

import gather_mirror as gm
import helpers
import pairing
import raftsim
from cases import CASES, cfg_of
from raftsim import _abi

pytestmark = pytest.mark.gpu

SUMS = ["node_ticks"] + _abi.COUNTER_NAMES
VIOL = ("viol_election", "viol_log", "viol_complete")
MODES = ("amnesia", "durable")
AFTER = 15000
STORM = cfg_of("crash_storm_clients", 2048)
STORM_TICKS = 20000
STEADY = dict(n_clusters=1024, nodes=5, hb=300, el_base=500, el_span=500)
# Spec-Raft shapes of the case table whose logs fill (OVERFLOW halts), 64 clusters: N = 9 with the
# N = 7 shape's short log and odd arena, and that N = 7 shape itself
SPEC_OVERFLOW = {
    "n9": (dict(CASES["burst_faults_mid_n9"], variant_flags=2, n_clusters=64, log_cap=48,
                arena_cap=101), 2000),
    "n7": (dict(CASES["burst_arena_odd_n7"], variant_flags=2, n_clusters=64), 4000),
}


def deltas(after, before):
    return {k: after[k] - before[k] for k in SUMS}


def mask_of(ids):
    return sum(1 << i for i in ids)


def halted_of(h):
    """{cluster: [ids of its halted nodes]} and {fault code: nodes} from per-node reads."""
    halted, faults = {}, {}
    for i, r in enumerate(h.read_nodes()):
        if r["fault"]:
            halted.setdefault(i // h.N, []).append(i % h.N + 1)
            faults[r["fault"]] = faults.get(r["fault"], 0) + 1
    return halted, faults


def oracle_restart(ref, plan, mode):
    """plan: {cluster: node ids}. Returns the nodes restarted."""
    return sum(raftsim.restart_by_writes(ref, c, ids, mode) for c, ids in plan.items())


def parity(g, ref, clusters, what, sample=48):
    """Digests of every cluster; of (a sample of) `clusters` a gather of every part against the
    mirror of the oracle's reads and of the GPU handle's own per-node reads."""
    pairing.same(g, ref, what)
    cl = sorted(clusters)
    cl = cl[:sample // 2] + cl[-(sample // 2):] if len(cl) > sample else cl
    got = g.gather(cl).data
    assert np.array_equal(got, gm.pack_bytes(ref, cl)), f"{what}: gather against the oracle's mirror"
    assert np.array_equal(got, gm.pack_bytes(g, cl)), f"{what}: gather against per-node reads"


def run_on(g, ref, what, ticks=AFTER):
    g0, r0 = g.counters(), ref.counters()
    pairing.step(g, ref, ticks, what)
    assert deltas(g.counters(), g0) == deltas(ref.counters(), r0), what


def raw_write(g, clusters, masks, mode=0, n=None):
    """raft_restart_write as the C ABI has it: (return code, message)."""
    c = (ctypes.c_uint32 * max(1, len(clusters)))(*clusters)
    m = (ctypes.c_uint16 * max(1, len(masks)))(*masks)
    rc = g._restart["write"](g._h, c, m, len(clusters) if n is None else n, mode)
    return rc, g._fns["last_error"]().decode()


def raw_where(g, fault_mask, mode=0):
    rc = g._restart["where"](g._h, fault_mask, mode)
    return rc, g._fns["last_error"]().decode()


# ---- 1, 2: the faithful crash storm, list form and `where` form --------------------------------
@pytest.fixture(scope="module")
def storm():
    """The oracle's side of the storm, computed once: the halted nodes at STORM_TICKS (one cluster
    made all-halted, see the module's text), the digests after their AMNESIA restart, and the
    digests and counter deltas AFTER ticks on. `mirror` is an oracle handle just after the restart,
    kept for the mirror reads."""
    ref = pairing.oracle(STORM, ticks=STORM_TICKS)
    halted, faults = halted_of(ref)
    four = min(c for c, ids in halted.items() if len(ids) == STORM["nodes"] - 1)
    last = next(i for i in range(1, STORM["nodes"] + 1) if i not in halted[four])
    ours = dict(cluster=four, node=last)
    halt_node(ref, four, last)
    halted[four] = sorted(halted[four] + [last])
    n = oracle_restart(ref, halted, "amnesia")
    twin = pairing.oracle(STORM, ticks=STORM_TICKS)           # the mirror's source, not stepped on
    halt_node(twin, four, last)
    oracle_restart(twin, halted, "amnesia")
    at_once, c0 = ref.digest().copy(), ref.counters()
    ref.step(AFTER)
    out = dict(halted=halted, faults=faults, made=ours, nodes=n, at_once=at_once, mirror=twin,
               later=ref.digest().copy(), deltas=deltas(ref.counters(), c0))
    ref.close()
    yield out
    twin.close()


def halt_node(h, cluster, node_id):
    recs = h.read_nodes(cluster, 1)
    recs[node_id - 1]["fault"] = 2
    h.write_nodes(cluster, recs)


def storm_gpu(storm):
    g = helpers.gpu(**STORM)
    g.step(STORM_TICKS)
    total, recs = g.select(any=["halted"])
    assert total == len(recs) > 0
    halt_node(g, storm["made"]["cluster"], storm["made"]["node"])
    total, recs = g.select(any=["halted"])
    assert {r["cluster"]: r["halted"] for r in recs} == storm["halted"]
    return g, recs


def storm_check(g, storm, what):
    assert g.tick == STORM_TICKS
    assert np.array_equal(g.digest(), storm["at_once"]), f"{what}: digests at once"
    cl = sorted(storm["halted"])
    cl = cl[:24] + cl[-24:] + [storm["made"]["cluster"]]
    got = g.gather(cl).data
    assert np.array_equal(got, gm.pack_bytes(storm["mirror"], cl)), f"{what}: the oracle's mirror"
    assert np.array_equal(got, gm.pack_bytes(g, cl)), f"{what}: per-node reads"
    c0 = g.counters()
    g.step(AFTER)
    assert np.array_equal(g.digest(), storm["later"]), f"{what}: digests {AFTER} ticks on"
    assert deltas(g.counters(), c0) == storm["deltas"], what


def test_storm_list_form(storm):
    g, recs = storm_gpu(storm)
    # every fault code the storm produced is restarted, and a cluster whose every node is halted
    assert set(storm["faults"]) >= {1, 2, 4}
    assert any(len(r["halted"]) == g.N for r in recs)
    assert g.restart(recs) == storm["nodes"] == sum(len(r["halted"]) for r in recs)
    assert g.host_written and g.last_restart_ms() > 0
    assert g.select(any=["halted"])[0] == 0
    storm_check(g, storm, "list form")
    g.close()


def test_storm_where_form(storm):
    g, recs = storm_gpu(storm)
    assert g.restart_where() == sum(bin(mask_of(r["halted"])).count("1") for r in recs) == \
        storm["nodes"]
    assert g.last_restart_ms() > 0 and g.restart_where() == 0
    storm_check(g, storm, "where form")
    g.close()


# ---- 3: Spec-Raft with OVERFLOW halts ------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SPEC_OVERFLOW))
def test_spec_raft_overflow_halts(name, mode):
    cfg, ticks = SPEC_OVERFLOW[name]
    with pairing.pair(cfg) as (g, ref):
        pairing.step(g, ref, ticks, "the run up")
        halted, faults = halted_of(ref)
        assert set(faults) == {4} and len(halted) >= 8, faults
        total, recs = g.select(any=["halted"])
        assert {r["cluster"]: r["halted"] for r in recs} == halted
        if name == "n9":
            assert g.restart(recs, mode=mode) == sum(faults.values())
        else:
            assert g.restart_where(("overflow",), mode) == sum(faults.values())
        oracle_restart(ref, halted, mode)
        parity(g, ref, halted, f"{name} {mode} at once")
        run_on(g, ref, f"{name} {mode} later")
        viol = [g.counters()[k] for k in VIOL]
        print(f"{name} {mode}: violations (election, log, complete) {AFTER} ticks after the "
              f"restart: {viol}")
        assert viol == [ref.counters()[k] for k in VIOL]        # recorded, not asserted to be zero


# ---- 4: edges -----------------------------------------------------------------------------------
EDGES = {
    # one-slot inboxes, N = 2, an odd arena
    "n2_inbox1": dict(CASES["n2"], n_clusters=96, inbox_cap=1, log_cap=16, arena_cap=37,
                      client_ppm=20000, hb=30, el_base=50, el_span=50),
    # sixteen-slot inboxes, N = 9, an odd arena
    "n9_inbox16": dict(CASES["c4_n9"], n_clusters=64, inbox_cap=16, log_cap=64, arena_cap=131,
                       client_ppm=20000, client_redirects=4, hb=30, el_base=50, el_span=50,
                       dmax=50),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(EDGES))
def test_edges(name, mode):
    cfg = EDGES[name]
    N, Q = cfg["nodes"], cfg["inbox_cap"]
    with pairing.pair(cfg) as (g, ref):
        pairing.step(g, ref, 3000, "the run up")
        # full queues: at inbox_cap 1 they occur; at 16 a REQ ring is filled with client-sets by
        # the same write on both handles
        if Q == 16:
            for h in (g, ref):
                t = h.tick
                h.write_queue(3, 2, 0, [[t + i, 3, 0, 900 + i, 0, 0, 0, 0] for i in range(Q)])
        recs = ref.read_nodes()
        plan, sent, full = {}, 0, 0
        for c in range(ref.C):
            ids = set()
            for k in range(1, N + 1):
                # a node whose own append-entries with a payload are still queued at a peer
                for m in ref.read_queue(c, k, 0):
                    if (m[1] & 7) == 2 and m[1] >> 16:
                        ids.add((m[1] >> 3) & 15)
                        sent += 1
                if recs[c * N + k - 1]["req_count"] == Q or recs[c * N + k - 1]["res_count"] == Q:
                    ids.add(k)
                    full += 1
            plan[c] = sorted(ids or {c % N + 1})
        assert sent > 0 and full > 0, (sent, full)
        if Q == 16:
            assert 2 in plan[3]
        assert g.restart(list(plan), [mask_of(ids) for ids in plan.values()], mode) == \
            sum(map(len, plan.values()))
        oracle_restart(ref, plan, mode)
        parity(g, ref, plan, f"{name} {mode} at once", sample=96)
        run_on(g, ref, f"{name} {mode} later")


# ---- 5: a live leader crashed on the steady path ----------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_leader_crash_on_the_steady_path(mode):
    """test_gpu_clone.py's STEADY handle: after three steady launches certificates are set and the
    followers' draws are owed. A restart that left the certificate in place would let the steady
    kernel run the cluster from a first line that no longer describes it. A step is two launches of
    10,000 ticks: the first launch after the crash bails every cluster (they all elect), the path
    choice then takes the general kernel for the next two launches (launch_plan.hpp,
    STEADY_COOLDOWN) and returns to the steady kernel with the fourth."""
    with pairing.pair(STEADY, threads=8) as (g, ref):
        for _ in range(3):
            g.step(10000)
        ref.step(30000)
        assert g.diag_last_bails() >= 0                      # the steady path ran
        total, recs = g.select(all=["one_leader"])
        assert total == g.C
        before = ref.read_nodes()
        terms = {r["cluster"]: before[r["cluster"] * g.N + r["leaders"][0] - 1]["current_term"]
                 for r in recs}
        assert g.restart(recs, nodes=[r["leaders"] for r in recs], mode=mode) == g.C
        oracle_restart(ref, {r["cluster"]: r["leaders"] for r in recs}, mode)
        assert g.select(all=["one_leader"])[0] == 0
        parity(g, ref, range(g.C), f"{mode} at once")
        for step in range(3):
            run_on(g, ref, f"{mode} step {step}", ticks=20000)
        total, recs = g.select(all=["one_leader"])
        assert total == g.C, "every cluster re-elects"
        if mode == "durable":                                # the old term was kept and outbid
            assert all(r["term_max"] > terms[r["cluster"]] for r in recs)
        assert g.diag_last_bails() >= 0, "on the steady path again"


@pytest.mark.parametrize("mode", MODES)
def test_follower_crash_under_a_certificate(mode):
    """The same handle, a follower of every cluster restarted. Between two heartbeat rounds a
    restarted follower leaves the first line of its block as the strong certificate describes it
    (no message queued, a deadline ahead), so a certificate left in place would let the steady
    kernel run the cluster from that line alone and never see the follower's new term and flags
    (device.hpp: every writer of a block clears the certificate). The crashed leader above does
    not show this: its new deadline fails the line-0 path's own tests."""
    with pairing.pair(STEADY, threads=8) as (g, ref):
        for _ in range(3):
            g.step(10000)
        ref.step(30000)
        total, recs = g.select(all=["one_leader"])
        assert total == g.C
        plan = {r["cluster"]: [r["leaders"][0] % g.N + 1] for r in recs}
        idle = sum(all(n["req_count"] == 0 for n in ref.read_nodes(c, 1)) for c in range(0, g.C, 8))
        assert idle > g.C // 16, "clusters between two rounds"
        assert g.restart(list(plan), list(plan.values()), mode) == g.C
        oracle_restart(ref, plan, mode)
        parity(g, ref, range(g.C), f"{mode} at once")
        for step in range(3):
            run_on(g, ref, f"{mode} step {step}", ticks=20000)
        assert g.select(all=["one_leader"])[0] == g.C
        assert g.diag_last_bails() >= 0


# ---- 6: T = 0 identity ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 5, 9])
def test_amnesia_at_tick_0_is_the_identity(N):
    cfg = dict(n_clusters=333, nodes=N, seed=5, cluster_offset=17, client_ppm=1000)
    with pairing.closing(helpers.gpu(**cfg), helpers.gpu(**cfg)) as (g, twin):
        before, nodes = g.digest(), g.read_nodes()
        assert g.restart_where(("running",)) == 333 * N
        assert np.array_equal(g.digest(), before) and g.read_nodes() == nodes
        assert g.restart(range(333), [mask_of(range(1, N + 1))] * 333) == 333 * N
        assert np.array_equal(g.digest(), before) and g.read_nodes() == nodes
        for h in (g, twin):
            h.step(4000)
        assert np.array_equal(g.digest(), twin.digest()) and g.counters() == twin.counters()


# ---- 7: shards ------------------------------------------------------------------------------------
def test_shards():
    cfg = dict(CASES["fast_timers"], n_clusters=3001)
    with pairing.closing(helpers.gpu(**cfg), helpers.gpu(**cfg, n_devices=3),
                         helpers.gpu(**cfg), helpers.gpu(**cfg, n_devices=3)) as hs:
        one, three, one_w, three_w = hs
        for h in hs:
            h.step(3000)
        # shards [0, 1000), [1000, 2000), [2000, 3001): a list that crosses both boundaries upwards
        # and downwards, with a different mask per cluster
        clusters = [999, 1000, 1999, 2000, 1998, 1001, 998, 2001, 3000, 0, 1500, 2500, 500, 1002,
                    2002, 997]
        assert len(set(clusters)) == len(clusters) == 16
        shard = lambda c: min(c // 1000, 2)  # noqa: E731
        moves = {(shard(a), shard(b)) for a, b in zip(clusters, clusters[1:])}
        assert moves >= {(0, 1), (1, 0), (1, 2), (2, 1)}
        masks = [mask_of({i % 5 + 1, (i * 3) % 5 + 1}) for i in range(16)]
        before = one.digest()
        for h in (one, three):
            assert h.restart(clusters, masks, "durable") == sum(bin(m).count("1") for m in masks)
        d = one.digest()
        rest = np.setdiff1d(np.arange(3001), clusters)
        assert (d[clusters] != before[clusters]).all() and np.array_equal(d[rest], before[rest])
        assert np.array_equal(three.digest(), d)
        assert np.array_equal(one.gather(clusters).data, three.gather(clusters).data)
        # the `where` form over all three shards
        n = one_w.restart_where(("npe", "ioobe", "running"))
        assert n == three_w.restart_where(("npe", "ioobe", "running")) > 3001
        assert np.array_equal(one_w.digest(), three_w.digest())
        for h in hs:
            h.step(2000)
        assert np.array_equal(one.digest(), three.digest())
        assert np.array_equal(one_w.digest(), three_w.digest())
        assert one.counters() == three.counters() and one_w.counters() == three_w.counters()


# ---- 8: stream order --------------------------------------------------------------------------
def test_stream_order():
    cfg = dict(CASES["fast_timers"], n_clusters=600)
    with pairing.closing(helpers.gpu(**cfg), helpers.gpu(**cfg)) as (g, twin):
        clusters, masks = list(range(0, 600, 2)), [mask_of([c % 5 + 1]) for c in range(0, 600, 2)]
        for h in (g, twin):
            h.step(1000)
        g.step_async(3000)
        assert g.restart(clusters, masks) == 300             # no sync in between
        twin.step(3000)
        assert twin.restart(clusters, masks) == 300
        assert np.array_equal(g.digest(), twin.digest())
        g.step_async(500)
        n = g.restart_where(("running",), "durable")
        twin.step(500)
        assert twin.restart_where(("running",), "durable") == n > 0
        assert np.array_equal(g.digest(), twin.digest())


# ---- 9: refusals ----------------------------------------------------------------------------------
def test_refusals():
    cfg = dict(CASES["fast_timers"], n_clusters=8)
    with pairing.closing(helpers.gpu(**cfg)) as (g,):
        g.step(500)
        before = g.digest()
        rc, msg = raw_write(g, [4, 5, 8, 9], [2, 2, 2, 2])
        assert rc == -22 and "clusters[2] = 8" in msg        # the first offending position
        rc, msg = raw_write(g, [4, 5, 6, 5, 4], [2] * 5)
        assert rc == -22 and "clusters[3] = 5" in msg and "twice" in msg
        rc, msg = raw_write(g, [4, 5, 6], [2, 0, 0])
        assert rc == -22 and "nodes[1] = 0x0" in msg
        rc, msg = raw_write(g, [4, 5, 6], [2, 4, 3])
        assert rc == -22 and "nodes[2] = 0x3" in msg
        rc, msg = raw_write(g, [4, 5, 6], [64, 4, 2])
        assert rc == -22 and "nodes[0] = 0x40" in msg and "1..5" in msg
        rc, msg = raw_write(g, [4], [2], mode=2)
        assert rc == -22 and "mode" in msg
        rc, msg = raw_write(g, [8], [0], mode=2)             # the mode before the lists
        assert rc == -22 and "mode" in msg
        rc, msg = raw_write(g, [8, 8], [0, 0])               # the range before twice before masks
        assert rc == -22 and "clusters[0] = 8" in msg
        rc, msg = raw_write(g, [7, 7], [0, 0])
        assert rc == -22 and "twice" in msg
        null = g._restart["write"]
        assert null(g._h, None, (ctypes.c_uint16 * 1)(2), 1, 0) == -22
        assert null(g._h, (ctypes.c_uint32 * 1)(0), None, 1, 0) == -22
        for fm, mode, text in ((0, 0, "fault_mask"), (32, 1, "fault_mask"), (1, 2, "mode")):
            rc, msg = raw_where(g, fm, mode)
            assert rc == -22 and text in msg
        assert raw_write(g, [], [])[0] == 0 and raw_write(g, [9], [0], n=0)[0] == 0
        assert g.restart([]) == 0
        # through Python: shapes, with the position
        with pytest.raises(ValueError, match=r"targets\[1\] = 8"):
            g.restart([4, 8], [2, 2])
        with pytest.raises(ValueError, match=r"nodes\[0\] names node id 6"):
            g.restart([4], [[6]])
        with pytest.raises(ValueError, match="unknown fault"):
            g.restart_where(("oom",))
        with pytest.raises(ValueError, match="unknown restart mode"):
            g.restart_where(mode="lazarus")
        assert np.array_equal(g.digest(), before), "a refused restart wrote nothing"
        # -ERANGE: T + el_base + el_span at 2^32 - 1. The handle's own horizon (set_tick, step)
        # keeps every tick below it, so at the last tick it admits a restart still succeeds and the
        # deadline stays below "never"; the predicate's edge is tests/test_restart_host.py's
        longest = max(cfg["hb"], cfg["el_base"] + cfg["el_span"], cfg["dmax"])
        g.set_tick(2 ** 32 - 2 - longest)
        with pytest.raises(helpers.RaftSimError, match="rc=-34"):
            g.set_tick(2 ** 32 - 1 - longest)
        assert g.restart([1], [2]) == 1
        dl = g.read_nodes(1, 1)[0]["deadline"]
        assert g.tick + cfg["el_base"] <= dl < 2 ** 32 - 1


# ---- 10: what a restart leaves alone ------------------------------------------------------------
def test_what_a_restart_leaves_alone():
    cfg = dict(CASES["traced"], n_clusters=200, hb=30, el_base=50, el_span=50)   # rings, streams
    with pairing.closing(helpers.gpu(**cfg)) as (g,):
        g.step(6000)
        N = g.N
        clusters = list(range(0, 200, 3))
        node = {c: c % N + 1 for c in clusters}
        rest = np.setdiff1d(np.arange(200), clusters)
        before = dict(counters=g.counters(), viol=g.violations(), digest=g.digest(),
                      nodes=g.read_nodes(), clusters=g.read_clusters())
        assert before["viol"][0] > 0 and before["counters"]["entries_applied"] > 0
        traces = {c: [g.trace(c, k) for k in range(1, N + 1)] for c in clusters[:12]}
        streams = {c: [g.commit_stream(c, k) for k in range(1, N + 1)] for c in clusters}
        assert any(s for ss in streams.values() for s in ss)
        queues = {c: [[g.read_queue(c, k, w) for w in (0, 1)] for k in range(1, N + 1)]
                  for c in clusters}
        assert any((m[1] >> 3) & 15 == node[c] for c in clusters for k in range(N)
                   for w in (0, 1) for m in queues[c][k][w]), "messages of a restarted node queued"
        arenas = {c: [g.read_arena(c, k) for k in range(1, N + 1)] for c in clusters[:12]}
        T = g.tick
        assert g.restart(clusters, [mask_of([node[c]]) for c in clusters]) == len(clusters)
        assert g.tick == T and g.counters() == before["counters"] and g.violations() == before["viol"]
        assert g.read_clusters() == before["clusters"]       # hwm and the client cursor
        d = g.digest()
        assert np.array_equal(d[rest], before["digest"][rest]), "the unnamed clusters"
        after = g.read_nodes()
        for c in clusters:
            for k in range(1, N + 1):
                b, a = before["nodes"][c * N + k - 1], after[c * N + k - 1]
                if k == node[c]:
                    assert a == raftsim.restart_record(b, T, g.config, c, "amnesia", node_id=k)
                    assert a["commit_count"] == b["commit_count"]
                    assert g.read_queue(c, k, 0) == [] and g.read_queue(c, k, 1) == []
                else:
                    assert a == b, "another node's record"
                    assert [g.read_queue(c, k, w) for w in (0, 1)] == queues[c][k - 1]
                assert g.commit_stream(c, k) == streams[c][k - 1]
        for c in clusters[:12]:
            assert [g.trace(c, k) for k in range(1, N + 1)] == traces[c], "trace rings and seq"
            assert [g.read_arena(c, k) for k in range(1, N + 1)] == arenas[c], "no arena slot moves"
        # the next event of a restarted node continues its trace ring's seq
        g.step(3000)
        c = clusters[0]
        tr, was = g.trace(c, node[c]), traces[c][node[c] - 1]
        assert tr and was and tr[-1]["seq"] > was[-1]["seq"]
        assert [e["seq"] for e in tr] == list(range(tr[0]["seq"], tr[-1]["seq"] + 1))


# ---- 11: supervise ------------------------------------------------------------------------------
def test_supervise():
    with pairing.pair(STORM) as (g, ref):
        want = []
        for _ in range(5):
            ref.step(4000)
            want.append(oracle_restart(ref, halted_of(ref)[0], "amnesia"))
        assert raftsim.supervise(g, 20000, 4000) == want
        assert sum(want) > 0
        pairing.same(g, ref, "after five supervised rounds", counters=True)
