"""GPU parity: libraftsim.so (HIP, gfx950) against the C oracle, bit-exact per cluster.

Every cluster's canonical digest (SIM_SPEC §6: node records, queues, logs, arena cursors, trace
hashes, checker state) and every counter must match. On a mismatch the failing cluster is re-run
alone tick by tick on both sides and the first divergent tick is reported with both states.
"""
import numpy as np
import pytest

import helpers
import pairing
from cases import BURSTS, C4_BURSTS, CASES, FAULTS
from helpers import client_set_into

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_matches_oracle(name):
    cfg = CASES[name]
    with pairing.pair(cfg) as (g, r):
        pairing.run(g, r, [5000] * 4, bisect=cfg)
        cg = pairing.same_counters(g, r)
        assert cg["node_ticks"] == cfg["n_clusters"] * cfg["nodes"] * 20000


@pytest.mark.parametrize("seed", [1, 42, 0xDEADBEEF, 0x1_2345_6789])
def test_gpu_c2_full_size(seed):
    """BASELINE config 2: 65,536 five-node clusters, no faults, for the seeds of SURVEY §8(d) and
    one above 2^32 (Philox key word 1 nonzero): digest-equal after each of four 10k-tick launches.
    The first launch (elections) runs the steady kernel, which runs init-node's election in closed
    form, two timers firing together included (about 30 clusters per seed; only three together
    would be handed to the general body); the last one is the steady kernel alone on the
    256-workgroup grid with no cluster bailed (core.clj:91-139,105-123,141-149,162-169,181)."""
    cfg = dict(n_clusters=65536, nodes=5, seed=seed)
    bails = []
    with pairing.pair(cfg) as (g, r):
        for launch in range(4):
            g.step(10000)
            r.step(10000)
            bails.append(g.diag_last_bails())
            pairing.same(g, r, f"launch {launch}")
        pairing.same_counters(g, r)
    assert 0 <= bails[0] <= 2 and bails[-1] == 0, bails


@pytest.mark.parametrize("variant,nodes", [(0, 5), (2, 5), (3, 5), (0, 9), (2, 7), (2, 2), (2, 4),
                                           (2, 6), (2, 8)])
def test_gpu_storm_window(variant, nodes):
    """The STORM body (tick_wave.hpp): a fresh handle with client traffic runs the ticks before
    el_base -- where only client-sets at followers and their redirects can happen -- as a launch of
    its own, split off the first step; digest- and counter-equal to the oracle after it and after
    the elections that follow (core.clj:151-160 with server.clj:62-63; 166-169). A host write of the
    clock ends the storm ticks: the same step is then one launch, with the same results. (Spec-Raft
    at even N: no CASES entry runs tick_kernel<N, 0, SPEC, 0, STORM> there, and a handle whose
    state the host wrote has no storm ticks, so no fuzz or known-answer test does either.)"""
    cfg = dict(n_clusters=4096, nodes=nodes, seed=11 + variant, hb=400, el_base=1500, el_span=800,
               client_ppm=300000, client_period=4096, client_burst=1024, client_redirects=4,
               log_cap=256, variant_flags=variant, drop_ppm=50000, dmin=1, dmax=20)
    with pairing.pair(cfg, dict(ticks_per_launch=4000)) as (g, r):
        g.step(4000)
        r.step(4000)
        assert g.last_step_timing()[1] == 2              # [0, 1500) storm, then [1500, 4000)
        pairing.same(g, r, "storm step")
        g.step(4000)
        r.step(4000)
        assert g.last_step_timing()[1] == 1
        pairing.same(g, r, "second step")
        c = pairing.same_counters(g, r)
        assert c["redirects"] > 0 and c["leaders"] > 0
    with pairing.pair(cfg, dict(ticks_per_launch=4000)) as (g2, r2):
        g2.set_tick(0)                                   # a host write of the clock
        g2.step(4000)
        assert g2.last_step_timing()[1] == 1
        r2.step(4000)
        pairing.same(g2, r2, "step after set_tick(0)")


@pytest.mark.parametrize("variant,inbox,nodes", [(0, 16, 5), (2, 2, 5), (0, 16, 3), (2, 16, 9),
                                                 (0, 3, 9)])
def test_gpu_storm_engine(variant, inbox, nodes):
    """The storm kernel (storm_kernel.hip, one lane per cluster; handles of 131,072 clusters or
    more, every N from 2 to 9): storm launches split into chunks (rings carried across launches),
    with small inboxes whose overflowing clusters are rerun by the lane-per-node STORM body;
    digest- and counter-equal to the oracle through the storm ticks and the elections after them
    (core.clj:151-160, server.clj:62-63). The storm kernel's leftover list stays a minority with
    the default inbox (a regression to rerunning most clusters would show here)."""
    cfg = dict(n_clusters=131072, nodes=nodes, seed=21 + variant + nodes, el_base=3000,
               el_span=2000, client_ppm=200000, client_period=8192, client_burst=2048,
               client_redirects=4, inbox_cap=inbox, log_cap=128, variant_flags=variant,
               drop_ppm=100000, dmin=1, dmax=30, part_ppm=50000)
    bails = []
    with pairing.pair(cfg) as (g, r):
        for _ in range(4):
            g.step(1250)
            r.step(1250)
            if g.tick <= 3000 + 1250:
                bails.append(g.diag_storm_bails())
            pairing.same(g, r, "launch")
        pairing.same_counters(g, r)
    assert bails and min(bails) >= 0, bails              # the storm kernel ran every storm launch
    if inbox >= 16:
        assert max(bails) < 131072 // 4, bails


@pytest.mark.parametrize("nodes,d", [(2, 1), (3, 2), (4, 1), (5, 3), (5, 1)])
def test_gpu_init_election_closed_form(nodes, d):
    """The steady kernel's election from init-node (steady_kernel.hip) for every follower count
    and a delay above 1 (the electing vote response and the first append-response tick move with
    both): short timers so that elections, the first heartbeat rounds and the ties it hands to the
    general body all fall inside the first launch; digest- and counter-equal to the oracle after
    each launch, with few clusters bailed (core.clj:91-139,166-169)."""
    cfg = dict(n_clusters=16384, nodes=nodes, seed=7 + nodes, hb=300, el_base=700, el_span=900,
               dmin=d, dmax=d)
    bails = []
    with pairing.pair(cfg) as (g, r):
        for launch in range(3):
            g.step(3000)
            r.step(3000)
            bails.append(g.diag_last_bails())
            pairing.same(g, r, f"launch {launch}")
        pairing.same_counters(g, r)
    assert 0 <= bails[0] < 16384 // 20, bails


@pytest.mark.parametrize("mode", ["auto", "always", "never"])
@pytest.mark.parametrize("event", ["set_tick", "client_set", "client_cursor", "node_term",
                                   "node_log"])
def test_gpu_host_writes_after_lite_launches(event, mode, monkeypatch):
    """Host writes after 14 LITE launches (past the 8-launch packing period, with the packing
    reused between rebuilds): set_tick, a queued client-set and a finite client cursor (both clear
    LITE for the rest of the handle), and node records rewritten under clusters the steady kernel
    left with a certificate (a follower's term raised; a log entry given to a leader and committed:
    raft_sim_write_nodes clears the certificate, device.hpp) land at every phase of the rebuild
    cycle; GPU == oracle after each of the next 10 launches (raftsim.hip: packing keys and
    histogram stay consistent). With RAFTSIM_STEADY=never every launch runs the general body's
    LITE instance, so the node writes reach it without the steady kernel's catch-up."""
    monkeypatch.setenv("RAFTSIM_STEADY", mode)
    cfg = dict(n_clusters=4096, nodes=5, seed=42, ticks_per_launch=1000, log_cap=64)
    for phase in (0, 3):
        with pairing.pair(cfg) as (g, r):
            for _ in range(14 + phase):
                g.step(1000)
                r.step(1000)
            for be in (g, r):
                if event == "set_tick":
                    be.set_tick(be.tick + 777)
                elif event == "client_set":
                    for c in (5, 100, 4095):
                        client_set_into(be, c, 1 + c % 5, 1000 + c)
                elif event == "client_cursor":
                    be.write_clusters(7, [dict(hwm=(0, 0, 0), client_next=be.tick + 100,
                                               client_count=0)])
                else:
                    for c in (3, 200, 4000):
                        raw = be.read_nodes_raw(c, 1)
                        lead = next(i for i in range(5) if raw[i].role == 2)
                        if event == "node_term":           # a follower one term ahead
                            raw[(lead + 1) % 5].current_term += 1
                        else:                              # the leader's log gets a committed entry
                            be.write_arena(c, lead + 1, [(raw[lead].current_term, 77)])
                            raw[lead].log_len = 1
                            raw[lead].commit_index = 1
                            raw[lead].arena_base = 0
                            raw[lead].arena_frontier = 1
                        be.write_nodes(c, raw)
            pairing.run(g, r, [1000] * 10, "launch")
            pairing.same_counters(g, r)


@pytest.mark.parametrize("nodes,variant_flags,steady_mode,moved", [
    (3, 0, "never", 0), (5, 0, "never", 0), (5, 0, "always", 0), (7, 0, None, 0), (9, 0, None, 0),
    (6, 2, None, 0),
    (4, 0, "never", 1), (5, 0, "always", 1), (8, 0, None, 1), (9, 0, None, 1), (6, 2, None, 1)])
def test_gpu_host_written_logs_wrap_odd_arena(nodes, variant_flags, steady_mode, moved,
                                              monkeypatch):
    """Host-written logs that cross the end of an odd-sized arena, in fault-free handles: the only
    payloads a LITE launch ever sees. After 1,500 ticks every cluster with one running leader
    gets k entries written into that leader's arena at base = A - 1 - c % 5 (so the run wraps the
    arena's end, A = 51 or 37: no multiple of the 8-slot chunks), the older half one term back, a
    third of them uncommitted, a third half committed. The next heartbeats ship them: P3 copies
    them into every follower's arena and P4 compares them one entry per round trip
    (arena_copy<1>, W = 1) in tick_kernel<N, 0, 0, LITE> -- forced at N <= 5, the only path at
    N >= 7 -- through the steady kernel's catch-up (always), and in the Spec-Raft N = 6 kernel.
    The faithful leader (next-index 0) ships the entries from the second on, which an empty
    follower appends at position 0, one off the leader's log: a log-matching violation; every
    later heartbeat re-sends the last entry and the follower appends it again (core.clj:105-123
    truncates nothing) until its log reaches log_cap: OVERFLOW halts inside the same kernels;
    Spec-Raft appends each entry once. GPU == oracle after each of six more launches, and every
    counter at the end.

    moved: the other nodes' logs are moved to the arena's last slots too (base = A - 2 -
    (c + i) % 3), and in even clusters they hold the leader's first entry. Without it only the
    leader's arena wraps (the followers append from slot 0 and halt at log_cap <= A / 2: P3's
    destination and the appender's side of P4's compare never cross an arena's end), and every
    append that P4 compares across a wrap is one the leader's shifted log flags anyway: a compare
    that wrapped either log to the wrong slot passed every case. In the even clusters the first
    append crosses the followers' wrap and leaves logs equal to the leader's: no violation there
    (asserted on the oracle), so a wrong compare shows as one."""
    if steady_mode is None:
        monkeypatch.delenv("RAFTSIM_STEADY", raising=False)
    else:
        monkeypatch.setenv("RAFTSIM_STEADY", steady_mode)
    L, A, k = (16, 37, 16) if nodes == 9 else (24, 51, 10)
    cfg = dict(n_clusters=192, nodes=nodes, seed=200 + nodes, hb=60, el_base=100, el_span=100,
               log_cap=L, arena_cap=A, ticks_per_launch=500, commit_stream_cap=5,
               variant_flags=variant_flags)
    if nodes == 9:
        cfg.update(dmin=3, dmax=3)
    with pairing.pair(cfg) as (g, r):
        pairing.step(g, r, 1500)
        before = r.counters()
        recs = r.read_nodes()
        written = clean = 0
        for c in range(cfg["n_clusters"]):
            leads = [i for i in range(nodes)
                     if recs[c * nodes + i]["role"] == 2 and recs[c * nodes + i]["fault"] == 0]
            if len(leads) != 1:
                continue
            lead = leads[0]
            written += 1
            clean += c % 2 == 0
            base = A - 1 - c % 5
            for be in (g, r):
                raw = be.read_nodes_raw(c, 1)
                term = raw[lead].current_term
                arena = [(0, 0)] * A
                for j in range(k):
                    arena[(base + j) % A] = (term if j >= k // 2 else max(1, term - 1), 1000 * c + j)
                be.write_arena(c, lead + 1, arena)
                raw[lead].log_len = k
                raw[lead].commit_index = (c % 3) * (k // 2)
                raw[lead].arena_base = base
                raw[lead].arena_frontier = base + k
                for i in range(nodes if moved else 0):
                    if i == lead or raw[i].log_len:
                        continue
                    fb = A - 2 - (c + i) % 3
                    raw[i].arena_base = raw[i].arena_frontier = fb
                    if c % 2 == 0:
                        be.write_arena(c, i + 1, [(0, 0)] * fb + [arena[base % A]])
                        raw[i].log_len = 1
                        raw[i].arena_frontier = fb + 1
                be.write_nodes(c, raw)
        pairing.same(g, r, "state load")
        pairing.run(g, r, [500] * 6, "launch")
        cr = pairing.same_counters(g, r)
        # witnesses, on the oracle's counters: the written logs were shipped whole and, in the
        # faithful model, re-appended until logs overflowed
        assert written >= 150
        assert cr["entries_appended"] - before["entries_appended"] >= 150 * (nodes - 1) * (k - 1)
        if variant_flags == 0:
            assert cr["halt_overflow"] > 0 and cr["viol_log"] > 0
        if moved and variant_flags == 0:     # one violation per follower, in the odd clusters alone
            assert clean >= 75 and cr["viol_log"] == (written - clean) * (nodes - 1)
        if steady_mode is not None:
            assert (g.diag_last_bails() >= 0) == (steady_mode == "always")


@pytest.mark.parametrize("nodes", [7, 9])
def test_gpu_c4_logs_reach_capacity(nodes):
    """BASELINE config 4 to its end: 4096-entry logs fill up under the bursty client, append-entries
    carry 1000+ entries (core.clj:56-67 ships the whole suffix), and OVERFLOW halts appear (D8);
    GPU == oracle on every cluster, counter and the payload maximum."""
    cfg = dict(n_clusters=64, nodes=nodes, seed=7 + nodes, **C4_BURSTS)
    with pairing.pair(cfg) as (g, r):
        pairing.run(g, r, [55000] * 2, bisect=cfg)
        cg = pairing.same_counters(g, r)
        assert cg["payload_max"] >= 1000 and cg["halt_overflow"] > 0
        assert max(n["log_len"] for n in g.read_nodes()) >= 3000


def test_gpu_sharded_handle_equals_single():
    """n_devices = 3 (three shards; on a one-GPU box they share the device) reproduces the
    one-shard handle: digests, counters, reads that cross shard boundaries, and resume."""
    cfg = dict(n_clusters=1000, nodes=5, seed=71, client_ppm=80000, log_cap=256, **BURSTS,
               **FAULTS)
    one, three = helpers.gpu(**cfg), helpers.gpu(n_devices=3, **cfg)
    for s in (one, three):
        s.step(20000)
    assert np.array_equal(one.digest(), three.digest())
    assert one.counters() == three.counters()
    assert one.read_nodes(300, 100) == three.read_nodes(300, 100)
    assert one.read_clusters(330, 10) == three.read_clusters(330, 10)
    for c in (332, 333, 334, 666, 667):
        for i in (1, 5):
            assert one.read_queue(c, i, 0) == three.read_queue(c, i, 0)
            assert one.log(c, i) == three.log(c, i)


def test_gpu_printed_trace_matches_oracle():
    """F3: the `; Node` / `; Message` dump (core.clj:182-186) of GPU-recorded events equals the
    oracle's, text for text, on a faulty client-driven run."""
    cfg = dict(n_clusters=8, nodes=5, seed=35, client_ppm=3000, log_cap=256, trace_cap=4096,
               trace_entry_cap=1 << 15, **FAULTS)
    g, r = helpers.gpu(**cfg), helpers.oracle(**cfg)
    g.step(20000)
    r.step(20000)
    n_entries = 0
    for c in range(cfg["n_clusters"]):
        for i in range(1, 6):
            tg = g.edn_trace(c, i)
            assert tg == r.edn_trace(c, i), (c, i)
            n_entries += tg.count(":val ")
    assert n_entries > 0


def test_gpu_spec_raft_safety_at_scale():
    """BASELINE config 5 shape on the GPU: 65,536 Spec-Raft clusters with faults, client traffic
    and fast timers show no violation (control), while the same clusters with the up-to-date vote
    check dropped do; both bit-exact against the oracle on a sampled slice."""
    base = dict(n_clusters=65536, nodes=5, seed=51, client_ppm=5000, log_cap=256, hb=300,
                el_base=500, el_span=500, **FAULTS)
    ctl, bug = helpers.gpu(variant_flags=2, **base), helpers.gpu(variant_flags=3, **base)
    for s in (ctl, bug):
        s.step(20000)
    c, b = ctl.counters(), bug.counters()
    assert c["leaders"] > 100000 and c["viol_election"] == c["viol_log"] == c["viol_complete"] == 0
    assert b["viol_complete"] > 0 and b["first_violation_tick"] is not None
    lo = 4096
    for flags, sim in ((2, ctl), (3, bug)):
        r = pairing.oracle(dict(base, n_clusters=lo, variant_flags=flags))
        r.step(20000)
        assert np.array_equal(sim.digest(0, lo), r.digest())


def test_gpu_shard_invariance():
    """Two handles over disjoint cluster ranges reproduce one handle over both (D13)."""
    base = dict(nodes=5, seed=99, client_ppm=1000, log_cap=128, **FAULTS)
    whole = helpers.gpu(n_clusters=600, **base)
    lo = helpers.gpu(n_clusters=250, cluster_offset=0, **base)
    hi = helpers.gpu(n_clusters=350, cluster_offset=250, **base)
    for s in (whole, lo, hi):
        s.step(12000)
    assert np.array_equal(whole.digest(), np.concatenate([lo.digest(), hi.digest()]))
    cw, cl, ch = whole.counters(), lo.counters(), hi.counters()
    for k in cw:
        if k == "first_violation_tick":
            vals = [v for v in (cl[k], ch[k]) if v is not None]
            assert cw[k] == (min(vals) if vals else None)
        elif k == "payload_max":
            assert cw[k] == max(cl[k], ch[k])
        else:
            assert cw[k] == cl[k] + ch[k], k


def test_gpu_write_state_roundtrip():
    """State written through the ABI reads back identically and steps like the oracle."""
    cfg = dict(n_clusters=64, nodes=5, seed=3, client_ppm=3000, log_cap=64, **FAULTS)
    src = helpers.oracle(**cfg)
    src.step(15000)
    g = helpers.gpu(**cfg)
    r = helpers.oracle(**cfg)
    for be in (g, r):
        be.set_tick(15000)                       # resume: deadlines are absolute ticks
        be.write_nodes(0, src.read_nodes_raw())
        be.write_clusters(0, src.read_clusters())
        for c in range(cfg["n_clusters"]):
            for i in range(1, 6):
                be.write_arena(c, i, src.read_arena(c, i))
                for w in (0, 1):
                    be.write_queue(c, i, w, src.read_queue(c, i, w))
    assert np.array_equal(g.digest(), src.digest())
    for be in (g, r, src):
        be.step(8000)
    assert np.array_equal(g.digest(), r.digest())
    assert np.array_equal(g.digest(), src.digest())     # resumed == never stopped


def test_gpu_multi_launch_step():
    """One raft_sim_step spanning several launches (ticks_per_launch < n_ticks) equals the oracle."""
    cfg = dict(n_clusters=512, nodes=5, seed=81, client_ppm=20000, log_cap=64,
               ticks_per_launch=3000, **BURSTS, **FAULTS)
    with pairing.pair(cfg, threads=1) as (g, r):
        pairing.step(g, r, 17000, counters=True)
        assert g.tick == 17000


def test_gpu_tick_horizon():
    """No deadline or arrival may wrap past 2^32 (SIM_SPEC D1): steps that could are refused."""
    g = helpers.gpu(n_clusters=64, nodes=5, seed=1)
    top = 2 ** 32 - 1 - 10000        # the longest timer is el_base + el_span = 10000
    g.set_tick(top - 3000)
    g.step(2999)
    with pytest.raises(helpers.RaftSimError, match="2\\^32"):
        g.step(2)
    g.step(0)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [
    dict(n_clusters=4096, nodes=5, seed=42),
    dict(n_clusters=2048, nodes=7, seed=3, client_ppm=20000, log_cap=128, **FAULTS),
    dict(n_clusters=1024, nodes=5, seed=41, client_ppm=2000, log_cap=256, variant_flags=2,
         commit_stream_cap=64, **FAULTS),
    # N >= 7 with client traffic: the burst engine's ticks feed the packing key (tick_wave.hpp)
    CASES["burst_faults_mid_n7"],
    CASES["burst_faults_c4_n9"],
], ids=["c2_shape", "faults_n7", "spec", "burst_faults_mid_n7", "burst_faults_c4_n9"])
def test_gpu_schedule_invariance(cfg):
    """RAFT_SCHED_ALIGNED (clusters regrouped onto waves by next event before every launch) and
    RAFT_SCHED_FIXED produce the same per-cluster digests and counters, launch by launch."""
    a = helpers.gpu(**cfg, schedule=0, ticks_per_launch=2500)
    b = helpers.gpu(**cfg, schedule=1, ticks_per_launch=2500)
    for _ in range(4):
        a.step(5000)
        b.step(5000)
        assert np.array_equal(a.digest(), b.digest())
        assert a.counters() == b.counters()


@pytest.mark.gpu
def test_gpu_step_async_matches_step():
    """K raft_sim_step_async calls + one raft_sim_sync leave the same state, counters and tick as
    K synchronous raft_sim_step calls, and the timing covers every launch of the K steps."""
    cfg = dict(n_clusters=2048, nodes=5, seed=9, client_ppm=5000, log_cap=128,
               ticks_per_launch=3000, **FAULTS)
    a, b = helpers.gpu(**cfg), helpers.gpu(**cfg)
    for _ in range(4):
        a.step(5000)
        b.step_async(5000)
    b.sync()
    assert a.tick == b.tick == 20000
    assert np.array_equal(a.digest(), b.digest())
    assert a.counters() == b.counters()
    ms, launches = b.last_step_timing()
    assert launches == 8 and ms > 0


@pytest.mark.parametrize("ppm", [0, 30000])
def test_gpu_host_written_client_cursor(ppm):
    """A client cursor written by the host (checkpoint/resume through raft_sim_write_clusters) is
    honoured like any other, also with client_ppm = 0, where every power of the gap search is
    2^32 and the next injection never comes (SIM_SPEC §4 P0)."""
    cfg = dict(n_clusters=64, nodes=5, seed=77, client_ppm=ppm, log_cap=64)
    recs = [dict(hwm=(0, 0, 0), client_next=100 + 37 * i, client_count=i) for i in range(64)]
    with pairing.pair(cfg, threads=1) as (g, r):
        g.write_clusters(0, recs)
        r.write_clusters(0, recs)
        pairing.run(g, r, [4000] * 3)
        assert pairing.same_counters(g, r)["client_injected"] >= 64


def test_gpu_steady_path_taken():
    """C2 from init-node: the first launch takes the steady path with the elections in closed form
    (at most a couple of tied clusters bailed to the general body); once every cluster has its
    leader the steady kernel runs every cluster alone (0 bails); the state equals the oracle's
    after every launch."""
    cfg = dict(n_clusters=8192, nodes=5, seed=83)
    bails = []
    with pairing.pair(cfg) as (g, r):
        for launch in range(4):
            g.step(10000)
            r.step(10000)
            bails.append(g.diag_last_bails())
            pairing.same(g, r, f"launch {launch}")
        pairing.same_counters(g, r)
    assert 0 <= bails[0] <= 2 and bails[-1] == 0, bails


LITE_CASES = ["c2_small", "lite_n2", "lite_n3", "lite_n4", "lite_elections", "lite_tiny_inbox",
              "lite_odd_launches", "lite_short_round"]


@pytest.mark.parametrize("name", LITE_CASES)
def test_gpu_forced_steady_matches_oracle(name, monkeypatch):
    """Every LITE launch on the steady kernel (RAFTSIM_STEADY=always), from init-node: elections
    and every other event outside its model go through the workgroup's catch-up (the general
    tick body over the clusters it bailed, several wave slots per wave); GPU == oracle after
    every chunk."""
    monkeypatch.setenv("RAFTSIM_STEADY", "always")
    cfg = CASES[name]
    with pairing.pair(cfg) as (g, r):
        pairing.run(g, r, [5000] * 4, bisect=cfg)
        pairing.same_counters(g, r)
        assert g.diag_last_bails() >= 0      # the last launch took the steady path


@pytest.mark.parametrize("name", LITE_CASES)
def test_gpu_forced_general_matches_oracle(name, monkeypatch):
    """Every LITE launch at N <= 5 on the general body's LITE instance, tick_kernel<N, 0, 0, LITE>
    (RAFTSIM_STEADY=never), from init-node: the kernel that auto mode runs only in the cool-down
    launches after a steady launch bailed more than 1/16 of its clusters; GPU == oracle after
    every chunk."""
    monkeypatch.setenv("RAFTSIM_STEADY", "never")
    cfg = CASES[name]
    with pairing.pair(cfg) as (g, r):
        pairing.run(g, r, [5000] * 4, bisect=cfg)
        pairing.same_counters(g, r)
        bails = g.diag_last_bails()
    print(f"{name}: diag_last_bails {bails}")
    assert bails == -1                       # the last launch did not take the steady path
