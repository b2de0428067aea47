"""The N >= 7 burst engine (tick_wave.hpp BURST) against the C oracle where test_gpu_parity's
cases cannot reach: the launch-wide 2^28 gate of its 28-bit arrival packing, host-written messages
in a leader's REQ queue when a burst starts (the entry filter for a queued message), and shards.
tests/test_burst_witness.py shows on the oracle that the inputs reach the engine's states.
"""
import numpy as np
import pytest

import helpers
import pairing
from cases import B4, CASES, FAST, GATE_CFG, GATE_T0, GATE_TICKS, gate_setup

pytestmark = pytest.mark.gpu


def test_gpu_burst_gate_2_28():
    """Launches that end at or before tick 2^28 - 1 run with the engine on, the launch that
    straddles it and the later ones with it off (its arrivals are packed in 28 bits): bursts with
    mild faults from 15,000 ticks before the gate to 9,000 past it, digest-equal to the oracle
    after every 2,500-tick launch and counter-equal at the end. The oracle alone shows 5489 / 8936
    engine-eligible samples below / above the gate (test_burst_witness.py)."""
    cfg, T0 = GATE_CFG, GATE_T0
    with pairing.pair(cfg) as (g, r):
        for be in (g, r):
            be.set_tick(T0)
            gate_setup(be)
        pairing.run(g, r, pairing.chunks(GATE_TICKS, 2500), "launch")
        assert g.tick == T0 + GATE_TICKS > 2 ** 28
        cg = pairing.same_counters(g, r)
        assert cg["client_injected"] > 0 and cg["payload_max"] >= 500 and cg["dropped"] > 0


HOST_CFG = dict(n_clusters=192, nodes=7, seed=141, ticks_per_launch=1000, **B4, **FAST)
HOST_STOP = 4090          # the client's second burst starts at tick 4096
CPW = 64 // HOST_CFG["nodes"]      # clusters per wave (tick_kernel.hip); id order with schedule=1


def _host_messages(tick, cnext, leader, N):
    """(name, the leader's REQ queue) per variant; words: arrival hdr term a b eterm eval poff.
    `cnext` is the cluster's next injection tick, `leader` the leader's id."""
    peer = leader % N + 1
    return [
        # due client-sets: the engine is entered at `tick` with the message in its ring, and the
        # leader takes it in that tick
        ("plain", [[tick, 3, 0, 9001, 0, 0, 0, 0]]),
        ("hops15", [[tick, 3, 0, 9002, 15, 0, 0, 0]]),     # the most hops the ring's packing holds
        # words the engine's ring does not hold (the filter keeps such a cluster with the tick
        # loop, whose trace hash takes the term word)
        ("hops16", [[tick, 3, 0, 9003, 16, 0, 0, 0]]),
        ("term7", [[tick, 3, 7, 9005, 0, 0, 0, 0]]),
        # arrives three ticks after the burst's first injection: at that injection's tick the
        # leader holds a message that is not due, and the engine must not take it early
        ("future", [[cnext + 3, 3, 0, 9004, 0, 0, 0, 0]]),
        # a due message that is no client-set: a stale request-vote from a peer (term 0 and no
        # other word set, so that the header alone tells it from a client-set)
        ("request_vote", [[tick, 1 | peer << 3, 0, 0, 0, 0, 0, 0]]),
        ("two", [[tick, 3, 0, 9006, 0, 0, 0, 0], [tick + 1, 3, 0, 9007, 1, 0, 0, 0]]),   # rq.c > 1
    ]


@pytest.mark.parametrize("schedule", [1, 0], ids=["fixed", "aligned"])
def test_gpu_burst_host_written_leader_messages(schedule):
    """Messages written by the host into a leader's REQ queue six ticks before a burst, in
    clusters that meet the engine's entry condition, two clusters per variant (one for the last):
    a due client-set, which enters the engine's ring with the cluster; one with 15 hops; one with
    16 hops, which the ring's packing does not hold; one with a nonzero term word (`term == 0`);
    a client-set that arrives three ticks after the cluster's first injection: at that tick
    the entry filter meets a queued message that is not due (`arrival <= t`; taking it appends its
    value three ticks early); a due request-vote (`hdr == CLIENT_SET`; taking it appends a value
    and loses the vote response); and two queued client-sets (rq.c > 1, the entry condition).
    Digest-equal to the oracle after three 1,000-tick launches and one of 37 ticks, counter-equal
    at the end.

    A cluster enters the engine only if the clusters of its wave that stay with the tick loop
    have no event in the next 16 ticks (tick_wave.hpp `tlim`, BURST_MIN). With the fixed schedule
    a wave holds CPW clusters in id order, so each variant gets a wave of its own in which every
    cluster is quiet until well into the burst (checked on the oracle): the written clusters then
    reach the filter whatever it decides. Under the aligned schedule the packing decides the wave
    mates; the test runs under both.

    Of the filter's terms this pins `hdr == CLIENT_SET`, `term == 0` (the tick loop's trace hash
    takes the term word, the engine's does not) and `arrival <= t`. `b < 16` and the zero tail
    words are not pinned: the leader takes a due client-set in the tick at which the engine is
    entered, where the hop count is not read, so the 15- and 16-hop variants check only that
    nothing else goes wrong with them."""
    cfg = dict(HOST_CFG, schedule=schedule)
    with pairing.pair(cfg) as (g, r):
        pairing.step(g, r, HOST_STOP)
        N, C, tick = cfg["nodes"], cfg["n_clusters"], r.tick
        recs, cl = r.read_nodes(), r.read_clusters()

        def quiet(c):
            """An idle leader and followers with nothing to do until 16 ticks into the burst."""
            nodes, cnext = recs[c * N:(c + 1) * N], cl[c]["client_next"]
            lk = helpers.burst_leader(nodes, tick)
            return (lk is not None and nodes[lk]["req_count"] == 0 and tick < cnext < tick + 16
                    and all(n["deadline"] > cnext + 16 for n in nodes if not n["fault"]))

        waves = [w for w in range(C // CPW)
                 if all(quiet(c) for c in range(CPW * w, CPW * w + CPW))]
        assert len(waves) >= 7, waves  # measured on the oracle: 9 of 21 waves, 177 quiet clusters
        targets = []
        for v, w in enumerate(waves[:7]):
            for c in range(CPW * w, CPW * w + (1 if v == 6 else 2)):
                leader = 1 + helpers.burst_leader(recs[c * N:(c + 1) * N], tick)
                name, msgs = _host_messages(tick, cl[c]["client_next"], leader, N)[v]
                targets.append((name, c, leader))
                for be in (g, r):
                    be.write_queue(c, leader, 0, msgs)
        assert len(targets) == 13 and targets[-1][0] == "two"
        for name, c, leader in targets:
            assert g.read_queue(c, leader, 0) == r.read_queue(c, leader, 0), name
        pairing.same(g, r, "the written queues")
        before = r.counters()
        pairing.run(g, r, (1000, 1000, 1000, 37), "launch")
        cg = pairing.same_counters(g, r)
        for k in ("client_injected", "redirects", "entries_appended", "ev_rv"):   # the burst ran
            assert cg[k] > before[k], k
        for name, c, leader in targets:                               # the written values' fate
            log = r.log(c, leader)
            assert g.log(c, leader) == log, name
            if name == "future":            # appended behind the burst's first client-set
                assert 9004 in [v for _, v in log[1:]], log[:8]


def test_gpu_burst_sharded_handle_equals_single():
    """burst_faults_mid_n9 on three shards (on a one-GPU box they share the device) reproduces the
    one-shard handle: digests, counters, and queue and log reads across shard boundaries."""
    cfg = CASES["burst_faults_mid_n9"]
    one, three = helpers.gpu(**cfg), helpers.gpu(n_devices=3, **cfg)
    for _ in range(4):
        for s in (one, three):
            s.step(5000)
        assert np.array_equal(one.digest(), three.digest())
    assert one.counters() == three.counters()
    assert one.read_nodes(80, 12) == three.read_nodes(80, 12)       # 256 clusters: 85 | 85 | 86
    assert one.read_clusters(168, 6) == three.read_clusters(168, 6)
    for c in (84, 85, 86, 169, 170, 171):
        for i in (1, 9):
            assert one.read_queue(c, i, 0) == three.read_queue(c, i, 0)
            assert one.read_queue(c, i, 1) == three.read_queue(c, i, 1)
            assert one.log(c, i) == three.log(c, i)
