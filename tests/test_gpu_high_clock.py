"""GPU parity at high clocks: every kernel family across tick 2^31 and up to the horizon.

The clock is a 32-bit absolute tick; deadlines, arrivals, client cursors, violation records and
trace events all hold absolute ticks. Each case here runs from a fresh handle moved to a base tick
(tests/high_clock.py): LOW (the control), SIGN with a launch boundary on 2^31 (sign0) and with
2^31 inside a launch (sign7), and TOP, whose last step ends on the last tick a step may end at
(after it one more tick is refused on both sides). Every comparison is bit-exact against the C
oracle, which tests/test_high_clock_oracle.py holds to pyref's Python integers at the same bases
and whose counters it shows to be far from trivial for every configuration below.

Shapes: 256 clusters (512 where stated), short timers (hb 40, election 60 + 60), delays up to 10,
6,000 ticks in launches of 1,500 unless stated.
"""
import numpy as np
import pytest

import audit_oracle
import census_oracle
import gather_mirror as gm
import helpers
import high_clock as hc
import raftsim
from raftsim import ClusterPack
from test_gpu_parity import B4, FAST
from test_gpu_steady_line0 import both, cut_cfg
from viol_oracle import KINDS, as_records, expected_records, expected_window

pytestmark = pytest.mark.gpu

C = 256
TICKS, LAUNCH = 6000, 1500
CHUNKS = [LAUNCH] * (TICKS // LAUNCH)
SHORT = dict(hb=40, el_base=60, el_span=60)
NET = dict(drop_ppm=100000, dup_ppm=10000, dmin=1, dmax=10, part_ppm=100000)
CLIENTS = dict(client_ppm=20000, client_period=4096, client_burst=1024, client_redirects=4,
               log_cap=256)


def case(**kw):
    return dict(dict(n_clusters=C, ticks_per_launch=LAUNCH, **SHORT), **kw)


FAULTS_N5 = case(nodes=5, seed=301, part_epoch=7, **NET)
CLIENTS_N5 = case(nodes=5, seed=303, part_epoch=7, **CLIENTS, **NET)

# name -> config; the comment names the kernel family the case reaches
GENERAL = {
    # tick_kernel<5, 0, 0, 0>: the faithful N = 5 body with drops, duplicates, partitions
    "faults_n5": FAULTS_N5,
    "clients_n5": CLIENTS_N5,
    # tick_kernel<N, 0, 0, 0> for the other node counts (the n2..n8 shapes)
    "n2": case(nodes=2, seed=19, client_ppm=500, **NET),
    "n3": case(nodes=3, seed=21, client_ppm=500, **NET),
    "n4": case(nodes=4, seed=23, client_ppm=500, **NET),
    "n6": case(nodes=6, seed=25, client_ppm=500, **NET),
    "n8": case(nodes=8, seed=27, client_ppm=500, **NET),
    # N >= 7 at config-4 burst rates: above tick 2^28 the burst engine is gated off and the tick
    # loop carries the bursts (at LOW the engine itself runs them)
    "burst_n7": case(nodes=7, seed=103, **B4, **FAST, **NET),
    "burst_n9": case(nodes=9, seed=105, **B4, **FAST, **NET),
    "burst_n8_inbox2": case(nodes=8, seed=111, inbox_cap=2, **B4, **FAST, **NET),
    # ... and with the short timers: after the overdue-fresh start the long ones leave few leaders
    # in 6,000 ticks, these have one in a quarter of the clusters when the bursts come
    "burst_n7_short": case(nodes=7, seed=103, **B4, **NET),
    "burst_n9_short": case(nodes=9, seed=105, **B4, **NET),
    # Spec-Raft bodies, tick_kernel<N, 0, SPEC, 0>, and the two bug variants (they violate)
    "spec_n5": case(nodes=5, seed=41, client_ppm=2000, log_cap=256, variant_flags=2,
                    commit_stream_cap=64, **NET),
    "spec_n8": case(nodes=8, seed=45, client_ppm=2000, log_cap=256, variant_flags=2, **NET),
    "variant1_n5": case(nodes=5, seed=9, client_ppm=20000, log_cap=128, variant_flags=1, **NET),
    "spec_nolog_n5": case(nodes=5, seed=43, client_ppm=20000, log_cap=256, variant_flags=3,
                          **NET),
    # overflowing two-slot inboxes under heavy duplication; an arena that is no multiple of the
    # 8-slot chunks
    "overflow": case(nodes=9, seed=11, inbox_cap=2, dup_ppm=300000, dmax=3, client_ppm=5000,
                     log_cap=64),
    "arena_odd": case(nodes=5, seed=14, client_ppm=20000, log_cap=16, arena_cap=37,
                      dup_ppm=100000, dmax=10, commit_stream_cap=5),
    # launches of 7 ticks; both schedules (the wave packing's sched_bucket(ev, t0))
    "tiny_launches": dict(CLIENTS_N5, seed=17, ticks_per_launch=7),
    "sched_aligned": dict(CLIENTS_N5, schedule=0),
    "sched_fixed": dict(CLIENTS_N5, schedule=1),
    # the partition epoch's divisor
    "epoch_1": dict(FAULTS_N5, part_epoch=1),
    "epoch_3": dict(FAULTS_N5, part_epoch=3),
    "epoch_1000": dict(FAULTS_N5, part_epoch=1000),
    "epoch_65537": dict(FAULTS_N5, part_epoch=65537),
    "epoch_2p31": dict(FAULTS_N5, part_epoch=2 ** 31 + 3),
    # the client schedule's divisors: a short period, and one above 2^31 (at TOP its next window
    # starts past the clock: the cursor saturates at "never" and nothing is injected)
    "period_37": dict(CLIENTS_N5, client_period=37, client_burst=11),
    "period_2p31": dict(CLIENTS_N5, client_period=2 ** 31 + 5, client_burst=2 ** 30 + 1),
    # fault-free, client-free handles at N >= 6: tick_kernel<N, 0, *, LITE> (and the Spec-Raft
    # N = 6 instance with heartbeats slower than the election timer)
    "lite_n6": case(nodes=6, seed=171),
    "lite_n7_d4": case(nodes=7, seed=173, dmin=4, dmax=4),
    # (nine timers firing together overflow four-slot inboxes for good: lite_n9_inbox4 elects
    # almost nobody and runs elections and overflow throughout; lite_n9 settles)
    "lite_n9_inbox4": case(nodes=9, seed=177, inbox_cap=4),
    "lite_n9": case(nodes=9, seed=179),
    "spec_lite_n6_elections": case(nodes=6, seed=191, hb=70, el_base=50, el_span=40, dmin=3,
                                   dmax=3, variant_flags=2),
}
# trace rings on (they enter the digest): tick_kernel<N, TRACE, 0, 0>
TRACED = {
    "traced_n5": case(nodes=5, seed=31, client_ppm=2000, log_cap=128, trace_cap=48,
                      trace_entry_cap=300, commit_stream_cap=16, **NET),
    "traced_n6": case(nodes=6, seed=189, dmin=2, dmax=2, trace_cap=16, trace_entry_cap=8),
}
# the violating cases the queries run on
QUERIES = {
    "variant1_n5": GENERAL["variant1_n5"],
    "spec_nolog_n5_512": dict(GENERAL["spec_nolog_n5"], n_clusters=512),
}
LITE = [(n, d) for n in (2, 3, 4, 5) for d in (1, 3)]


def lite_cfg(nodes, d):
    """test_gpu_steady_line0.cut_cfg at 256 clusters, one launch per step, and the launch plan:
    300 P ticks in launches of 3 P (the elections settle), 40 P + 1, then one launch of
    1000 P + 3 ticks."""
    cfg, P = cut_cfg(nodes, d, C)
    cfg["ticks_per_launch"] = 65536
    return cfg, P, [3 * P] * 100 + [40 * P + 1, 1000 * P + 3]


def oracle(**cfg):
    r = helpers.oracle(**cfg)
    helpers.oracle_threads(r, helpers.cpu_threads())
    return r


def pair(cfg, T0):
    return hc.start(helpers.gpu, cfg, T0), hc.start(oracle, cfg, T0)


def same_counters(g, r):
    cg, cr = g.counters(), r.counters()
    assert cg == cr, {k: (cg[k], cr[k]) for k in cg if cg[k] != cr[k]}
    return cg


def end_of_run(g, r, cfg, base):
    """At TOP the run stands on the last tick a step may end at: one more is refused on both
    sides and changes nothing."""
    if base == "top":
        hc.refused_at_the_end(g, cfg)
        hc.refused_at_the_end(r, cfg)
        hc.same_digests(g, r, "after the refusal")
    g.close()
    r.close()


@pytest.mark.parametrize("base", hc.BASES)
@pytest.mark.parametrize("name", list(GENERAL))
def test_general_body(name, base):
    """Digests after every 1,500-tick chunk, every counter (first_violation_tick and payload_max
    among them) at the end."""
    cfg = GENERAL[name]
    g, r = pair(cfg, hc.base_tick(base, cfg, TICKS))
    hc.run_pair(g, r, CHUNKS)
    c = same_counters(g, r)
    assert c["node_ticks"] == cfg["n_clusters"] * cfg["nodes"] * TICKS
    end_of_run(g, r, cfg, base)


@pytest.mark.parametrize("base", hc.BASES)
@pytest.mark.parametrize("name", list(TRACED))
def test_traced(name, base):
    """With the trace rings on: digests, counters, and for 8 clusters every recorded event (its
    absolute tick among the fields) and the printed dump."""
    cfg = TRACED[name]
    T0 = hc.base_tick(base, cfg, TICKS)
    g, r = pair(cfg, T0)
    hc.run_pair(g, r, CHUNKS)
    same_counters(g, r)
    events = 0
    for c in range(8):
        for i in range(1, cfg["nodes"] + 1):
            tg = g.trace(c, i)
            assert tg == r.trace(c, i), (c, i)
            assert all(T0 <= e["tick"] < T0 + TICKS for e in tg), (c, i)
            assert g.edn_trace(c, i) == r.edn_trace(c, i), (c, i)
            events += len(tg)
    assert events >= 4 * cfg["nodes"] * cfg["trace_cap"]          # most rings are full
    end_of_run(g, r, cfg, base)


@pytest.mark.parametrize("base", hc.BASES)
@pytest.mark.parametrize("mode", ["always", None, "never"])
@pytest.mark.parametrize("nodes,d", LITE)
def test_lite_launches(nodes, d, mode, base, monkeypatch):
    """The steady kernel (always), auto mode and the general body's LITE instance (never) from a
    fresh handle moved to T0, all timers overdue together: digests, counters and every node
    record after each launch. The bases are sized to the whole plan, so at SIGN the long launch
    holds 2^31 among its whole rounds."""
    if mode is None:
        monkeypatch.delenv("RAFTSIM_STEADY", raising=False)
    else:
        monkeypatch.setenv("RAFTSIM_STEADY", mode)
    cfg, P, plan = lite_cfg(nodes, d)
    T0 = hc.base_tick(base, cfg, sum(plan))
    g, r = pair(cfg, T0)
    for i, n in enumerate(plan):
        assert n <= 65536
        both(g, r, n, f"launch {i} of {n} ticks")
    if mode == "always":
        assert g.diag_last_bails() >= 0, "the long launch did not take the steady kernel"
    if mode == "never":
        assert g.diag_last_bails() == -1
    if base in ("sign0", "sign7"):
        assert r.tick - plan[-1] < 2 ** 31 < r.tick
    end_of_run(g, r, cfg, base)


def windows(top):
    """[t_lo, t_hi) of the violation queries; `top` is the latest first_tick of any record."""
    return [(0, 2 ** 31), (2 ** 31, 2 ** 32 - 1), (0, 2 ** 32), (0, 2 ** 64 - 1),
            (2 ** 31, 2 ** 64 - 1), (top + 1, 2 ** 64 - 1), (2 ** 32 - 1, 2 ** 64 - 1),
            (2 ** 32, 2 ** 64 - 1)]


@pytest.mark.parametrize("base", hc.BASES)
@pytest.mark.parametrize("name", list(QUERIES))
def test_queries_and_packs(name, base, tmp_path):
    """Violation records, their windows and clear(); census, audit, gather and fork at the end of
    the run; the fork and its source then go on for 3 x 500 ticks (at TOP to the last tick a
    step may end at)."""
    cfg = QUERIES[name]
    n = cfg["n_clusters"]
    extra = [500] * 3
    T0 = (hc.TOP(cfg, TICKS + sum(extra)) if base == "top" else hc.base_tick(base, cfg, TICKS))
    setup = hc.setup_for(cfg, T0)
    points = tuple(T0 + LAUNCH * k for k in (1, 2, 3))
    want = expected_records(cfg, n, points, tick0=T0, setup=setup)
    g, r = pair(cfg, T0)
    for t, exp in zip(points, want):
        hc.run_pair(g, r, [t - g.tick])
        recs = as_records(exp)
        assert g.violations() == (len(recs), recs), t
        first = min((x["first_tick"] for x in recs), default=None)
        assert g.counters()["first_violation_tick"] == first, t
    assert len(recs) >= 8                                  # the lists compared are not empty
    for lo, hi in windows(max(x["first_tick"] for x in recs)):
        sub = [x for x in recs if lo <= x["first_tick"] < hi]
        assert g.violations(t_lo=lo, t_hi=hi) == (len(sub), sub), (lo, hi)
    # clear() (at SIGN above 2^31), then the records of the rest of the run alone
    t_clear, t_end = points[-1], T0 + TICKS
    before = g.digest(), g.counters()
    g.clear_violations()
    assert g.violations() == (0, [])
    assert np.array_equal(g.digest(), before[0]) and g.counters() == before[1]
    hc.run_pair(g, r, [t_end - t_clear])
    win = expected_window(cfg, n, t_clear, t_end, step=100, tick0=T0, setup=setup)
    total, recs = g.violations()
    assert total == len(win) and [x["cluster"] for x in recs] == sorted(win)
    for x in recs:
        (lo, hi), counts = win[x["cluster"]]
        assert tuple(x[k] for k in KINDS) == counts, x
        assert lo <= x["first_tick"] < hi, (x, lo, hi)
    same_counters(g, r)
    # census and audit of the state as it stands
    census, crecs = census_oracle.of_backend(r)
    assert g.census() == census
    every = tuple(census_oracle.CLASSES)
    assert g.select(any=every) == census_oracle.select_of(crecs, any=every)
    assert g.select(any=("halted", "multi_leader"), none=("settled",)) == \
        census_oracle.select_of(crecs, any=("halted", "multi_leader"), none=("settled",))
    summary, arecs = audit_oracle.of_backend(r)
    assert g.audit() == summary
    every = tuple(audit_oracle.CLASSES)
    assert g.audit_select(any=every) == audit_oracle.select_of(arecs, any=every)
    assert g.audit_select(any=("diverged",)) == audit_oracle.select_of(arecs, any=("diverged",))
    # packs: the device's bytes against the mirror of the handle's and of the oracle's reads
    ids = [0, 31, 63, n - 1, 101]
    pack = g.gather(ids)
    assert pack.tick == g.tick == t_end and pack.clusters == ids
    assert np.array_equal(pack.data, gm.pack_of(g, ids).data)
    assert np.array_equal(pack.data, gm.pack_bytes(r, ids))
    loaded = ClusterPack.load(pack.save(tmp_path / "pack"))
    assert type(loaded.tick) is int and loaded.tick == t_end
    assert np.array_equal(loaded.data, pack.data)
    f = raftsim.fork(loaded, 1, trace_cap=0, trace_entry_cap=0)
    assert f.tick == t_end and f.config.cluster_offset == 31
    assert f.digest()[0] == g.digest(31, 1)[0] == r.digest(31, 1)[0]
    for k in extra:
        f.step(k)
        hc.run_pair(g, r, [k])
        assert f.tick == g.tick
        assert f.digest()[0] == g.digest(31, 1)[0] == r.digest(31, 1)[0]
    # replay reruns from init-node: a moved handle is refused (no defect)
    with pytest.raises(helpers.RaftSimError, match="written by the host"):
        raftsim.replay(g, 31)
    if base == "top":
        hc.refused_at_the_end(f, cfg)
    f.close()
    end_of_run(g, r, cfg, base)


@pytest.mark.parametrize("base", hc.BASES)
def test_gather_after_steady_launches(base, monkeypatch):
    """A handle that has just taken steady launches: the followers' deadlines are owed timer
    draws (last event + el_base + draw), which the gather resolves at ticks above 2^31 and next
    to the horizon; the pack equals the mirror of the handle's reads and of the oracle's."""
    monkeypatch.setenv("RAFTSIM_STEADY", "always")
    cfg, P, _ = lite_cfg(5, 2)
    plan = [3 * P] * 100 + [40 * P + 1, 17 * P + 5]
    g, r = pair(cfg, hc.base_tick(base, cfg, sum(plan)))
    hc.run_pair(g, r, plan)
    assert g.diag_last_bails() >= 0
    ids = [0, 31, 63, 255, 101]
    pack = g.gather(ids)
    assert pack.tick == r.tick
    assert np.array_equal(pack.data, gm.pack_of(g, ids).data)
    assert np.array_equal(pack.data, gm.pack_bytes(r, ids))
    dl = [nd.deadline for i in range(len(ids)) for nd in pack.nodes[i]]
    assert all(r.tick <= x <= r.tick + hc.longest(cfg) for x in dl)
    hc.same_digests(g, r, "after the gather")
    end_of_run(g, r, cfg, base)


@pytest.mark.parametrize("base", ["sign0", "sign7"])
def test_three_shards_equal_one(base):
    """n_devices = 3 across 2^31 equals the one-shard handle and the oracle: digests, counters,
    violations()."""
    cfg = CLIENTS_N5
    T0 = hc.base_tick(base, cfg, TICKS)
    one, r = pair(cfg, T0)
    three = hc.start(helpers.gpu, dict(cfg, n_devices=3), T0)
    for n in CHUNKS:
        three.step(n)
    hc.run_pair(one, r, CHUNKS)
    hc.same_digests(three, r, "three shards")
    assert three.counters() == one.counters() == r.counters()
    total, recs = one.violations()
    assert total > 0 and three.violations() == (total, recs)
    assert min(x["first_tick"] for x in recs) == one.counters()["first_violation_tick"]
    for h in (one, three, r):
        h.close()
