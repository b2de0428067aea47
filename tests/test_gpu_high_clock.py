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
import pairing
import raftsim
from cases import CLIENTS_N5, GENERAL, LITE, QUERIES, TRACED, lite_cfg
from cases import HC_CHUNKS as CHUNKS, HC_LAUNCH as LAUNCH, HC_TICKS as TICKS
from raftsim import ClusterPack
from steady_pair import step
from viol_oracle import KINDS, as_records, expected_records, expected_window

pytestmark = pytest.mark.gpu


def end_of_run(g, r, cfg, base):
    """At TOP the run stands on the last tick a step may end at: one more is refused on both
    sides and changes nothing."""
    if base == "top":
        hc.refused_at_the_end(g, cfg)
        hc.refused_at_the_end(r, cfg)
        pairing.same(g, r, "after the refusal")


@pytest.mark.parametrize("base", hc.BASES)
@pytest.mark.parametrize("name", list(GENERAL))
def test_general_body(name, base):
    """Digests after every 1,500-tick chunk, every counter (first_violation_tick and payload_max
    among them) at the end."""
    cfg = GENERAL[name]
    with hc.pair(cfg, hc.base_tick(base, cfg, TICKS)) as (g, r):
        pairing.run(g, r, CHUNKS)
        c = pairing.same_counters(g, r)
        assert c["node_ticks"] == cfg["n_clusters"] * cfg["nodes"] * TICKS
        end_of_run(g, r, cfg, base)


@pytest.mark.parametrize("base", hc.BASES)
@pytest.mark.parametrize("name", list(TRACED))
def test_traced(name, base):
    """With the trace rings on: digests, counters, and for 8 clusters every recorded event (its
    absolute tick among the fields) and the printed dump."""
    cfg = TRACED[name]
    T0 = hc.base_tick(base, cfg, TICKS)
    with hc.pair(cfg, T0) as (g, r):
        pairing.run(g, r, CHUNKS)
        pairing.same_counters(g, r)
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
    with hc.pair(cfg, T0) as (g, r):
        for i, n in enumerate(plan):
            assert n <= 65536
            step(g, r, n, f"launch {i} of {n} ticks")
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
    with hc.pair(cfg, T0) as (g, r):
        for t, exp in zip(points, want):
            pairing.run(g, r, [t - g.tick])
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
        pairing.run(g, r, [t_end - t_clear])
        win = expected_window(cfg, n, t_clear, t_end, step=100, tick0=T0, setup=setup)
        total, recs = g.violations()
        assert total == len(win) and [x["cluster"] for x in recs] == sorted(win)
        for x in recs:
            (lo, hi), counts = win[x["cluster"]]
            assert tuple(x[k] for k in KINDS) == counts, x
            assert lo <= x["first_tick"] < hi, (x, lo, hi)
        pairing.same_counters(g, r)
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
            pairing.run(g, r, [k])
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
    with hc.pair(cfg, hc.base_tick(base, cfg, sum(plan))) as (g, r):
        pairing.run(g, r, plan)
        assert g.diag_last_bails() >= 0
        ids = [0, 31, 63, 255, 101]
        pack = g.gather(ids)
        assert pack.tick == r.tick
        assert np.array_equal(pack.data, gm.pack_of(g, ids).data)
        assert np.array_equal(pack.data, gm.pack_bytes(r, ids))
        dl = [nd.deadline for i in range(len(ids)) for nd in pack.nodes[i]]
        assert all(r.tick <= x <= r.tick + hc.longest(cfg) for x in dl)
        pairing.same(g, r, "after the gather")
        end_of_run(g, r, cfg, base)


@pytest.mark.parametrize("base", ["sign0", "sign7"])
def test_three_shards_equal_one(base):
    """n_devices = 3 across 2^31 equals the one-shard handle and the oracle: digests, counters,
    violations()."""
    cfg = CLIENTS_N5
    T0 = hc.base_tick(base, cfg, TICKS)
    with hc.pair(cfg, T0) as (one, r):
        with hc.start(helpers.gpu, dict(cfg, n_devices=3), T0) as three:
            for n in CHUNKS:
                three.step(n)
            pairing.run(one, r, CHUNKS)
            pairing.same(three, r, "three shards")
            assert three.counters() == one.counters() == r.counters()
            total, recs = one.violations()
            assert total > 0 and three.violations() == (total, recs)
            assert min(x["first_tick"] for x in recs) == one.counters()["first_violation_tick"]
