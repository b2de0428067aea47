"""Per-cluster violation records on the GPU: Simulator.violations (the device-side compaction over
the records the checker keeps), clear_violations, raftsim.replay and dist.locate_first_violation,
held to the oracle's per-cluster values (tests/viol_oracle.py: one-cluster oracle handles, a
method tests/test_violations_abi.py checks on the oracle alone).

Figures measured on the oracle for the cases below (all asserted through expected_records):
burst_variant_mid_n8 at 96 clusters, 20,000 ticks: 67 violating clusters, 42 / 485 / 10 violations,
first tick 295; fast_timers: 37 clusters, first tick 150; spec_nolog: 81 clusters, leader
completeness only, first tick 1225; spec_c3: none; arena_odd at 4,133 clusters, 3,000 ticks: 3,237
clusters, 69 / 36,531 / 76, first tick 75; c5_variant at 3,001 clusters, 9,000 ticks: 39 clusters
(18 / 14 / 7 over three shards), 23 of the 47 groups of 64 clusters empty, first tick 5327."""
import ctypes

import numpy as np
import pytest

import helpers
import pairing
import raftsim
from cases import CASES
from raftsim import dist
from viol_oracle import KINDS, as_records, expected_records, expected_window

pytestmark = pytest.mark.gpu

STEPS = (5000, 10000, 15000, 20000)
SMALL = ("burst_variant_mid_n8", "fast_timers", "spec_nolog", "spec_c3")


def small_cfg(name):
    return dict(CASES[name], n_clusters=96)


@pytest.fixture(scope="module")
def small_runs():
    """Each SMALL case run once on the GPU: after every 5,000-tick step the full violations()
    answer and the counters; after the run the digests. The handles stay open (replay)."""
    runs = {}
    for name in SMALL:
        g = helpers.gpu(**small_cfg(name))
        seen = []
        for t in STEPS:
            g.step(t - g.tick)
            seen.append((g.violations(), g.counters()))
        runs[name] = dict(sim=g, seen=seen, digest=g.digest())
    yield runs
    for r in runs.values():
        r["sim"].close()


@pytest.mark.parametrize("name", SMALL)
def test_records_equal_the_oracles(small_runs, name):
    """The three kinds, the burst engine's compare included (N = 8), the faithful N = 5 kernel,
    Spec-Raft without the vote check (leader completeness only) and the zero-violation control."""
    want = expected_records(small_cfg(name), 96, STEPS)
    assert (name == "spec_c3") == (not want[-1])
    for t, exp, ((total, recs), _) in zip(STEPS, want, small_runs[name]["seen"]):
        assert total == len(exp), (name, t)
        assert recs == as_records(exp), (name, t)
    if name == "spec_c3":
        assert small_runs[name]["seen"][-1][0] == (0, [])


@pytest.mark.parametrize("name", SMALL)
def test_sums_and_minimum_are_the_counters(small_runs, name):
    for t, ((_, recs), ctr) in zip(STEPS, small_runs[name]["seen"]):
        for k in KINDS:
            assert sum(r[k] for r in recs) == ctr["viol_" + k], (name, t, k)
        first = min((r["first_tick"] for r in recs), default=None)
        assert first == ctr["first_violation_tick"], (name, t)


@pytest.mark.parametrize("name", ["burst_variant_mid_n8", "fast_timers"])
def test_state_is_untouched(small_runs, name):
    """No record write lands in state: every cluster's digest is the oracle's after the run."""
    r = pairing.oracle(small_cfg(name))
    r.step(STEPS[-1])
    assert np.array_equal(small_runs[name]["digest"], r.digest())
    assert small_runs[name]["seen"][-1][1] == r.counters()


def test_compaction_dense():
    """4,133 clusters (no multiple of the wave, the workgroup or its chunk; three workgroups), most
    of them violating: the full list, a limit below the total, the count alone, kind masks and a
    first-tick window."""
    cfg = dict(CASES["arena_odd"], n_clusters=4133)
    exp = expected_records(cfg, 4133, 3000)
    want = as_records(exp)
    g = helpers.gpu(**cfg)
    g.step(3000)
    assert len(want) == 3237
    assert g.violations() == (len(want), want)
    assert g.violations(limit=100) == (len(want), want[:100])
    assert g.violations(limit=0) == (len(want), [])
    assert g.violations(limit=5000) == (len(want), want)            # a capacity above the total
    for kind in KINDS:
        sub = [r for r in want if r[kind]]
        assert sub and len(sub) < len(want)
        assert g.violations(kinds=(kind,)) == (len(sub), sub), kind
    two = [r for r in want if r["election"] or r["complete"]]
    assert g.violations(kinds=("election", "complete")) == (len(two), two)
    firsts = sorted(r["first_tick"] for r in want)
    med = firsts[len(firsts) // 2]
    early = [r for r in want if r["first_tick"] < med]
    late = [r for r in want if r["first_tick"] >= med]
    assert early and late
    assert g.violations(t_hi=med) == (len(early), early)
    assert g.violations(t_lo=med) == (len(late), late)
    mid = [r for r in want if firsts[len(firsts) // 4] <= r["first_tick"] < med]
    assert g.violations(t_lo=firsts[len(firsts) // 4], t_hi=med, limit=7) == (len(mid), mid[:7])
    assert g.violations(t_lo=med, t_hi=med) == (0, [])               # an empty window
    c = g.counters()
    assert [sum(r[k] for r in want) for k in KINDS] == [c["viol_" + k] for k in KINDS]
    g.close()


def test_compaction_sparse_and_shards():
    """3,001 clusters of which 39 violate, half of the 64-cluster groups empty: one shard against
    three on the same device (their lists concatenate in shard order, rebased to the handle), and
    locate_first_violation after the search."""
    cfg = dict(CASES["c5_variant"], n_clusters=3001)
    exp = expected_records(cfg, 3001, 9000)
    want = as_records(exp)
    lo = [3001 * d // 3 for d in range(4)]
    per_shard = [sum(lo[d] <= c < lo[d + 1] for c in exp) for d in range(3)]
    fv = min(r["first_tick"] for r in want)
    empty = 47 - len({c // 64 for c in exp})         # whole waves without a match
    assert (len(want), per_shard, empty, fv) == (39, [18, 14, 7], 23, 5327)
    at_fv = [r["global_id"] for r in want if r["first_tick"] == fv]
    for nd in (1, 3):
        g = helpers.gpu(n_devices=nd, **cfg)
        tick, stepped, _ = dist.first_violation_search(g, 3000, 9000)
        assert (tick, stepped) == (fv, 6000)
        assert dist.locate_first_violation(g) == (fv, at_fv), nd
        g.step(9000 - g.tick)
        assert g.violations() == (len(want), want), nd
        assert g.violations(limit=per_shard[0] + 1) == (len(want), want[:per_shard[0] + 1]), nd
        assert g.violations(limit=0) == (len(want), []), nd
        assert dist.locate_first_violation(g) == (fv, at_fv), nd
        # a rank whose own minimum is later than the job's returns no cluster
        assert dist.locate_first_violation(g, lambda x: min(x, fv - 1)) == (fv - 1, [])
        g.close()
    # the same job's clusters 1000.. as a handle of their own (a rank's range): the same records
    # with the cluster index rebased and the global ids unchanged
    part = [dict(r, cluster=r["cluster"] - 1000) for r in want if r["cluster"] >= 1000]
    g = helpers.gpu(**dict(cfg, n_clusters=2001, cluster_offset=1000, n_devices=2))
    g.step(9000)
    assert part and g.violations() == (len(part), part)
    g.close()
    none = helpers.gpu(**dict(CASES["spec_c3"], n_clusters=96))
    none.step(2000)
    assert dist.locate_first_violation(none) == (None, [])
    none.close()


def test_records_do_not_depend_on_packing_or_launch_length(small_runs):
    """Clusters move between waves under RAFT_SCHED_ALIGNED and a launch boundary splits the run
    elsewhere with ticks_per_launch=37: the records are the same. A query enqueued behind
    step_async waits for the steps."""
    cfg = small_cfg("fast_timers")
    want = as_records(expected_records(cfg, 96, STEPS)[-1])
    assert small_runs["fast_timers"]["seen"][-1][0] == (len(want), want)    # aligned, default
    for extra in (dict(schedule=1), dict(ticks_per_launch=37), dict(schedule=1, ticks_per_launch=37)):
        g = helpers.gpu(**cfg, **extra)
        g.step_async(STEPS[-1])
        assert g.violations() == (len(want), want), extra
        g.sync()
        assert g.violations() == (len(want), want), extra
        g.close()


def test_clear_and_persistence():
    cfg = small_cfg("fast_timers")
    t0, t1 = 2500, 20000
    g = helpers.gpu(**cfg)
    g.step(t0)
    before = expected_records(cfg, 96, t0)
    assert before and g.violations() == (len(before), as_records(before))
    # host writes of state leave the records alone: a cluster's own records, read and rewritten
    c = sorted(before)[0]
    dig, ctr = g.digest(), g.counters()
    g.write_nodes(c, list(g.read_nodes_raw(c, 1)))
    g.write_clusters(c, g.read_clusters(c, 1))
    assert g.violations() == (len(before), as_records(before))
    assert np.array_equal(g.digest(), dig)
    # clear: an empty list; state and counters as they were
    g.clear_violations()
    assert g.violations() == (0, [])
    assert np.array_equal(g.digest(), dig) and g.counters() == ctr
    # from here on the records are those of the later ticks alone
    g.step(t1 - t0)
    win = expected_window(cfg, 96, t0, t1, step=100)
    assert len(win) >= 3
    total, recs = g.violations()
    assert total == len(win) and [r["cluster"] for r in recs] == sorted(win)
    for r in recs:
        (lo, hi), counts = win[r["cluster"]]
        assert tuple(r[k] for k in KINDS) == counts, r
        assert lo <= r["first_tick"] < hi, (r, lo, hi)
    after = g.counters()
    whole = expected_records(cfg, 96, t1)
    for i, k in enumerate(KINDS):                      # the counters were not cleared
        assert after["viol_" + k] == sum(v[1][i] for v in whole.values())
    g.close()


def test_replay(small_runs):
    """search -> violating cluster -> the cluster alone with its `wait` trace."""
    src = small_runs["fast_timers"]["sim"]
    cfg = small_cfg("fast_timers")
    total, recs = src.violations()
    first = min(recs, key=lambda r: (r["first_tick"], r["cluster"]))
    assert first["first_tick"] == src.counters()["first_violation_tick"]
    one = raftsim.replay(src, first["cluster"])
    assert one.tick == src.tick == STEPS[-1] and one.C == 1
    assert one.config.cluster_offset == first["global_id"] and one.config.trace_cap > 0
    ctr = one.counters()
    assert tuple(ctr["viol_" + k] for k in KINDS) == tuple(first[k] for k in KINDS)
    assert ctr["first_violation_tick"] == first["first_tick"]
    assert one.violations() == (1, [dict(first, cluster=0)])
    ref = helpers.oracle(**src.replay_config(first["cluster"]))
    ref.step(STEPS[-1])
    assert np.array_equal(one.digest(), ref.digest())
    assert ref.counters() == ctr
    txt = one.edn_trace(0, 1)
    assert txt and txt == ref.edn_trace(0, 1)
    # stepping the replay to an earlier tick stops before the violation is counted
    early = raftsim.replay(src, first["cluster"], ticks=first["first_tick"])
    assert early.tick == first["first_tick"] and early.violations() == (0, [])
    early.step(1)
    assert early.violations()[1][0]["first_tick"] == first["first_tick"]
    for h in (one, ref, early):
        h.close()
    # only a run from init-node is reproducible from its config
    moved = helpers.gpu(**dict(cfg, n_clusters=4))
    moved.step(100)
    moved.set_tick(100)
    with pytest.raises(raftsim.RaftSimError, match="init-node"):
        raftsim.replay(moved, 0)
    moved.close()


def test_bad_arguments():
    g = helpers.gpu(**dict(CASES["fast_timers"], n_clusters=4))
    read = g._viol["read"]
    buf = (raftsim._abi.Violation * 4)()
    for mask, lo, hi, out, cap in ((0, 0, 1, buf, 4), (8, 0, 1, buf, 4), (7, 2, 1, buf, 4),
                                   (7, 0, 1, None, 4)):
        assert read(g._h, mask, lo, hi, out, cap) == -22, (mask, lo, hi, cap)
        assert g._fns["last_error"]()
    assert read(g._h, 7, 0, 2 ** 64 - 1, None, 0) == 0
    assert read(g._h, 7, 5, 5, buf, 4) == 0
    with pytest.raises(ValueError):
        g.violations(kinds=("safety",))
    with pytest.raises(raftsim.RaftSimError):
        g.violations(kinds=())
    assert ctypes.sizeof(buf) == 96
    g.close()
