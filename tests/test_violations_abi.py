"""Violation records without a GPU: the ABI extension (raft_viol_*: layout, exported symbols, the
Clojure facade's view), the arithmetic of replay_config, and the method tests/test_gpu_violations.py
rests on, checked on the oracle alone: one-cluster oracle handles give per-cluster records whose
sums are the whole handle's counters."""
import ctypes
import re

import pytest

import helpers
import hostprog
import pairing
import raftsim
import viol_oracle
from cases import CASES, GENERAL
from hostprog import HEADER, ROOT
from raftsim import _abi, _backend

CLJ = (ROOT / "clojure" / "src" / "raft" / "sim.clj").read_text()


def test_violation_layout_matches_the_c_compiler(tmp_path):
    out = hostprog.c_layout(tmp_path, {"raft_violation_t": _abi.Violation}, [
        'printf("kinds %d %d %d\\n", RAFT_VIOL_ELECTION, RAFT_VIOL_LOG, RAFT_VIOL_COMPLETE);'])
    assert ctypes.sizeof(_abi.Violation) == 24
    assert out[-1].split()[1:] == [str(_abi.VIOL_KINDS[k]) for k in viol_oracle.KINDS]
    # the per-kind counts follow the counter enum's order (the kernel indexes them by it)
    i = _abi.COUNTER_NAMES.index("viol_election")
    assert _abi.COUNTER_NAMES[i:i + 3] == ["viol_" + k for k in viol_oracle.KINDS]


def test_library_exports_the_violation_entry_points():
    assert hostprog.exported(r"raft_viol_\w+") == set(_abi.VIOL_SYMBOLS) == \
        {"raft_viol_read", "raft_viol_clear"}
    lib = ctypes.CDLL(str(raftsim.LIB_PATH))        # loads without a GPU
    fns = _abi.bind(lib, "raft_viol_", sigs=_abi._VIOL_SIGS)
    assert set(fns) == {"read", "clear"}
    # bad arguments are refused before any device is touched, with a message
    last_error = _abi.bind(lib, "raft_sim_")["last_error"]
    assert fns["read"](None, 7, 0, 1, None, 0) == -22 and b"null" in last_error()
    assert fns["clear"](None) == -22


def test_header_declares_both_symbol_sets():
    """The raft_sim_* functions are still exactly the table the oracle mirrors; the raft_viol_*
    ones exactly the second table, which is bound for the product library only."""
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"\b(raft_sim_\w+)\s*\(", text))) == sorted(_abi.PRODUCT_SYMBOLS)
    assert _abi.PRODUCT_SYMBOLS == ["raft_sim_" + n for n in _abi._SIGS]
    assert sorted(set(re.findall(r"\b(raft_viol_\w+)\s*\(", text))) == sorted(_abi.VIOL_SYMBOLS)
    assert "#define RAFT_SIM_ABI_VERSION 2" in text
    # the oracle Backend still loads: it binds the first table only
    with helpers.oracle(n_clusters=1) as h:
        assert not hasattr(h, "violations") and not h.host_written


def test_clojure_facade_names_the_entry_points():
    assert int(re.search(r"\(def violation-size (\d+)\)", CLJ).group(1)) == \
        ctypes.sizeof(_abi.Violation)
    assert set(re.findall(r'"(raft_viol_\w+)"', CLJ)) == set(_abi.VIOL_SYMBOLS)
    for name in ("(defn violations", "(defn clear-violations!"):
        assert name in CLJ, name
    offs = [getattr(_abi.Violation, f).offset for f in ("first_tick", "count", "kinds")]
    assert offs == [4, 8, 20]
    for off in (4, 8, 12, 16, 20):
        assert f"(.getInt m (+ b {off}))" in CLJ, off


def test_replay_config_arithmetic():
    cfg = _abi.Config()
    for f, _ in _abi.Config._fields_:
        setattr(cfg, f, 3)
    cfg.n_clusters, cfg.cluster_offset, cfg.n_devices, cfg.seed = 3001, 70000, 3, 2 ** 40 + 5
    cfg.ticks_per_launch, cfg.trace_cap, cfg.trace_entry_cap = 37, 0, 0
    one = _backend.replay_config(cfg, 2999)
    assert set(one) == {f for f, _ in _abi.Config._fields_}
    assert (one["n_clusters"], one["cluster_offset"], one["n_devices"]) == (1, 72999, 1)
    assert one["trace_cap"] > 0 and one["trace_entry_cap"] > 0        # the trace rings are on
    same = set(one) - {"n_clusters", "cluster_offset", "n_devices", "trace_cap", "trace_entry_cap"}
    assert all(one[f] == getattr(cfg, f) for f in same)
    assert one["seed"] == 2 ** 40 + 5 and one["ticks_per_launch"] == 37
    over = _backend.replay_config(cfg, 0, trace_cap=7, trace_entry_cap=0, commit_stream_cap=9)
    assert (over["trace_cap"], over["trace_entry_cap"], over["commit_stream_cap"]) == (7, 0, 9)
    assert over["cluster_offset"] == 70000
    for bad in (-1, 3001):
        with pytest.raises(ValueError):
            _backend.replay_config(cfg, bad)
    with pytest.raises(TypeError):
        _backend.replay_config(cfg, 0, no_such_field=1)
    # the config an oracle handle is built from round-trips
    base = dict(CASES["fast_timers"], n_clusters=8, cluster_offset=100)
    with helpers.oracle(**base) as h:
        one = _backend.replay_config(h.config, 5, trace_cap=0, trace_entry_cap=0)
    assert one == dict({f: getattr(h.config, f) for f, _ in _abi.Config._fields_},
                       n_clusters=1, cluster_offset=105, n_devices=1)


def test_host_writes_are_remembered():
    """raftsim.replay refuses a handle whose state or clock the host wrote: the flag it reads."""
    with helpers.oracle(n_clusters=2) as h:
        assert not h.host_written
        h.step(10)
        h.read_nodes()
        assert not h.host_written
        h.set_tick(20)
        assert h.host_written
    with helpers.oracle(n_clusters=2) as h:
        h.write_nodes(0, list(h.read_nodes_raw(0, 1)))
        assert h.host_written


def test_one_cluster_handles_sum_to_the_whole_handle():
    """The method, on the oracle alone: burst_variant_mid_n8 at 96 clusters and 20,000 ticks. The
    per-cluster counters of one-cluster handles sum to the whole handle's, their earliest first
    tick is its first_violation_tick, and every kind occurs, so the GPU tests that compare with
    these records cannot pass on empty lists. (Measured: election 42 in 38 clusters, log 485 in
    66, complete 10 in 8; 67 violating clusters; first tick 295.)"""
    cfg = dict(CASES["burst_variant_mid_n8"], n_clusters=96)
    steps = (5000, 10000, 15000, 20000)
    per_step = viol_oracle.expected_records(cfg, 96, steps)
    whole = pairing.oracle(cfg)
    for t, exp in zip(steps, per_step):
        whole.step(t - whole.tick)
        c = whole.counters()
        for i, k in enumerate(viol_oracle.KINDS):
            assert sum(counts[i] for _, counts in exp.values()) == c["viol_" + k], (t, k)
        assert min(first for first, _ in exp.values()) == c["first_violation_tick"], t
    exp = per_step[-1]
    for i, k in enumerate(viol_oracle.KINDS):
        assert sum(1 for _, counts in exp.values() if counts[i]) >= 1, k
    assert all(0 <= c < 96 and any(counts) for c, (_, counts) in exp.items())
    recs = viol_oracle.as_records(exp)
    assert [r["cluster"] for r in recs] == sorted(exp) and len(recs) == len(exp)


def test_one_cluster_handles_sum_to_the_whole_handle_across_2_31():
    """The same method from a moved clock (expected_records' tick0 and setup): the whole handle
    and the one-cluster handles are moved to 2^31 - 3000 and given their client cursors as
    high_clock.start does; the sums and the earliest first tick agree at three checkpoints, the
    last two at and above 2^31. (Measured at 96 clusters: election 18 / log 295 / complete 11 at
    the end, first tick 2147481308.)"""
    import high_clock as hc

    cfg = dict(GENERAL["variant1_n5"], n_clusters=96)
    T0 = hc.SIGN(6000)
    points = (T0 + 1500, T0 + 3000, T0 + 6000)
    per_step = viol_oracle.expected_records(cfg, 96, points, tick0=T0, setup=hc.setup_for(cfg, T0))
    whole = hc.start(helpers.oracle, cfg, T0)
    assert points[1] == 2 ** 31
    for t, exp in zip(points, per_step):
        whole.step(t - whole.tick)
        c = whole.counters()
        print(t, {k: c["viol_" + k] for k in viol_oracle.KINDS}, c["first_violation_tick"])
        for i, k in enumerate(viol_oracle.KINDS):
            assert sum(counts[i] for _, counts in exp.values()) == c["viol_" + k], (t, k)
        assert min(first for first, _ in exp.values()) == c["first_violation_tick"], t
        assert all(T0 <= first < t for first, _ in exp.values())
    for i, k in enumerate(viol_oracle.KINDS):
        assert sum(1 for _, counts in per_step[-1].values() if counts[i]) >= 1, k
    assert any(first >= 2 ** 31 for first, _ in per_step[-1].values())
