"""What Simulator.audit() and Simulator.audit_select() must return, from any Backend's read_nodes
and log (test infrastructure).

Written from SIM_SPEC.md ("Derived, not state: the log audit"), not from the kernel: per pair of
nodes the first differing position, then the class bits read off those. Run on the oracle it is the
independent reference (the oracle's records and logs are bit-exact with the GPU's: the parity
suite); run on a GPU handle's own read-back it checks host-written logs no run reaches.
"""
from __future__ import annotations

from class_predicate import matches

CLASSES = {"diverged": 1, "commit_diverged": 2, "match_broken": 4, "term_order": 8,
           "identical": 16}
SCALARS = ("entries", "agree_sum", "agree_min", "agree_max", "diverged_nodes",
           "commit_diverged_nodes", "diverge_index_min", "commit_diverge_index_min")


def cluster_audit(logs, commits):
    """The record's fields of one cluster from its N logs ([(term, val)] each, node id 1 first)
    and its N commit indices. An index field that names no position is None."""
    n = len(logs)
    cls = 0
    agree = min(len(x) for x in logs)
    div_idx = cdiv_idx = order_idx = None
    div_nodes, cdiv_nodes = set(), set()
    for i in range(n):
        for j in range(i + 1, n):
            a, b = logs[i], logs[j]
            m = min(len(a), len(b))
            d = next((p for p in range(m) if a[p] != b[p]), m)
            agree = min(agree, d)
            if d == m:
                continue
            cls |= 1
            div_nodes |= {i + 1, j + 1}
            div_idx = d if div_idx is None else min(div_idx, d)
            if d < min(commits[i], commits[j]):
                cls |= 2
                cdiv_nodes |= {i + 1, j + 1}
                cdiv_idx = d if cdiv_idx is None else min(cdiv_idx, d)
            if any(a[p][0] == b[p][0] for p in range(d, m)):
                cls |= 4
    for log in logs:
        for p in range(len(log) - 1):
            if log[p][0] > log[p + 1][0]:
                cls |= 8
                order_idx = p if order_idx is None else min(order_idx, p)
                break
    if not cls & 1 and len({len(x) for x in logs}) == 1:
        cls |= 16
    return {"classes": tuple(k for k, b in CLASSES.items() if cls & b), "agree_len": agree,
            "diverge_index": div_idx, "commit_diverge_index": cdiv_idx, "order_index": order_idx,
            "diverged": sorted(div_nodes), "commit_diverged": sorted(cdiv_nodes),
            "len_min": min(len(x) for x in logs)}


def records_of(logs, commits, n_nodes, cluster_offset=0):
    """Every cluster's record, in the form Simulator.audit_select returns them, from flat lists of
    logs and commit indices (n_nodes per cluster)."""
    recs = []
    for c in range(len(logs) // n_nodes):
        rec = {"cluster": c, "global_id": cluster_offset + c}
        rec.update(cluster_audit(logs[c * n_nodes:(c + 1) * n_nodes],
                                 commits[c * n_nodes:(c + 1) * n_nodes]))
        recs.append(rec)
    return recs


def summary_of(recs, logs):
    """The summary, in the form Simulator.audit returns it, from records_of's list and the logs."""
    div = [r["diverge_index"] for r in recs if r["diverge_index"] is not None]
    cdiv = [r["commit_diverge_index"] for r in recs if r["commit_diverge_index"] is not None]
    agree = [r["agree_len"] for r in recs]
    return {"clusters": len(recs),
            "by_class": {k: sum(k in r["classes"] for r in recs) for k in CLASSES},
            "entries": sum(len(x) for x in logs), "agree_sum": sum(agree),
            "agree_min": min(agree), "agree_max": max(agree),
            "diverged_nodes": sum(len(r["diverged"]) for r in recs),
            "commit_diverged_nodes": sum(len(r["commit_diverged"]) for r in recs),
            "diverge_index_min": min(div) if div else None,
            "commit_diverge_index_min": min(cdiv) if cdiv else None}


def select_of(recs, any=(), all=(), none=(), limit=None):
    """(total, records) as Simulator.audit_select returns them, from records_of's list."""
    hit = [r for r in recs if matches(r, any, all, none)]
    return len(hit), hit if limit is None else hit[:limit]


def of_backend(be):
    """(summary, records) of a Backend (the oracle, or a GPU handle through its read-back). The
    node records are read once; a log is read only where log_len says there is one."""
    nodes = be.read_nodes()
    logs = [be.log(i // be.N, i % be.N + 1) if r["log_len"] else [] for i, r in enumerate(nodes)]
    assert [len(x) for x in logs] == [r["log_len"] for r in nodes]
    recs = records_of(logs, [r["commit_index"] for r in nodes], be.N, be.config.cluster_offset)
    return summary_of(recs, logs), recs


_cache = {}


def oracle_at(cfg, ticks):
    """[(summary, records)] of an oracle run of cfg from init-node, one per checkpoint of the
    increasing tuple `ticks`. Computed once per argument set and shared between the tests."""
    import pairing

    key = (tuple(sorted(cfg.items())), tuple(ticks))
    if key not in _cache:
        out = []
        with pairing.oracle(cfg) as h:
            for t in ticks:
                h.step(t - h.tick)
                out.append(of_backend(h))
        _cache[key] = out
    return _cache[key]


def population(summary):
    """by_class in the table's column order."""
    return [summary["by_class"][k] for k in CLASSES]
