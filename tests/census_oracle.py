"""What Simulator.census() and Simulator.select() must return, from any Backend's read_nodes and
read_clusters (test infrastructure).

Written from the class table of SIM_SPEC.md ("Derived, not state: cluster classes"), not from the
kernel. Run on the oracle it is the independent reference: the oracle's records are bit-exact with
the GPU's (the parity suite), so the census of the oracle's records is the census the GPU owes.
"""
from __future__ import annotations

from class_predicate import matches

MAX_NODES = 9
CLASSES = {"no_leader": 1, "one_leader": 2, "multi_leader": 4, "halted": 8, "no_quorum": 16,
           "same_term_leaders": 32, "log_full": 64, "candidate": 128, "settled": 256}
LEADER, CANDIDATE = 2, 1
VARIANT_SPEC = 2
SCALARS = ("term_min", "term_max", "term_sum", "commit_max", "commit_sum", "len_max", "len_sum",
           "req_queued", "res_queued", "hwm_max", "hwm_sum")


def quorum(n_nodes, variant_flags):
    return n_nodes // 2 + 1 if variant_flags & VARIANT_SPEC else (n_nodes + 1) >> 1


def cluster_state(nodes, log_cap, variant_flags):
    """The class word and the record's fields of one cluster, from its N read_nodes() dicts."""
    n = len(nodes)
    live = [r for r in nodes if r["fault"] == 0]
    leaders = [(i + 1, r) for i, r in enumerate(nodes) if r["fault"] == 0 and r["role"] == LEADER]
    nl = len(leaders)
    cls = 1 if nl == 0 else 2 if nl == 1 else 4
    if len(live) < n:
        cls |= 8
    if len(live) < quorum(n, variant_flags):
        cls |= 16
    terms = [r["current_term"] for _, r in leaders]
    if len(set(terms)) < len(terms):
        cls |= 32
    if any(r["log_len"] == log_cap for r in nodes):
        cls |= 64
    if any(r["role"] == CANDIDATE for r in live):
        cls |= 128
    if nl == 1:
        lid, lr = leaders[0]
        if all(r["leader_id"] == lid and r["current_term"] == lr["current_term"] for r in live):
            cls |= 256
    return {
        "classes": tuple(k for k, b in CLASSES.items() if cls & b),
        "leaders": [i for i, _ in leaders],
        "halted": [i + 1 for i, r in enumerate(nodes) if r["fault"] != 0],
        "term_max": max(r["current_term"] for r in nodes),
        "term_min": min(r["current_term"] for r in nodes),
        "commit_max": max(r["commit_index"] for r in nodes),
        "len_max": max(r["log_len"] for r in nodes),
        "queued": sum(r["req_count"] + r["res_count"] for r in nodes),
    }


def records_of(nodes, n_nodes, log_cap, variant_flags, cluster_offset=0):
    """Every cluster's record, in the form Simulator.select returns them, from a flat read_nodes()
    list (n_nodes dicts per cluster)."""
    recs = []
    for c in range(len(nodes) // n_nodes):
        rec = {"cluster": c, "global_id": cluster_offset + c}
        rec.update(cluster_state(nodes[c * n_nodes:(c + 1) * n_nodes], log_cap, variant_flags))
        recs.append(rec)
    return recs


def census_of(nodes, clusters, n_nodes, log_cap, variant_flags):
    """The census, in the form Simulator.census returns it, from flat read_nodes() and
    read_clusters() lists."""
    recs = records_of(nodes, n_nodes, log_cap, variant_flags)
    live = [r for r in nodes if r["fault"] == 0]
    out = {"clusters": len(recs), "nodes": len(nodes),
           "by_class": {k: sum(k in r["classes"] for r in recs) for k in CLASSES},
           "leaders_hist": [sum(len(r["leaders"]) == i for r in recs) for i in range(n_nodes + 1)],
           "live_hist": [sum(n_nodes - len(r["halted"]) == i for r in recs)
                         for i in range(n_nodes + 1)],
           "role_nodes": [sum(r["role"] == i for r in live) for i in range(4)],
           "fault_nodes": [sum(r["fault"] == i for r in nodes) for i in range(5)]}
    terms = [r["current_term"] for r in nodes]
    commits = [r["commit_index"] for r in nodes]
    lens = [r["log_len"] for r in nodes]
    hwm = [c["hwm"][0] for c in clusters]
    out.update(term_min=min(terms), term_max=max(terms), term_sum=sum(terms),
               commit_max=max(commits), commit_sum=sum(commits), len_max=max(lens),
               len_sum=sum(lens), req_queued=sum(r["req_count"] for r in nodes),
               res_queued=sum(r["res_count"] for r in nodes), hwm_max=max(hwm), hwm_sum=sum(hwm))
    return out


def select_of(recs, any=(), all=(), none=(), limit=None):
    """(total, records) as Simulator.select returns them, from records_of's list."""
    hit = [r for r in recs if matches(r, any, all, none)]
    return len(hit), hit if limit is None else hit[:limit]


def of_backend(be):
    """(census, records) of a Backend (the oracle, or a GPU handle through its read-back)."""
    cfg = be.config
    nodes = be.read_nodes()
    return (census_of(nodes, be.read_clusters(), be.N, cfg.log_cap, cfg.variant_flags),
            records_of(nodes, be.N, cfg.log_cap, cfg.variant_flags, cfg.cluster_offset))


_cache = {}


def oracle_at(cfg, ticks):
    """[(census, records)] of an oracle run of cfg from init-node, one per checkpoint of the
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


def population(census):
    """by_class in the table's column order."""
    return [census["by_class"][k] for k in CLASSES]
