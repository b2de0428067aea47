"""ctypes mirror of include/raftsim.h (the C ABI of libraftsim.so).

The structure layouts here must match the header byte for byte; tests/test_abi.py checks the sizes
and offsets against the C compiler's view.
"""
from __future__ import annotations

import ctypes as C

MAX_NODES = 9
MAX_INBOX = 16

COUNTER_NAMES = ["ev_rv", "ev_ae", "ev_cs", "ev_vr", "ev_ar", "ev_timeout", "ev_heartbeat",
                 "leaders", "sent", "delivered", "dropped", "partitioned", "duplicated",
                 "overflow", "to_halted", "client_injected", "halt_ioobe", "halt_npe", "halt_cce",
                 "halt_overflow", "entries_appended", "entries_applied", "payload_evicted",
                 "viol_election", "viol_log", "viol_complete", "redirects", "client_abandoned"]


class Config(C.Structure):
    _fields_ = [("n_clusters", C.c_uint32), ("cluster_offset", C.c_uint32),
                ("nodes", C.c_uint32), ("log_cap", C.c_uint32), ("arena_cap", C.c_uint32),
                ("inbox_cap", C.c_uint32), ("seed", C.c_uint64), ("hb", C.c_uint32),
                ("el_base", C.c_uint32), ("el_span", C.c_uint32), ("drop_ppm", C.c_uint32),
                ("dup_ppm", C.c_uint32), ("dmin", C.c_uint32), ("dmax", C.c_uint32),
                ("part_ppm", C.c_uint32), ("part_epoch", C.c_uint32),
                ("client_ppm", C.c_uint32), ("variant_flags", C.c_uint32),
                ("device", C.c_int32), ("ticks_per_launch", C.c_uint32),
                ("commit_stream_cap", C.c_uint32), ("trace_cap", C.c_uint32),
                ("trace_entry_cap", C.c_uint32), ("schedule", C.c_uint32),
                ("client_period", C.c_uint32), ("client_burst", C.c_uint32),
                ("client_redirects", C.c_uint32), ("n_devices", C.c_int32)]


class Node(C.Structure):
    _fields_ = [("role", C.c_uint8), ("voted_for", C.c_uint8), ("leader_id", C.c_uint8),
                ("fault", C.c_uint8), ("entries_is_seq", C.c_uint8), ("ls_present", C.c_uint8),
                ("votes", C.c_uint16), ("ls_keys", C.c_uint16), ("reserved0", C.c_uint16),
                ("current_term", C.c_uint32), ("commit_index", C.c_uint32),
                ("log_len", C.c_uint32), ("deadline", C.c_uint32),
                ("next_index", C.c_int32 * MAX_NODES), ("match_index", C.c_int32 * MAX_NODES),
                ("last_led_term", C.c_uint32), ("arena_base", C.c_uint32),
                ("arena_frontier", C.c_uint32), ("req_count", C.c_uint32),
                ("res_count", C.c_uint32), ("commit_count", C.c_uint32),
                ("trace_hash", C.c_uint64)]

    def as_dict(self, n_nodes):
        d = {f: getattr(self, f) for f, _ in self._fields_
             if not f.startswith("reserved")}
        d["next_index"] = list(self.next_index)[:n_nodes]
        d["match_index"] = list(self.match_index)[:n_nodes]
        return d


class Msg(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in
                ("arrival", "hdr", "term", "a", "b", "eterm", "eval", "poff")]

    def words(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


class Entry(C.Structure):
    _fields_ = [("term", C.c_uint32), ("val", C.c_uint32)]


class TraceEvent(C.Structure):
    _fields_ = [("tick", C.c_uint32), ("seq", C.c_uint32), ("msg", Msg),
                ("role", C.c_uint8), ("voted_for", C.c_uint8), ("leader_id", C.c_uint8),
                ("ls_present", C.c_uint8), ("votes", C.c_uint16), ("ls_keys", C.c_uint16),
                ("current_term", C.c_uint32), ("next_index", C.c_int32 * MAX_NODES),
                ("match_index", C.c_int32 * MAX_NODES), ("entries_seq", C.c_uint32)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_}
        d["msg"] = {f: getattr(self.msg, f) for f, _ in Msg._fields_}
        d["next_index"] = list(self.next_index)
        d["match_index"] = list(self.match_index)
        return d


class Cluster(C.Structure):
    _fields_ = [("hwm_index", C.c_uint32), ("hwm_term", C.c_uint32), ("hwm_val", C.c_uint32),
                ("client_next", C.c_uint32), ("client_count", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]

    def as_dict(self):
        return {"hwm": (self.hwm_index, self.hwm_term, self.hwm_val),
                "client_next": self.client_next, "client_count": self.client_count}


class Counters(C.Structure):
    _fields_ = [("node_ticks", C.c_uint64), ("first_violation_tick", C.c_uint64),
                ("c", C.c_uint64 * len(COUNTER_NAMES)), ("payload_max", C.c_uint64)]

    def as_dict(self):
        d = {name: self.c[i] for i, name in enumerate(COUNTER_NAMES)}
        d["node_ticks"] = self.node_ticks
        d["payload_max"] = self.payload_max
        d["first_violation_tick"] = (None if self.first_violation_tick == 2 ** 64 - 1
                                     else self.first_violation_tick)
        return d


class Violation(C.Structure):
    """raft_violation_t: one violating cluster (no reference counterpart)."""
    _fields_ = [("cluster", C.c_uint32), ("first_tick", C.c_uint32), ("count", C.c_uint32 * 3),
                ("kinds", C.c_uint32)]


# raft_viol_kind bits, in the order of raft_violation_t.count
VIOL_KINDS = {"election": 1, "log": 2, "complete": 4}

P = C.POINTER
_SIGS = {
    "abi_version": (C.c_int, []),
    "default_config": (None, [P(Config)]),
    "create": (C.c_int, [P(Config), P(C.c_void_p)]),
    "step": (C.c_int, [C.c_void_p, C.c_uint32]),
    "step_async": (C.c_int, [C.c_void_p, C.c_uint32]),
    "sync": (C.c_int, [C.c_void_p]),
    "tick": (C.c_uint64, [C.c_void_p]),
    "set_tick": (C.c_int, [C.c_void_p, C.c_uint64]),
    "read_nodes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(Node)]),
    "write_nodes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(Node)]),
    "read_queue": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, P(Msg),
                             C.c_uint32]),
    "write_queue": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, P(Msg),
                              C.c_uint32]),
    "read_arena": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(Entry), C.c_uint32]),
    "write_arena": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(Entry), C.c_uint32]),
    "read_commit_stream": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(C.c_uint32),
                                     C.c_uint32]),
    "write_commit_stream": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(C.c_uint32),
                                      C.c_uint32]),
    "read_trace": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, P(TraceEvent),
                             C.c_uint32]),
    "read_trace_entries": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, P(Entry),
                                     C.c_uint32]),
    "read_clusters": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(Cluster)]),
    "write_clusters": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(Cluster)]),
    "read_counters": (C.c_int, [C.c_void_p, P(Counters)]),
    "digest": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, P(C.c_uint64)]),
    "last_step_timing": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_uint32)]),
    "last_span": (C.c_int, [C.c_void_p, P(C.c_double)]),
    "destroy": (None, [C.c_void_p]),
    "last_error": (C.c_char_p, []),
}

# Every symbol include/raftsim.h declares (tests/test_abi.py checks the header agrees).
PRODUCT_SYMBOLS = ["raft_sim_" + n for n in _SIGS]


# The entry points with no reference counterpart that the oracle library does not mirror
# (include/raftsim.h, "Violation records"): bound for the product library only, under their own
# prefix, so PRODUCT_SYMBOLS stays the raft_sim_* set the oracle implements as raft_ref_*.
_VIOL_SIGS = {
    "read": (C.c_int64, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, P(Violation),
                         C.c_uint32]),
    "clear": (C.c_int, [C.c_void_p]),
}
VIOL_SYMBOLS = ["raft_viol_" + n for n in _VIOL_SIGS]


# raft_cluster_class bits (include/raftsim.h, "State census"; SIM_SPEC.md, "Derived, not state")
CLUSTER_CLASSES = {"no_leader": 1, "one_leader": 2, "multi_leader": 4, "halted": 8,
                   "no_quorum": 16, "same_term_leaders": 32, "log_full": 64, "candidate": 128,
                   "settled": 256}
CLS_ALL = 511


class Census(C.Structure):
    """raft_census_t: the census of a handle's clusters (no reference counterpart)."""
    _fields_ = [("clusters", C.c_uint64), ("nodes", C.c_uint64), ("by_class", C.c_uint64 * 16),
                ("leaders_hist", C.c_uint64 * (MAX_NODES + 1)),
                ("live_hist", C.c_uint64 * (MAX_NODES + 1)), ("role_nodes", C.c_uint64 * 4),
                ("fault_nodes", C.c_uint64 * 5), ("term_min", C.c_uint64),
                ("term_max", C.c_uint64), ("term_sum", C.c_uint64), ("commit_max", C.c_uint64),
                ("commit_sum", C.c_uint64), ("len_max", C.c_uint64), ("len_sum", C.c_uint64),
                ("req_queued", C.c_uint64), ("res_queued", C.c_uint64), ("hwm_max", C.c_uint64),
                ("hwm_sum", C.c_uint64)]

    def as_dict(self, n_nodes):
        d = {}
        for f, t in self._fields_:               # the structure's order
            v = getattr(self, f)
            d[f] = int(v) if t is C.c_uint64 else [int(x) for x in v]
        d["by_class"] = {k: d["by_class"][b.bit_length() - 1] for k, b in CLUSTER_CLASSES.items()}
        d["leaders_hist"] = d["leaders_hist"][:n_nodes + 1]
        d["live_hist"] = d["live_hist"][:n_nodes + 1]
        return d


class ClusterState(C.Structure):
    """raft_cluster_state_t: one selected cluster (no reference counterpart)."""
    _fields_ = [("cluster", C.c_uint32), ("classes", C.c_uint32), ("leaders", C.c_uint16),
                ("halted", C.c_uint16), ("term_max", C.c_uint32), ("term_min", C.c_uint32),
                ("commit_max", C.c_uint32), ("len_max", C.c_uint32), ("queued", C.c_uint32)]


# The state census, like the violation records, has no oracle counterpart: bound for the product
# library only, under its own prefix.
_CENSUS_SIGS = {
    "read": (C.c_int, [C.c_void_p, P(Census)]),
    "select": (C.c_int64, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, P(ClusterState),
                           C.c_uint32]),
}
CENSUS_SYMBOLS = ["raft_census_" + n for n in _CENSUS_SIGS]


# raft_audit_class bits (include/raftsim.h, "Log audit"; SIM_SPEC.md, "Derived, not state")
AUDIT_CLASSES = {"diverged": 1, "commit_diverged": 2, "match_broken": 4, "term_order": 8,
                 "identical": 16}
AUD_ALL = 31
_NONE32, _NONE64 = 2 ** 32 - 1, 2 ** 64 - 1


class Audit(C.Structure):
    """raft_audit_t: the log audit of a handle's clusters (no reference counterpart)."""
    _fields_ = [("clusters", C.c_uint64), ("by_class", C.c_uint64 * 8), ("entries", C.c_uint64),
                ("agree_sum", C.c_uint64), ("agree_min", C.c_uint64), ("agree_max", C.c_uint64),
                ("diverged_nodes", C.c_uint64), ("commit_diverged_nodes", C.c_uint64),
                ("diverge_index_min", C.c_uint64), ("commit_diverge_index_min", C.c_uint64)]

    def as_dict(self):
        d = {}
        for f, t in self._fields_:               # the structure's order
            v = getattr(self, f)
            d[f] = int(v) if t is C.c_uint64 else [int(x) for x in v]
        d["by_class"] = {k: d["by_class"][b.bit_length() - 1] for k, b in AUDIT_CLASSES.items()}
        for f in ("diverge_index_min", "commit_diverge_index_min"):
            d[f] = None if d[f] == _NONE64 else d[f]
        return d


class AuditRecord(C.Structure):
    """raft_audit_record_t: one selected cluster (no reference counterpart)."""
    _fields_ = [("cluster", C.c_uint32), ("classes", C.c_uint32), ("agree_len", C.c_uint32),
                ("diverge_index", C.c_uint32), ("commit_diverge_index", C.c_uint32),
                ("order_index", C.c_uint32), ("diverged", C.c_uint16),
                ("commit_diverged", C.c_uint16), ("len_min", C.c_uint32)]

    def as_dict(self, n_nodes, cluster_offset=0):
        ids = range(1, n_nodes + 1)
        idx = lambda v: None if v == _NONE32 else v  # noqa: E731
        return {"cluster": self.cluster, "global_id": cluster_offset + self.cluster,
                "classes": tuple(k for k, b in AUDIT_CLASSES.items() if self.classes & b),
                "agree_len": self.agree_len, "diverge_index": idx(self.diverge_index),
                "commit_diverge_index": idx(self.commit_diverge_index),
                "order_index": idx(self.order_index),
                "diverged": [i for i in ids if (self.diverged >> i) & 1],
                "commit_diverged": [i for i in ids if (self.commit_diverged >> i) & 1],
                "len_min": self.len_min}


# The log audit, like the census, has no oracle counterpart: bound for the product library only,
# under its own prefix.
_AUDIT_SIGS = {
    "read": (C.c_int, [C.c_void_p, P(Audit)]),
    "select": (C.c_int64, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, P(AuditRecord),
                           C.c_uint32]),
}
AUDIT_SYMBOLS = ["raft_audit_" + n for n in _AUDIT_SIGS]


# raft_gather_part bits (include/raftsim.h, "Cluster packs"), in the order of a record's parts
GATHER_PARTS = {"cluster": 1, "nodes": 2, "queues": 4, "logs": 8, "arenas": 16, "streams": 32}
GATHER_ALL = 63


class GatherLayout(C.Structure):
    """raft_gather_layout_t: where a pack's parts stand in a cluster's record."""
    _fields_ = [("stride", C.c_uint64), ("off", C.c_uint64 * 6), ("size", C.c_uint64 * 6)]

    def as_dict(self):
        """{"stride": bytes per cluster, part name: (offset, size) for the parts asked for}."""
        d = {"stride": int(self.stride)}
        for b, name in enumerate(GATHER_PARTS):
            if self.off[b] != _NONE64:
                d[name] = (int(self.off[b]), int(self.size[b]))
        return d


def gather_layout(nodes, inbox_cap, log_cap, arena_cap, commit_stream_cap, parts):
    """raft_gather_layout's answer for a config, as GatherLayout.as_dict gives it (needs no
    library): parts in bit order, each on a 16-byte boundary, absent parts take no room."""
    A = arena_cap or 4 * log_cap
    sizes = (C.sizeof(Cluster), nodes * C.sizeof(Node), nodes * 2 * inbox_cap * C.sizeof(Msg),
             nodes * log_cap * C.sizeof(Entry), nodes * A * C.sizeof(Entry),
             nodes * commit_stream_cap * 4)
    d, off = {}, 0
    for (name, bit), size in zip(GATHER_PARTS.items(), sizes):
        if parts & bit:
            d[name] = (off, size)
            off += (size + 15) & ~15
    return dict(stride=off, **d)


# Cluster packs, like the audit, have no oracle counterpart: bound for the product library only,
# under their own prefix.
_GATHER_SIGS = {
    "layout": (C.c_int, [C.c_void_p, C.c_uint32, P(GatherLayout)]),
    "read": (C.c_int64, [C.c_void_p, P(C.c_uint32), C.c_uint32, C.c_uint32, C.c_void_p,
                         C.c_uint64]),
}
GATHER_SYMBOLS = ["raft_gather_" + n for n in _GATHER_SIGS]


# The packs' way back (include/raftsim.h, raft_scatter_write): under a prefix of its own, so the
# raft_gather_* set stays the two read-side calls.
_SCATTER_SIGS = {
    "write": (C.c_int64, [C.c_void_p, P(C.c_uint32), P(C.c_uint32), C.c_uint32, C.c_uint32,
                          C.c_void_p, C.c_uint32]),
}
SCATTER_SYMBOLS = ["raft_scatter_" + n for n in _SCATTER_SIGS]
# the parts a pack must hold to be written back (and "streams" when commit_stream_cap > 0)
SCATTER_PARTS = ("cluster", "nodes", "queues", "arenas")


# Cluster state copied on the device (include/raftsim.h, "Cluster clones"): (dst, targets, src,
# sources, n), under a prefix of its own like the scatter.
_CLONE_SIGS = {
    "write": (C.c_int64, [C.c_void_p, P(C.c_uint32), C.c_void_p, P(C.c_uint32), C.c_uint32]),
}
CLONE_SYMBOLS = ["raft_clone_" + n for n in _CLONE_SIGS]
# the config fields two handles must share for a clone between them (arena_cap: the effective one)
CLONE_SHAPE = ("nodes", "inbox_cap", "log_cap", "arena_cap", "commit_stream_cap")


# Node restarts (include/raftsim.h, "Node restarts"): the list form (sim, clusters, node masks, n,
# mode) and the supervisor form (sim, fault_mask, mode); both return the nodes restarted.
_RESTART_SIGS = {
    "write": (C.c_int64, [C.c_void_p, P(C.c_uint32), P(C.c_uint16), C.c_uint32, C.c_uint32]),
    "where": (C.c_int64, [C.c_void_p, C.c_uint32, C.c_uint32]),
}
RESTART_SYMBOLS = ["raft_restart_" + n for n in _RESTART_SIGS]
RESTART_MODES = {"amnesia": 0, "durable": 1}                  # raft_restart_mode
# raft_node_t.fault by name: bit f of a raft_restart_where fault_mask is fault code f
FAULT_CODES = {"running": 0, "ioobe": 1, "npe": 2, "cce": 3, "overflow": 4}


def bind(lib, prefix, optional=(), sigs=None):
    """Attach argtypes/restype to `lib`'s `prefix + name` functions; return {name: fn}."""
    fns = {}
    for name, (res, args) in (_SIGS if sigs is None else sigs).items():
        sym = prefix + name
        if not hasattr(lib, sym):
            if name in optional:
                continue
            raise OSError(f"{sym} missing from {lib._name}")
        f = getattr(lib, sym)
        f.restype = res
        f.argtypes = args
        fns[name] = f
    return fns
