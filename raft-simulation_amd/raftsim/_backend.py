"""Host-side handle over a library that implements the include/raftsim.h ABI."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

ROLE_NAMES = {0: ":follower", 1: ":candidate", 2: ":leader", 3: ":follwer"}
FAULT_NAMES = {0: None, 1: "IndexOutOfBoundsException", 2: "NullPointerException",
               3: "ClassCastException", 4: "LogCapacityExceeded"}


class RaftSimError(RuntimeError):
    pass


def make_config(fns, **kw) -> _abi.Config:
    cfg = _abi.Config()
    fns["default_config"](C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown config field {k!r}")
        setattr(cfg, k, v)
    return cfg


def _npz(path):
    path = str(path)
    return path if path.endswith(".npz") else path + ".npz"


class ClusterPack:
    """The full canonical state of some clusters of a handle at one tick, as raft_gather_read
    packed it (include/raftsim.h, "Cluster packs"): one numpy.uint8 buffer of len(clusters)
    records of `layout["stride"]` bytes, and what is needed to read it without the handle.

      config    the source handle's config, a dict of raft_sim_config_t fields
      tick      the source handle's tick when the pack was taken
      clusters  the handle-local ids of the packed clusters, in record order; global_ids adds
                the config's cluster_offset
      layout    {"stride": bytes, part name: (offset, size)} for the parts the pack holds
      data      the records

    The accessors take the position `i` of a cluster in the pack and return views of `data` or
    plain Python values decoded from them; none of them copies a part."""

    def __init__(self, config, tick, clusters, layout, data):
        self.config = dict(config)
        self.tick = int(tick)
        self.clusters = [int(c) for c in clusters]
        self.layout = {k: (int(v) if k == "stride" else (int(v[0]), int(v[1])))
                       for k, v in layout.items()}
        self.data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        if self.data.size != len(self.clusters) * self.layout["stride"]:
            raise ValueError("the buffer is not len(clusters) * stride bytes")
        self.N = self.config["nodes"]
        self.Q = self.config["inbox_cap"]
        self.L = self.config["log_cap"]
        self.A = self.config["arena_cap"] or 4 * self.L
        self.SC = self.config["commit_stream_cap"]
        self.nodes = _PackNodes(self)

    def __len__(self):
        return len(self.clusters)

    @property
    def parts(self):
        return tuple(k for k in _abi.GATHER_PARTS if k in self.layout)

    @property
    def global_ids(self):
        return [self.config["cluster_offset"] + c for c in self.clusters]

    def part(self, i, name):
        """The bytes of part `name` of the pack's i-th cluster (a view)."""
        if name not in self.layout:
            raise ValueError(f"the pack holds no {name!r} part (it has {list(self.parts)})")
        if not 0 <= i < len(self.clusters):
            raise IndexError(f"position {i} outside the pack's {len(self.clusters)} clusters")
        off, size = self.layout[name]
        at = i * self.layout["stride"] + off
        return self.data[at:at + size]

    def _node(self, i, node_id):
        if not 1 <= node_id <= self.N:
            raise IndexError(f"node id {node_id} outside 1..{self.N}")
        return self.nodes[i][node_id - 1]

    def node_dicts(self, i):
        """The cluster's node records as read_nodes gives them."""
        return [n.as_dict(self.N) for n in self.nodes[i]]

    def cluster(self, i):
        """The cluster record as read_clusters gives it."""
        return _abi.Cluster.from_buffer(self.part(i, "cluster")).as_dict()

    def queue(self, i, node_id, which):
        """The messages of the node's req (which=0) or resp (1) queue, head first, as 8-word
        tuples (what read_queue gives)."""
        n = self._node(i, node_id)
        cnt = min(n.res_count if which else n.req_count, self.Q)
        q = self.part(i, "queues").view(np.uint32).reshape(self.N, 2, self.Q, 8)
        return [tuple(m) for m in q[node_id - 1, which, :cnt].tolist()]

    def log(self, i, node_id):
        """The node's logical log as (term, val) tuples (what Backend.log gives)."""
        n = min(self._node(i, node_id).log_len, self.L)
        lg = self.part(i, "logs").view(np.uint32).reshape(self.N, self.L, 2)
        return [tuple(e) for e in lg[node_id - 1, :n].tolist()]

    def arena(self, i, node_id):
        """The node's raw log arena as (term, val) tuples (what read_arena gives)."""
        self._node(i, node_id)
        ar = self.part(i, "arenas").view(np.uint32).reshape(self.N, self.A, 2)
        return [tuple(e) for e in ar[node_id - 1].tolist()]

    def commit_stream(self, i, node_id):
        """The newest committed values the ring retains, oldest first (what commit_stream gives)."""
        kept = min(self._node(i, node_id).commit_count, self.SC)
        if not self.SC:
            self.part(i, "streams")
            return []
        st = self.part(i, "streams").view(np.uint32).reshape(self.N, self.SC)
        return st[node_id - 1, :kept].tolist()

    def save(self, path):
        """Write the pack to one .npz file (numpy arrays and a JSON string; no pickle)."""
        import json
        meta = json.dumps({"config": self.config, "tick": self.tick, "layout": self.layout})
        np.savez(_npz(path), data=self.data, clusters=np.asarray(self.clusters, dtype=np.uint32),
                 meta=np.asarray(meta))
        return _npz(path)

    @classmethod
    def load(cls, path):
        import json
        with np.load(_npz(path), allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            return cls(meta["config"], meta["tick"], z["clusters"].tolist(), meta["layout"],
                       z["data"])


class _PackNodes:
    """pack.nodes: nodes[i] is the i-th cluster's N raft_node_t as an _abi.Node array over the
    pack's bytes (nodes[i][k] is node id k + 1)."""

    def __init__(self, pack):
        self._pack = pack

    def __len__(self):
        return len(self._pack.clusters)

    def __getitem__(self, i):
        p = self._pack
        return (_abi.Node * p.N).from_buffer(p.part(i, "nodes"))


class Backend:
    """One simulator handle. `lib_path` + `prefix` select the implementation."""

    def __init__(self, lib_path, prefix, **config):
        self._lib = C.CDLL(str(lib_path))
        self._fns = _abi.bind(self._lib, prefix, optional=("last_step_timing", "last_span"))
        if self._fns["abi_version"]() != 2:
            raise RaftSimError("ABI version mismatch")
        self.config = make_config(self._fns, **config)
        h = C.c_void_p()
        self._check(self._fns["create"](C.byref(self.config), C.byref(h)))
        self._h = h
        self.N = self.config.nodes
        self.C = self.config.n_clusters
        # True once the host wrote state or the clock (write_*, set_tick): such a run is no longer
        # the one the config alone reproduces from init-node (raftsim.replay refuses it)
        self.host_written = False

    # -- plumbing -------------------------------------------------------------------------------
    def _check(self, rc):
        if rc < 0:
            raise RaftSimError(f"rc={rc}: {self._fns['last_error']().decode()}")
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._fns["destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- stepping -------------------------------------------------------------------------------
    def step(self, n_ticks):
        self._check(self._fns["step"](self._h, int(n_ticks)))

    def step_async(self, n_ticks):
        """Enqueue n_ticks without waiting (the oracle runs them at once); see sync()."""
        self._check(self._fns["step_async"](self._h, int(n_ticks)))

    def sync(self):
        self._check(self._fns["sync"](self._h))

    @property
    def tick(self):
        return int(self._fns["tick"](self._h))

    def set_tick(self, tick):
        """Resume at `tick` (state restored through the write_* calls; SIM_SPEC deadlines are
        absolute ticks)."""
        self.host_written = True
        self._check(self._fns["set_tick"](self._h, int(tick)))

    def last_step_timing(self):
        ms, n = C.c_double(), C.c_uint32()
        self._check(self._fns["last_step_timing"](self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_span(self):
        """Device ms of everything the last step (or the steps since the previous sync) enqueued."""
        ms = C.c_double()
        self._check(self._fns["last_span"](self._h, C.byref(ms)))
        return ms.value

    # -- state ----------------------------------------------------------------------------------
    def read_nodes_raw(self, c0=0, nc=None):
        nc = self.C - c0 if nc is None else nc
        arr = (_abi.Node * (nc * self.N))()
        self._check(self._fns["read_nodes"](self._h, c0, nc, arr))
        return arr

    def read_nodes(self, c0=0, nc=None):
        return [n.as_dict(self.N) for n in self.read_nodes_raw(c0, nc)]

    def write_nodes(self, c0, records):
        self.host_written = True
        nc = len(records) // self.N
        arr = (_abi.Node * len(records))()
        for i, r in enumerate(records):
            if isinstance(r, _abi.Node):
                arr[i] = r
                continue
            for k, v in r.items():
                if k in ("next_index", "match_index"):
                    getattr(arr[i], k)[:len(v)] = list(v)
                elif k not in ("req_count", "res_count"):
                    setattr(arr[i], k, v)
        self._check(self._fns["write_nodes"](self._h, c0, nc, arr))

    def read_queue(self, cluster, node_id, which):
        buf = (_abi.Msg * _abi.MAX_INBOX)()
        n = self._check(self._fns["read_queue"](self._h, cluster, node_id, which, buf,
                                                _abi.MAX_INBOX))
        return [buf[i].words() for i in range(n)]

    def write_queue(self, cluster, node_id, which, msgs):
        self.host_written = True
        buf = (_abi.Msg * max(1, len(msgs)))()
        for i, w in enumerate(msgs):
            for f, v in zip(("arrival", "hdr", "term", "a", "b", "eterm", "eval", "poff"), w):
                setattr(buf[i], f, v)
        self._check(self._fns["write_queue"](self._h, cluster, node_id, which, buf, len(msgs)))

    def read_arena(self, cluster, node_id):
        A = self._check(self._fns["read_arena"](self._h, cluster, node_id, None, 0))
        buf = (_abi.Entry * A)()
        self._check(self._fns["read_arena"](self._h, cluster, node_id, buf, A))
        return [(e.term, e.val) for e in buf]

    def write_arena(self, cluster, node_id, entries):
        self.host_written = True
        buf = (_abi.Entry * max(1, len(entries)))()
        for i, (t, v) in enumerate(entries):
            buf[i].term, buf[i].val = t, v
        self._check(self._fns["write_arena"](self._h, cluster, node_id, buf, len(entries)))

    def log(self, cluster, node_id):
        """The node's logical log :entries (log.clj:33-34) as (term, val) tuples."""
        rec = self.read_nodes(cluster, 1)[node_id - 1]
        ar = self.read_arena(cluster, node_id)
        A = len(ar)
        return [ar[(rec["arena_base"] + i) % A] for i in range(rec["log_len"])]

    def commit_stream(self, cluster, node_id):
        """F2: the committed :val's apply-entries! wrote to node_<id>.log (log.clj:69-76), as far
        back as the configured ring (commit_stream_cap) reaches, oldest first."""
        cap = max(1, self.config.commit_stream_cap)
        buf = (C.c_uint32 * cap)()
        n = self._check(self._fns["read_commit_stream"](self._h, cluster, node_id, buf, cap))
        return list(buf[:n])

    def write_commit_stream(self, cluster, node_id, vals):
        self.host_written = True
        buf = (C.c_uint32 * max(1, len(vals)))(*vals)
        self._check(self._fns["write_commit_stream"](self._h, cluster, node_id, buf, len(vals)))

    def write_commit_logs(self, directory, cluster=0):
        """Write node_<id>.log files the way the reference's Log component does (log.clj:16-18):
        one committed value per line. Only the retained tail of the stream is available."""
        from pathlib import Path
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        for i in range(1, self.N + 1):
            (d / f"node_{i}.log").write_text("".join(f"{v}\n" for v in self.commit_stream(cluster, i)))

    def trace(self, cluster, node_id, first=0):
        """F3: the node's recorded `wait` iterations with seq >= first (core.clj:182-186), oldest
        first, as dicts of raft_trace_event_t fields."""
        out, cap = [], max(1, self.config.trace_cap)
        buf = (_abi.TraceEvent * cap)()
        while True:
            n = self._check(self._fns["read_trace"](self._h, cluster, node_id, first, buf, cap))
            out.extend(buf[i].as_dict() for i in range(n))
            if n < cap:
                return out
            first = out[-1]["seq"] + 1

    def trace_entries(self, cluster, node_id, first, count):
        """The `count` trace-entry-ring entries from index `first` as (term, val) pairs, or None
        when the ring no longer holds them all (or trace_entry_cap is 0)."""
        buf = (_abi.Entry * max(1, count))()
        n = self._fns["read_trace_entries"](self._h, cluster, node_id, first, buf, count)
        if n != count:
            return None
        return [(buf[i].term, buf[i].val) for i in range(n)]

    def edn_trace(self, cluster, node_id, first=0, set_order="sorted"):
        """The reference's stdout for node `node_id` of `cluster` from event `first` on:
        `; Node` / (prn node) / `; Message` / (prn message) per wait (core.clj:182-186)."""
        from . import edn
        parts = []
        for e in self.trace(cluster, node_id, first):
            entries = None
            if (e["msg"]["hdr"] & 7) == 2:
                cnt = e["msg"]["hdr"] >> 16
                entries = self.trace_entries(cluster, node_id, e["entries_seq"], cnt) if cnt else []
            parts.append(edn.format_event(e, entries, node_id, self.N, set_order))
        return "".join(parts)

    def write_traces(self, directory, cluster=0, set_order="sorted"):
        """One file per node, node_<id>.out, holding what that node's JVM prints per event."""
        from pathlib import Path
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        for i in range(1, self.N + 1):
            (d / f"node_{i}.out").write_text(self.edn_trace(cluster, i, set_order=set_order))

    def read_clusters(self, c0=0, nc=None):
        """Per-cluster records: checker high-water mark and client-injection cursor."""
        nc = self.C - c0 if nc is None else nc
        arr = (_abi.Cluster * nc)()
        self._check(self._fns["read_clusters"](self._h, c0, nc, arr))
        return [r.as_dict() for r in arr]

    def write_clusters(self, c0, recs):
        self.host_written = True
        arr = (_abi.Cluster * len(recs))()
        for i, r in enumerate(recs):
            arr[i].hwm_index, arr[i].hwm_term, arr[i].hwm_val = r["hwm"]
            arr[i].client_next, arr[i].client_count = r["client_next"], r["client_count"]
        self._check(self._fns["write_clusters"](self._h, c0, len(recs), arr))

    def counters(self):
        c = _abi.Counters()
        self._check(self._fns["read_counters"](self._h, C.byref(c)))
        return c.as_dict()

    def digest(self, c0=0, nc=None):
        nc = self.C - c0 if nc is None else nc
        out = np.zeros(nc, dtype=np.uint64)
        self._check(self._fns["digest"](self._h, c0, nc,
                                        out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def restore_cluster(self, pack, i, cluster=0):
        """Make cluster `cluster` of this handle the pack's i-th cluster at the pack's tick, through
        the write_* calls: set_tick (the whole handle's clock), write_nodes, write_clusters, every
        write_arena, every write_queue, then every write_commit_stream. The handle must have the
        pack's nodes, log_cap, arena_cap, inbox_cap and commit_stream_cap; for the cluster to go on
        as it would have in its source, also its timers, rates and seed, and cluster_offset +
        cluster equal to the packed cluster's global id (replay_config gives such a config).
        Needs the parts cluster, nodes, queues and arenas, and streams when commit_stream_cap > 0:
        ValueError names a missing one."""
        need = ["cluster", "nodes", "queues", "arenas"] + (["streams"] if pack.SC else [])
        for name in need:
            if name not in pack.layout:
                raise ValueError(f"restore_cluster needs the {name!r} part; the pack holds "
                                 f"{list(pack.parts)}")
        A = self.config.arena_cap or 4 * self.config.log_cap
        mine = (self.N, self.config.inbox_cap, self.config.log_cap, A,
                self.config.commit_stream_cap)
        if mine != (pack.N, pack.Q, pack.L, pack.A, pack.SC):
            raise ValueError("restore_cluster: the handle's nodes, inbox_cap, log_cap, arena_cap, "
                             f"commit_stream_cap {mine} are not the pack's "
                             f"{(pack.N, pack.Q, pack.L, pack.A, pack.SC)}")
        ids = range(1, self.N + 1)
        self.set_tick(pack.tick)
        self.write_nodes(cluster, list(pack.nodes[i]))
        self.write_clusters(cluster, [pack.cluster(i)])
        for k in ids:
            self.write_arena(cluster, k, pack.arena(i, k))
        for k in ids:
            for which in (0, 1):
                self.write_queue(cluster, k, which, pack.queue(i, k, which))
        if pack.SC:
            for k in ids:
                self.write_commit_stream(cluster, k, pack.commit_stream(i, k))

    # -- reference vocabulary -------------------------------------------------------------------
    def node_map(self, cluster, node_id):
        """The node as the reference's `prn node` would show it (core.clj:31-38,182-183)."""
        r = self.read_nodes(cluster, 1)[node_id - 1]
        ls = None
        if r["ls_present"]:
            keys = [p for p in range(1, self.N + 1) if (r["ls_keys"] >> p) & 1]
            ls = {":next-index": {p: r["next_index"][p - 1] for p in keys},
                  ":match-index": {p: r["match_index"][p - 1] for p in keys}}
        return {":id": node_id, ":state": ROLE_NAMES[r["role"]],
                ":current-term": r["current_term"],
                ":voted-for": r["voted_for"] or None, ":leader-id": r["leader_id"] or None,
                ":leader-state": ls,
                ":votes": {p for p in range(1, self.N + 1) if (r["votes"] >> p) & 1},
                "halted": FAULT_NAMES[r["fault"]]}


# The default trace rings of a replay handle: one cluster, so a few MB hold a long run's events.
REPLAY_TRACE_CAP = 4096
REPLAY_TRACE_ENTRY_CAP = 1 << 15


class GpuBackend(Backend):
    """A handle of libraftsim.so: the ABI the oracle mirrors, plus the entry points it has no
    counterpart for (include/raftsim.h, "Violation records"): which clusters violated, which
    invariant, when first -- and the config that replays one of them alone; and ("State census")
    what state the clusters are in now, counted and selected on the device; and ("Log audit")
    whether the nodes' logs agree as they stand, and whether they disagree below the commit
    indices; and ("Cluster packs") the full state of the clusters such a query selected, packed
    on the device into a ClusterPack."""

    def __init__(self, lib_path, prefix, **config):
        super().__init__(lib_path, prefix, **config)
        self._viol = _abi.bind(self._lib, "raft_viol_", sigs=_abi._VIOL_SIGS)
        self._census = _abi.bind(self._lib, "raft_census_", sigs=_abi._CENSUS_SIGS)
        self._audit = _abi.bind(self._lib, "raft_audit_", sigs=_abi._AUDIT_SIGS)
        self._gather = _abi.bind(self._lib, "raft_gather_", sigs=_abi._GATHER_SIGS)
        self._scatter = _abi.bind(self._lib, "raft_scatter_", sigs=_abi._SCATTER_SIGS)
        self._clone = _abi.bind(self._lib, "raft_clone_", sigs=_abi._CLONE_SIGS)
        self._restart = _abi.bind(self._lib, "raft_restart_", sigs=_abi._RESTART_SIGS)

    # -- what the three device-side queries share ------------------------------------------------
    @staticmethod
    def _mask(names, table, noun):
        mask = 0
        for k in names:
            if k not in table:
                raise ValueError(f"unknown {noun} {k!r} (one of {list(table)})")
            mask |= table[k]
        return mask

    def _selected(self, fn, rec_type, args, limit):
        """(total, the records copied) of the selection entry point fn(handle, *args, out, cap).
        limit None: every match, at the cost of a first call that only counts them; limit 0: one
        call, the total alone."""
        def read(cap):
            buf = (rec_type * max(1, cap))()
            return self._check(int(fn(self._h, *args, buf if cap else None, cap))), buf

        cap = read(0)[0] if limit is None else int(limit)
        total, buf = read(cap)
        return total, buf[:min(total, cap)]

    def _diag_ms(self, symbol):
        f = getattr(self._lib, symbol)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        ms = C.c_double()
        self._check(f(self._h, C.byref(ms)))
        return ms.value

    def diag_last_bails(self):
        """Diagnostic: clusters the steady kernel handed to the general kernel in the last tick
        launch (steady_kernel.hip), or -1 if that launch did not take the steady path."""
        f = self._lib.raftsim_diag_last_bails
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return int(f(self._h))

    def diag_storm_bails(self):
        """Diagnostic: clusters the storm kernel (storm_kernel.hip) listed for the lane-per-node
        STORM body in the last storm launch, summed over shards; -1 if no storm-kernel launch ran
        on this handle."""
        f = self._lib.raftsim_diag_storm_bails
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return int(f(self._h))

    def timed_launches(self):
        """Launches of the last sync window that carried HIP events: last_step_timing's average
        is over these (every general launch, the first steady launch after a sync)."""
        f = self._lib.raftsim_last_timed_launches
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return int(f(self._h))

    def violations(self, kinds=("election", "log", "complete"), t_lo=0, t_hi=None, limit=None):
        """The clusters the checker counted a violation for: (total, records). A cluster matches
        when it has a violation of one of `kinds` and its first violation tick lies in
        [t_lo, t_hi) (t_hi None: no upper bound). `records` lists the matches in ascending cluster
        order, the first `limit` of them when a limit is given (limit=0: the total alone), as
        dicts: cluster (handle-local, as read_nodes takes it), global_id (cluster_offset +
        cluster), first_tick, election / log / complete (the cluster's counts) and kinds (the
        names of its nonzero counts). The selection runs on the device; only the records asked for
        are copied."""
        mask = self._mask(kinds, _abi.VIOL_KINDS, "violation kind")
        t_hi = 2 ** 64 - 1 if t_hi is None else int(t_hi)
        total, found = self._selected(self._viol["read"], _abi.Violation, (mask, int(t_lo), t_hi),
                                      limit)
        off = self.config.cluster_offset
        names = list(_abi.VIOL_KINDS)
        recs = []
        for v in found:
            rec = {"cluster": v.cluster, "global_id": off + v.cluster, "first_tick": v.first_tick}
            rec.update(zip(names, v.count))
            rec["kinds"] = tuple(n for n in names if v.kinds & _abi.VIOL_KINDS[n])
            recs.append(rec)
        return total, recs

    def clear_violations(self):
        """Forget every cluster's violation record (state, digests and counters are unchanged)."""
        self._check(self._viol["clear"](self._h))

    def last_violations_ms(self):
        """Diagnostic: device time (HIP events) of the last violations() query's kernels."""
        return self._diag_ms("raftsim_diag_viol_ms")

    # -- state census (include/raftsim.h, "State census") ---------------------------------------
    def census(self):
        """What state the handle's clusters are in right now, counted on the device (one pass over
        the hot blocks, nothing but the 464-byte result copied): a dict of raft_census_t's fields.
        `by_class` maps every class name (_abi.CLUSTER_CLASSES; SIM_SPEC.md, "Derived, not state")
        to the number of clusters in it; `leaders_hist[i]` / `live_hist[i]` count the clusters with
        exactly i live leaders / live nodes (i = 0..nodes); `role_nodes` counts live nodes by
        role, `fault_nodes` all nodes by fault code; the rest are sums and extrema over all nodes
        (term, commit, len, queued messages) and clusters (hwm). Stream-ordered: valid after
        step_async, which it waits for. Read-only."""
        c = _abi.Census()
        self._check(self._census["read"](self._h, C.byref(c)))
        return c.as_dict(self.N)

    @staticmethod
    def _class_mask(names):
        return GpuBackend._mask(names, _abi.CLUSTER_CLASSES, "cluster class")

    def select(self, any=(), all=(), none=(), limit=None):
        """The clusters in given state classes: (total, records). A cluster matches when it is in
        one of the classes `any` (empty: no such condition), in every class of `all` and in no
        class of `none` (names of _abi.CLUSTER_CLASSES). `records` lists the matches in ascending
        cluster order, the first `limit` of them when a limit is given (limit=0: the total alone),
        as dicts: cluster (handle-local, as read_nodes takes it), global_id (cluster_offset +
        cluster), classes (the names of all the cluster's classes), leaders and halted (lists of
        node ids), term_max, term_min, commit_max, len_max (over all its nodes) and queued
        (messages in its queues). The selection runs on the device; only the records asked for are
        copied. On a run from init-node, raftsim.replay(sim, rec["cluster"]) reruns a selected
        cluster alone with its `wait` trace."""
        masks = [self._class_mask(x) for x in (any, all, none)]
        total, found = self._selected(self._census["select"], _abi.ClusterState, masks, limit)
        off = self.config.cluster_offset
        ids = range(1, self.N + 1)
        recs = []
        for v in found:
            recs.append({
                "cluster": v.cluster, "global_id": off + v.cluster,
                "classes": tuple(k for k, b in _abi.CLUSTER_CLASSES.items() if v.classes & b),
                "leaders": [i for i in ids if (v.leaders >> i) & 1],
                "halted": [i for i in ids if (v.halted >> i) & 1],
                "term_max": v.term_max, "term_min": v.term_min, "commit_max": v.commit_max,
                "len_max": v.len_max, "queued": v.queued})
        return total, recs

    def last_census_ms(self):
        """Diagnostic: device time (HIP events) of the last census() or select() query's kernels."""
        return self._diag_ms("raftsim_diag_census_ms")

    # -- log audit (include/raftsim.h, "Log audit") ----------------------------------------------
    def audit(self):
        """Whether the nodes' logs agree right now, answered on the device from the arenas as they
        stand (one pass over every log, nothing but the 136-byte result copied): a dict of
        raft_audit_t's fields. `by_class` maps every class name (_abi.AUDIT_CLASSES; SIM_SPEC.md,
        "Derived, not state") to the number of clusters in it: diverged (two logs differ at a
        position both hold), commit_diverged (below both commit indices: State Machine Safety is
        broken), match_broken (same index and term, yet not identical up to there), term_order (a
        log's terms decrease somewhere), identical. `entries` is the sum of all log lengths,
        agree_* the common prefix of a cluster's logs over the clusters, *_nodes the nodes that
        belong to a diverging pair, *_index_min the first diverging position anywhere (None: no
        cluster diverges). Stream-ordered: valid after step_async, which it waits for. Read-only.
        The per-cluster records stay on the device until the next step or write of nodes, arenas or
        clusters: an audit_select() after it reads them, not the logs again."""
        a = _abi.Audit()
        self._check(self._audit["read"](self._h, C.byref(a)))
        return a.as_dict()

    @staticmethod
    def _audit_mask(names):
        return GpuBackend._mask(names, _abi.AUDIT_CLASSES, "audit class")

    def audit_select(self, any=(), all=(), none=(), limit=None):
        """The clusters in given audit classes: (total, records), with the predicate and the
        limit of select() over the names of _abi.AUDIT_CLASSES. A record is a dict: cluster
        (handle-local, as read_nodes takes it), global_id, classes (the names of all the cluster's
        classes), agree_len (the common prefix of its N logs), diverge_index /
        commit_diverge_index (the first position at which two logs differ / differ below both
        commit indices; None: nowhere), order_index (the first position whose term exceeds the
        next one's; None), diverged / commit_diverged (the ids of the nodes in such a pair) and
        len_min (the shortest log). The selection runs on the device; only the records asked for
        are copied."""
        masks = [self._audit_mask(x) for x in (any, all, none)]
        total, found = self._selected(self._audit["select"], _abi.AuditRecord, masks, limit)
        off = self.config.cluster_offset
        return total, [v.as_dict(self.N, off) for v in found]

    def last_audit_ms(self):
        """Diagnostic: device time (HIP events) of the last audit() or audit_select() query's
        kernels."""
        return self._diag_ms("raftsim_diag_audit_ms")

    # -- cluster packs (include/raftsim.h, "Cluster packs") --------------------------------------
    def gather_layout(self, parts=tuple(_abi.GATHER_PARTS)):
        """Where the parts (names of _abi.GATHER_PARTS) stand in a cluster's record of this
        handle: {"stride": bytes, part name: (offset, size)}."""
        lay = _abi.GatherLayout()
        mask = self._mask(parts, _abi.GATHER_PARTS, "pack part")
        self._check(self._gather["layout"](self._h, mask, C.byref(lay)))
        return lay.as_dict()

    def gather(self, clusters, parts=tuple(_abi.GATHER_PARTS), limit=None):
        """The full state of the given clusters as a ClusterPack, packed on the device and copied
        once per device instead of once per node and part. `clusters` is a sequence of
        handle-local cluster ids, or of the record dicts violations(), select() and
        audit_select() return (their "cluster" key is used), in any order, duplicates allowed;
        `limit` takes the first that many. `parts` names the parts to pack (_abi.GATHER_PARTS:
        cluster, nodes, queues, logs, arenas, streams); nodes is always added, because the node
        records carry the counts the other parts are read with. Stream-ordered: valid after
        step_async, which it waits for. Read-only."""
        ids = [int(c["cluster"] if isinstance(c, dict) else c) for c in clusters]
        if limit is not None:
            ids = ids[:int(limit)]
        names = [k for k in _abi.GATHER_PARTS if k in set(parts) | {"nodes"}]
        mask = self._mask(parts, _abi.GATHER_PARTS, "pack part") | _abi.GATHER_PARTS["nodes"]
        lay = _abi.GatherLayout()
        self._check(self._gather["layout"](self._h, mask, C.byref(lay)))
        tick = self.tick
        data = np.empty(len(ids) * int(lay.stride), dtype=np.uint8)
        idx = np.asarray(ids, dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= self.C):
            bad = next(i for i, c in enumerate(ids) if not 0 <= c < self.C)
            raise ValueError(f"clusters[{bad}] = {ids[bad]} is outside the handle's {self.C}")
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        got = self._check(int(self._gather["read"](
            self._h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), len(ids), mask,
            data.ctypes.data_as(C.c_void_p), data.size)))
        assert got == data.size and list(lay.as_dict())[1:] == names
        cfg = {f: getattr(self.config, f) for f, _ in _abi.Config._fields_}
        return ClusterPack(cfg, tick, ids, lay.as_dict(), data)

    def last_gather_ms(self):
        """Diagnostic: device time (HIP events) of the last gather()'s kernels."""
        return self._diag_ms("raftsim_diag_gather_ms")

    def scatter(self, pack, clusters=None, records=None):
        """Write records of a ClusterPack into clusters of this handle on the device
        (raft_scatter_write): record records[i] of the pack becomes cluster clusters[i]; returns
        the number of clusters written. `clusters` (handle-local ids, any order, none twice)
        defaults to pack.clusters, `records` (positions in the pack) to 0..len(clusters)-1 and may
        name a position any number of times: one record placed at K ids is K futures of that state.
        The handle must have the pack's nodes, inbox_cap, log_cap, arena_cap and
        commit_stream_cap, and the pack the parts cluster, nodes, queues and arenas (and streams
        when commit_stream_cap > 0): ValueError names what is missing. The clock is not set
        (set_tick does that); violation records, counters and trace rings stay as they are. All or
        nothing: a refused call (RaftSimError naming the first offending position) wrote nothing."""
        check_pack_fits(self.config, pack, "scatter")
        def index_list(xs, name, bound, whose):
            if not isinstance(xs, np.ndarray):
                xs = [int(x["cluster"] if isinstance(x, dict) else x) for x in xs]
            a = np.asarray(xs, dtype=np.int64).reshape(-1)
            out = np.flatnonzero((a < 0) | (a >= bound))
            if out.size:
                raise ValueError(f"{name}[{out[0]}] = {a[out[0]]} is outside {whose} {bound}")
            return np.ascontiguousarray(a, dtype=np.uint32)

        idx = index_list(pack.clusters if clusters is None else clusters, "clusters", self.C,
                         "the handle's")
        n = idx.size
        if records is None:
            if n > len(pack):
                raise ValueError(f"{n} clusters for the pack's {len(pack)} records")
            rec_ptr = None
        else:
            rec = index_list(records, "records", len(pack), "the pack's")
            if rec.size != n:
                raise ValueError(f"{rec.size} records for {n} clusters")
            rec_ptr = rec.ctypes.data_as(C.POINTER(C.c_uint32))
        mask = self._mask(pack.parts, _abi.GATHER_PARTS, "pack part")
        self.host_written = True
        return self._check(int(self._scatter["write"](
            self._h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), rec_ptr, n, mask,
            pack.data.ctypes.data_as(C.c_void_p), len(pack))))

    def last_scatter_ms(self):
        """Diagnostic: device time (HIP events) of the last scatter()'s kernels."""
        return self._diag_ms("raftsim_diag_scatter_ms")

    # -- cluster clones (include/raftsim.h, "Cluster clones") ------------------------------------
    def clone(self, sources, targets, source=None):
        """Make cluster targets[i] of this handle the state of cluster sources[i] of `source`
        (default: this handle) on the device (raft_clone_write), with no pack in host memory:
        returns the number of clusters written. Both lists hold handle-local ids or the record
        dicts violations(), select() and audit_select() return (their "cluster" key is used), in
        any order; a source may be named any number of times (K targets of one source are K
        futures of that state: Philox is keyed by the global cluster id), a target once, and
        within one handle no cluster may be both. The target is what
        scatter(source.gather(sources)) leaves: exact deadlines, no steady certificate. The two
        handles must have the same nodes, inbox_cap, log_cap, arena_cap and commit_stream_cap and
        live on one GPU: ValueError names the field or the position. Neither clock is touched
        (set_tick does that); violation records, counters and trace `seq` numbers are not state
        and are not carried: the target's stay as they are. All or nothing: a refused call
        (RaftSimError naming the first offending position) wrote nothing."""
        src = self if source is None else source
        if not isinstance(src, GpuBackend):
            raise TypeError("clone: the source must be a handle of libraftsim.so")
        check_clone_fits(self.config, src.config)

        def index_list(xs, name, bound):
            if not isinstance(xs, np.ndarray):
                xs = [int(x["cluster"] if isinstance(x, dict) else x) for x in xs]
            a = np.asarray(xs, dtype=np.int64).reshape(-1)
            out = np.flatnonzero((a < 0) | (a >= bound))
            if out.size:
                raise ValueError(f"{name}[{out[0]}] = {a[out[0]]} is outside the handle's {bound}")
            return np.ascontiguousarray(a, dtype=np.uint32)

        src_idx = index_list(sources, "sources", src.C)
        tgt_idx = index_list(targets, "targets", self.C)
        if src_idx.size != tgt_idx.size:
            raise ValueError(f"{src_idx.size} sources for {tgt_idx.size} targets")
        u32p = C.POINTER(C.c_uint32)
        self.host_written = True
        return self._check(int(self._clone["write"](
            self._h, tgt_idx.ctypes.data_as(u32p), src._h, src_idx.ctypes.data_as(u32p),
            tgt_idx.size)))

    def last_clone_ms(self):
        """Diagnostic: device time (HIP events) of the kernels of the last clone() into this
        handle."""
        return self._diag_ms("raftsim_diag_clone_ms")

    # -- node restarts (include/raftsim.h, "Node restarts") --------------------------------------
    def restart(self, targets, nodes=None, mode="amnesia"):
        """Start halted (or any) nodes again on the device at the handle's tick
        (raft_restart_write; SIM_SPEC §4a): returns the number of nodes restarted. `targets` are
        handle-local cluster ids, in any order, none twice, each paired with nodes[i]: a mask (bit
        j = node id j, as `votes`) or a list of node ids; or the record dicts select() returns,
        for which `nodes` defaults to the record's `halted` ids, so
        sim.restart(sim.select(any=["halted"])[1]) restarts every halted node. mode "amnesia" is
        the reference's JVM started again (init-node, a fresh log, nothing read from disk),
        "durable" keeps current_term, voted_for and the log (Raft's Figure 2). Both empty the
        node's queues and re-arm its election timer from the current tick. ValueError names the
        position of a bad shape. All or nothing: a refused call (RaftSimError naming the first
        offending position) restarted nothing."""
        cl, masks = restart_lists(targets, nodes, self.C, self.N)
        self.host_written = True
        return self._check(int(self._restart["write"](
            self._h, cl.ctypes.data_as(C.POINTER(C.c_uint32)),
            masks.ctypes.data_as(C.POINTER(C.c_uint16)), cl.size, restart_mode(mode))))

    def restart_where(self, faults=("ioobe", "npe", "cce", "overflow"), mode="amnesia"):
        """Restart every node of the handle whose fault is one of `faults` (names of
        _abi.FAULT_CODES; "running" names the nodes that have not halted), found and counted on
        the device in one pass (raft_restart_where): returns the number of nodes restarted."""
        mask = self._mask(faults, {k: 1 << v for k, v in _abi.FAULT_CODES.items()}, "fault")
        self.host_written = True
        return self._check(int(self._restart["where"](self._h, mask, restart_mode(mode))))

    def last_restart_ms(self):
        """Diagnostic: device time (HIP events) of the last restart()'s or restart_where()'s
        kernels."""
        return self._diag_ms("raftsim_diag_restart_ms")

    def replay_config(self, cluster, **overrides):
        """The config (a dict of raft_sim_config_t fields) of a handle that simulates cluster
        `cluster` of this one alone: Philox is keyed by the global cluster id, so n_clusters=1 at
        cluster_offset + cluster reproduces it exactly from init-node. The trace rings are on by
        default (the `wait` trace, F3); `overrides` replace any field."""
        return replay_config(self.config, cluster, **overrides)


def restart_mode(mode):
    """raft_restart_mode of a name of _abi.RESTART_MODES or of 0 / 1."""
    if mode in _abi.RESTART_MODES:
        return _abi.RESTART_MODES[mode]
    if mode in (0, 1):
        return int(mode)
    raise ValueError(f"unknown restart mode {mode!r} (one of {list(_abi.RESTART_MODES)})")


def restart_lists(targets, nodes, n_clusters, n_nodes):
    """The (clusters, masks) arrays of GpuBackend.restart (needs no library). ValueError names the
    position of a cluster outside the handle, a cluster named twice, a missing or empty node list
    and a node id outside 1..n_nodes."""
    targets = list(targets)
    if nodes is not None:
        nodes = list(nodes)
        if len(nodes) != len(targets):
            raise ValueError(f"restart: {len(nodes)} node masks for {len(targets)} targets")
    ids_mask = ((1 << (n_nodes + 1)) - 1) & ~1
    cl = np.zeros(len(targets), dtype=np.uint32)
    masks = np.zeros(len(targets), dtype=np.uint16)
    seen = set()
    for i, t in enumerate(targets):
        c = int(t["cluster"] if isinstance(t, dict) else t)
        if not 0 <= c < n_clusters:
            raise ValueError(f"restart: targets[{i}] = {c} is outside the handle's {n_clusters}")
        if c in seen:
            raise ValueError(f"restart: targets[{i}] = {c} is named twice")
        seen.add(c)
        if nodes is not None:
            m = nodes[i]
        elif isinstance(t, dict) and "halted" in t:
            m = t["halted"]
        else:
            raise ValueError(f"restart: targets[{i}] = {c} has no node mask (give `nodes`, or "
                             "select() records, whose halted nodes are taken)")
        if not isinstance(m, (int, np.integer)):
            ids = [int(j) for j in m]
            bad = [j for j in ids if not 1 <= j <= n_nodes]
            if bad:
                raise ValueError(f"restart: nodes[{i}] names node id {bad[0]} outside 1..{n_nodes}")
            m = sum(1 << j for j in set(ids))
        m = int(m)
        if m == 0 or m & ~ids_mask:
            raise ValueError(f"restart: nodes[{i}] = {m:#x} names no node or a node outside "
                             f"ids 1..{n_nodes}")
        cl[i], masks[i] = c, m
    return cl, masks


def check_pack_fits(config, pack, who):
    """What a pack must be to be written into a handle of `config` (restore_cluster's conditions,
    needs no library): the parts cluster, nodes, queues, arenas (and streams when the pack keeps
    commit streams), and the handle's nodes, inbox_cap, log_cap, arena_cap, commit_stream_cap."""
    for name in list(_abi.SCATTER_PARTS) + (["streams"] if pack.SC else []):
        if name not in pack.layout:
            raise ValueError(f"{who} needs the {name!r} part; the pack holds {list(pack.parts)}")
    mine = (config.nodes, config.inbox_cap, config.log_cap,
            config.arena_cap or 4 * config.log_cap, config.commit_stream_cap)
    if mine != (pack.N, pack.Q, pack.L, pack.A, pack.SC):
        raise ValueError(f"{who}: the handle's nodes, inbox_cap, log_cap, arena_cap, "
                         f"commit_stream_cap {mine} are not the pack's "
                         f"{(pack.N, pack.Q, pack.L, pack.A, pack.SC)}")


def check_clone_fits(config, source_config):
    """What two handles must share for a clone between them (needs no library): nodes, inbox_cap,
    log_cap, the effective arena_cap and commit_stream_cap. ValueError names the first that
    differs."""
    def shape(c):
        return {f: (c.arena_cap or 4 * c.log_cap) if f == "arena_cap" else getattr(c, f)
                for f in _abi.CLONE_SHAPE}

    mine, theirs = shape(config), shape(source_config)
    for f in _abi.CLONE_SHAPE:
        if mine[f] != theirs[f]:
            raise ValueError(f"clone: the handles differ in {f}: the target's is {mine[f]}, "
                             f"the source's {theirs[f]}")


def replay_config(config, cluster, **overrides):
    """GpuBackend.replay_config on a bare _abi.Config (needs no library)."""
    if not 0 <= cluster < config.n_clusters:
        raise ValueError(f"cluster {cluster} outside the handle's {config.n_clusters}")
    cfg = {f: getattr(config, f) for f, _ in _abi.Config._fields_}
    cfg.update(n_clusters=1, cluster_offset=config.cluster_offset + cluster, n_devices=1,
               trace_cap=REPLAY_TRACE_CAP, trace_entry_cap=REPLAY_TRACE_ENTRY_CAP)
    for k in overrides:
        if k not in cfg:
            raise TypeError(f"unknown config field {k!r}")
    cfg.update(overrides)
    return cfg
