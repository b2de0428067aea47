"""The expected bytes of a cluster pack, built from a backend's per-node reads (test
infrastructure: the reference of tests/test_gpu_gather.py; runs on oracle handles without a GPU).

Written from the layout's definition (include/raftsim.h, "Cluster packs"), not from the kernel: a
record holds the parts asked for in bit order, each on a 16-byte boundary, padding zero;
  cluster  the raft_cluster_t read_clusters returns (reserved words zero)
  nodes    the N raft_node_t read_nodes returns, byte for byte
  queues   per node REQ then RES: inbox_cap messages, what read_queue returns, then zeros
  logs     per node log_cap entries: entry p is arena slot (arena_base + p) mod arena_cap for
           p < min(log_len, log_cap), then zeros
  arenas   per node what read_arena copies
  streams  per node commit_stream_cap words: what commit_stream returns, then zeros
"""
import ctypes

import numpy as np

from raftsim import _abi

PARTS = tuple(_abi.GATHER_PARTS)


def layout_of(backend, parts=PARTS):
    """The layout of `parts` for the backend's config, computed on the host."""
    c = backend.config
    mask = sum(_abi.GATHER_PARTS[p] for p in set(parts))
    return _abi.gather_layout(c.nodes, c.inbox_cap, c.log_cap, c.arena_cap, c.commit_stream_cap,
                              mask)


def read_arena(backend, c, node_id):
    """The node's raw arena through the backend's read_arena entry point, as an (A, 2) uint32
    array (Backend.read_arena makes a Python tuple of every entry: slow on 16k-slot arenas)."""
    fn = backend._fns["read_arena"]
    A = backend._check(fn(backend._h, c, node_id, None, 0))
    buf = (_abi.Entry * A)()
    backend._check(fn(backend._h, c, node_id, buf, A))
    return np.frombuffer(bytes(buf), dtype=np.uint32).reshape(A, 2)


def cluster_bytes(backend, c, layout):
    """One record: cluster `c` of `backend` in `layout` ({"stride", part: (offset, size)})."""
    cfg = backend.config
    N, Q, L, SC = cfg.nodes, cfg.inbox_cap, cfg.log_cap, cfg.commit_stream_cap
    rec = bytearray(layout["stride"])
    raw = backend.read_nodes_raw(c, 1)
    ids = range(1, N + 1)
    arenas = None
    if "logs" in layout or "arenas" in layout:
        arenas = [read_arena(backend, c, k) for k in ids]

    def put(name, data):
        off, size = layout[name]
        assert len(data) == size, (name, len(data), size)
        rec[off:off + size] = data

    if "cluster" in layout:
        d = backend.read_clusters(c, 1)[0]
        cl = _abi.Cluster()
        cl.hwm_index, cl.hwm_term, cl.hwm_val = d["hwm"]
        cl.client_next, cl.client_count = d["client_next"], d["client_count"]
        put("cluster", bytes(cl))
    if "nodes" in layout:
        put("nodes", bytes(raw))
    if "queues" in layout:
        q = np.zeros((N, 2, Q, 8), dtype=np.uint32)
        for k in ids:
            for which in (0, 1):
                msgs = backend.read_queue(c, k, which)
                assert len(msgs) == (raw[k - 1].res_count if which else raw[k - 1].req_count)
                if msgs:
                    q[k - 1, which, :len(msgs)] = np.asarray(msgs, dtype=np.uint32)
        put("queues", q.tobytes())
    if "logs" in layout:
        lg = np.zeros((N, L, 2), dtype=np.uint32)
        for k in ids:
            n, ar = raw[k - 1], arenas[k - 1]
            m = min(n.log_len, L)
            lg[k - 1, :m] = ar[(n.arena_base + np.arange(m, dtype=np.int64)) % len(ar)]
        put("logs", lg.tobytes())
    if "arenas" in layout:
        put("arenas", b"".join(ar.tobytes() for ar in arenas))
    if "streams" in layout:
        s = np.zeros((N, SC), dtype=np.uint32)
        for k in ids:
            vals = backend.commit_stream(c, k) if SC else []
            assert len(vals) == min(raw[k - 1].commit_count, SC)
            s[k - 1, :len(vals)] = vals
        put("streams", s.tobytes())
    return bytes(rec)


def pack_bytes(backend, clusters, parts=PARTS, layout=None):
    """The bytes raft_gather_read must give for `clusters` (handle-local ids, any order) and
    `parts` (names): a numpy.uint8 array of len(clusters) * stride bytes."""
    layout = layout_of(backend, parts) if layout is None else layout
    assert [k for k in layout if k != "stride"] == [p for p in PARTS if p in set(parts)]
    cache = {}
    out = bytearray()
    for c in clusters:
        if c not in cache:
            cache[c] = cluster_bytes(backend, c, layout)
        out += cache[c]
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def pack_of(backend, clusters, parts=PARTS):
    """A raftsim.ClusterPack over the mirror's bytes (how the CPU tests make packs of oracle
    handles)."""
    from raftsim import ClusterPack
    layout = layout_of(backend, parts)
    cfg = {f: getattr(backend.config, f) for f, _ in _abi.Config._fields_}
    return ClusterPack(cfg, backend.tick, list(clusters), layout,
                       pack_bytes(backend, clusters, parts, layout))


assert ctypes.sizeof(_abi.Node) == 136
