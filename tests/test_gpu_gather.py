"""Cluster packs on the GPU (include/raftsim.h, "Cluster packs"): raft_gather_read's bytes against
tests/gather_mirror.py, which builds them from the per-node reads of the same handle and of an
oracle handle of the same config and ticks; the list handling, the chunks, that the call only
reads; and raftsim.fork, which continues one packed cluster bit-exactly.

The cases and ticks of the parity test are tests/test_gather_abi.py's GPU_CASES: its witness test
shows on the oracle that they hold logs that cross the arena's end, wrapped commit-stream rings,
queues of two and more messages, payloads and full logs."""
import ctypes

import numpy as np
import pytest

import gather_mirror as gm
import helpers
import pairing
import raftsim
import viol_oracle
from cases import CASES, GPU_CASES, ROUNDTRIP
from raftsim import ClusterPack, _abi

pytestmark = pytest.mark.gpu

ALL = _abi.GATHER_ALL
BIT = _abi.GATHER_PARTS
NONE64 = 2 ** 64 - 1


def raw_gather(g, ids, mask, cap=None):
    """raft_gather_layout and raft_gather_read as the C ABI has them: (layout dict, bytes)."""
    lay = _abi.GatherLayout()
    assert g._gather["layout"](g._h, mask, ctypes.byref(lay)) == 0
    idx = (ctypes.c_uint32 * max(1, len(ids)))(*ids)
    n = len(ids) * lay.stride
    out = np.full(n + 16, 0xA5, dtype=np.uint8)          # a guard behind the records
    got = g._gather["read"](g._h, idx, len(ids), mask, out.ctypes.data_as(ctypes.c_void_p),
                            n if cap is None else cap)
    assert got == n, (got, g._fns["last_error"]())
    assert (out[n:] == 0xA5).all()
    return lay.as_dict(), out[:n]


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_every_part_equals_the_mirror(name):
    cfg, ticks = GPU_CASES[name]
    C = cfg["n_clusters"]
    g, ref = helpers.gpu(**cfg), pairing.oracle(cfg, threads=8, ticks=ticks)
    g.step(ticks)
    ids = list(range(C))
    pack = g.gather(ids)
    assert pack.parts == gm.PARTS and pack.tick == ticks and pack.clusters == ids
    assert pack.layout == gm.layout_of(g) == g.gather_layout()
    assert pack.layout["stride"] % 16 == 0
    assert np.array_equal(pack.data, gm.pack_bytes(g, ids)), "the handle's own reads"
    assert np.array_equal(pack.data, gm.pack_bytes(ref, ids)), "the oracle's reads"
    assert g.last_gather_ms() > 0
    # each part alone, and a pair: the same bytes at the layout's offsets, nothing else
    full = pack.data.reshape(C, -1)
    for mask in [b for b in BIT.values()] + [BIT["cluster"] | BIT["logs"]]:
        lay, data = raw_gather(g, ids, mask)
        names = [k for k, b in BIT.items() if mask & b]
        assert [k for k in lay if k != "stride"] == names
        assert lay == _abi.gather_layout(g.N, g.config.inbox_cap, g.config.log_cap,
                                         g.config.arena_cap, g.config.commit_stream_cap, mask)
        rows = data.reshape(C, -1) if lay["stride"] else data.reshape(C, 0)
        covered = np.zeros(lay["stride"], dtype=bool)
        for k in names:
            off, size = lay[k]
            foff = pack.layout[k][0]
            assert np.array_equal(rows[:, off:off + size], full[:, foff:foff + size]), (mask, k)
            covered[off:off + size] = True
        assert not rows[:, ~covered].any(), "padding is zero"
    # the accessors over the device's bytes are the handle's reads
    for c in (0, C // 2, C - 1):
        assert pack.cluster(c) == g.read_clusters(c, 1)[0]
        assert pack.node_dicts(c) == g.read_nodes(c, 1)
        for k in range(1, g.N + 1):
            assert pack.log(c, k) == g.log(c, k)
            assert pack.commit_stream(c, k) == g.commit_stream(c, k)
            assert [pack.queue(c, k, w) for w in (0, 1)] == [g.read_queue(c, k, w) for w in (0, 1)]
    g.close()


def test_owed_draws_are_resolved_and_certificates_stay():
    """A C2-shaped handle after three steady launches: the followers' deadlines are owed draws
    (FL_DRAW), which the NODES part resolves as read_nodes does; the next launch bails what a twin
    that never gathered bails."""
    cfg = dict(n_clusters=1024, nodes=5, hb=300, el_base=500, el_span=500)
    g, twin = helpers.gpu(**cfg), helpers.gpu(**cfg)
    for h in (g, twin):
        for _ in range(3):
            h.step(10000)
    assert g.diag_last_bails() >= 0                      # the steady path ran
    lay, data = raw_gather(g, list(range(1024)), BIT["nodes"])
    assert lay == dict(stride=688, nodes=(0, 680))
    want = np.frombuffer(bytes(g.read_nodes_raw()), dtype=np.uint8).reshape(1024, 680)
    assert np.array_equal(data.reshape(1024, 688)[:, :680], want)
    assert not data.reshape(1024, 688)[:, 680:].any()
    # the deadlines are draws, not the stored lower bounds: they spread over the election span
    dl = np.array([n.deadline for n in g.read_nodes_raw()]).reshape(1024, 5)
    assert len(np.unique(dl % 500)) > 100
    assert np.array_equal(g.gather(range(1024)).data, gm.pack_bytes(g, range(1024)))
    for h in (g, twin):
        h.step(10000)
    assert g.diag_last_bails() == twin.diag_last_bails() >= 0
    assert np.array_equal(g.digest(), twin.digest()) and g.counters() == twin.counters()
    g.close()
    twin.close()


def test_list_handling_and_shards():
    cfg = dict(CASES["fast_timers"], n_clusters=3001)
    one, three = helpers.gpu(**cfg), helpers.gpu(**cfg, n_devices=3)
    for h in (one, three):
        h.step(2000)
    C = 3001
    full = one.gather(range(C)).data.reshape(C, -1)
    # reversed, with duplicates, both ends
    ids = list(range(C - 1, -1, -7)) + [0, C - 1, 0, 1500, 1500]
    assert 0 in ids and C - 1 in ids
    p = one.gather(ids)
    assert np.array_equal(p.data.reshape(len(ids), -1), full[ids])
    # one cluster, none
    assert np.array_equal(one.gather([C - 1]).data, full[C - 1])
    empty = one.gather([])
    assert len(empty) == 0 and empty.data.size == 0
    lay, data = raw_gather(one, [], ALL)
    assert data.size == 0
    # records of selections are accepted, and a limit
    total, recs = one.audit_select(any=("diverged",))
    assert total > 10
    p = one.gather(recs, parts=("logs",), limit=10)
    assert p.clusters == [r["cluster"] for r in recs[:10]] and p.parts == ("nodes", "logs")
    assert [p.log(i, 1) for i in range(10)] == [one.log(r["cluster"], 1) for r in recs[:10]]
    # three shards on the one GPU (1000 / 1000 / 1001 clusters): a list that interleaves them
    inter = [c for t in zip(range(0, 1000), range(1000, 2000), range(2000, 3000)) for c in t][::5]
    inter += [3000, 999, 1000, 1999, 2000, 0]
    q = three.gather(inter)
    assert np.array_equal(q.data.reshape(len(inter), -1), full[inter])
    # ... and lists a shard holds a consecutive run of (copied straight into the caller's buffer)
    for ids in (list(range(990, 1010)), list(range(2500, 3001)), [1000]):
        assert np.array_equal(three.gather(ids).data.reshape(len(ids), -1), full[ids])
    assert np.array_equal(three.gather([1, 2001, 1001]).data,
                          gm.pack_bytes(three, [1, 2001, 1001]))
    one.close()
    three.close()


def test_refusals_that_need_the_config():
    g = helpers.gpu(**dict(CASES["fast_timers"], n_clusters=8))
    read, err = g._gather["read"], g._fns["last_error"]
    lay = g.gather_layout()
    buf = np.zeros(8 * lay["stride"], dtype=np.uint8)
    out = buf.ctypes.data_as(ctypes.c_void_p)
    idx = (ctypes.c_uint32 * 4)(0, 7, 8, 9)
    assert read(g._h, idx, 4, ALL, out, buf.size) == -22
    assert b"clusters[2] = 8" in err()                   # the first offending position
    assert read(g._h, idx, 2, ALL, out, 2 * lay["stride"] - 1) == -34 and b"cap_bytes" in err()
    assert read(g._h, idx, 2, ALL, out, 2 * lay["stride"]) == 2 * lay["stride"]
    assert read(g._h, idx, 0, ALL, None, 0) == 0 and read(g._h, None, 0, ALL, None, 0) == 0
    assert not buf[2 * lay["stride"]:].any()
    # the layout through the C call: absent parts are UINT64_MAX
    c = _abi.GatherLayout()
    assert g._gather["layout"](g._h, BIT["nodes"] | BIT["arenas"], ctypes.byref(c)) == 0
    assert [c.off[b] == NONE64 for b in range(6)] == [True, False, True, True, False, True]
    assert [c.size[b] for b in (0, 2, 3, 5)] == [0, 0, 0, 0] and c.stride % 16 == 0
    assert g._gather["layout"](g._h, 64, ctypes.byref(c)) == -22
    with pytest.raises(ValueError, match=r"clusters\[1\] = 8"):
        g.gather([0, 8])
    with pytest.raises(ValueError, match="unknown pack part"):
        g.gather([0], parts=("trace",))
    g.close()


def test_chunks():
    """ARENAS of 128 clusters of nine 16,384-slot arenas: 151 MB, three trips through the 64-MiB
    scratch (56 + 56 + 16 records). A pattern written into the arenas of the first and the last
    cluster and of those around the chunk boundaries comes back; all the others are zero."""
    g = helpers.gpu(n_clusters=128, nodes=9, log_cap=4096)
    A = 4 * 4096
    lay = g.gather_layout(("nodes", "arenas"))
    per_chunk = (64 << 20) // (lay["stride"] + 8)
    assert per_chunk == 56 and lay["stride"] * 128 > 2 * (64 << 20)
    marked = [0, per_chunk - 1, per_chunk, per_chunk + 1, 2 * per_chunk - 1, 2 * per_chunk, 126, 127]

    def pattern(c, k):
        p = np.arange(A, dtype=np.uint32)
        return np.stack([p * 9 + k + (c << 20), ~p ^ (c * 131 + k)], axis=1).astype(np.uint32)

    for c in marked:
        for k in range(1, 10):
            ar = np.ascontiguousarray(pattern(c, k))
            g._check(g._fns["write_arena"](g._h, c, k, (_abi.Entry * A).from_buffer(ar), A))
    pack = g.gather(range(128), parts=("arenas",))
    assert pack.parts == ("nodes", "arenas") and pack.data.size == 128 * lay["stride"]
    for c in range(128):
        got = pack.part(c, "arenas").view(np.uint32).reshape(9, A, 2)
        if c in marked:
            for k in range(1, 10):
                assert np.array_equal(got[k - 1], pattern(c, k)), (c, k)
        else:
            assert not got.any(), c
        assert pack.nodes[c][0].log_len == 0 and pack.nodes[c][8].deadline >= 5000
    # a shorter list afterwards reuses the scratch
    again = g.gather([127, 56], parts=("arenas",))
    assert np.array_equal(again.part(0, "arenas"), pack.part(127, "arenas"))
    assert np.array_equal(again.part(1, "arenas"), pack.part(56, "arenas"))
    g.close()


def test_read_only_and_stream_ordered():
    cfg = dict(CASES["fast_timers"], n_clusters=333)
    g = helpers.gpu(**cfg)
    g.step(2000)
    before = g.digest(), g.counters(), g.violations(), g.audit()
    want = g.gather(range(333)).data
    after = g.digest(), g.counters(), g.violations(), g.audit()
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    assert np.array_equal(g.gather(range(333)).data, want)      # bitwise the same answer
    g.close()
    # step_async with no sync: the gather waits for the steps
    for extra in (dict(), dict(ticks_per_launch=37, schedule=1)):
        g = helpers.gpu(**cfg, **extra)
        for _ in range(4):
            g.step_async(500)
        first = g.gather(range(333))
        g.sync()
        assert first.tick == 2000 and np.array_equal(first.data, want), extra
        assert np.array_equal(g.gather(range(333)).data, want), extra
        g.close()


def test_the_audits_records_stay_valid():
    """A gather between two audit() calls: the second finds its records valid and runs no pass
    (its device time is that of an audit() right after an audit(), not that of the pass)."""
    g = helpers.gpu(**CASES["c4_n9_bursts"])
    g.step(20000)                                        # through the second and third client burst
    a0 = g.audit()
    g.step(0)                                            # a step clears the flag
    assert g.audit() == a0
    ms_pass = g.last_audit_ms()
    assert g.audit() == a0
    ms_valid = g.last_audit_ms()
    g.gather(range(0, 256, 3))
    assert g.audit() == a0
    ms_after = g.last_audit_ms()
    print(f"audit of {a0['entries']} entries: pass {ms_pass:.4f} ms, valid {ms_valid:.4f} ms, "
          f"after a gather {ms_after:.4f} ms")
    assert a0["entries"] > 256 * 9 * 100                 # long logs: the pass walks megabytes
    assert ms_valid < ms_pass / 4, (ms_valid, ms_pass)
    assert ms_after < ms_pass / 4, (ms_after, ms_pass)
    g.close()


PICKS = (0, 31, 63)


def test_fork_continues_bit_exactly(tmp_path):
    sim = helpers.gpu(**ROUNDTRIP)
    sim.step(15000)
    direct = [raftsim.fork(sim, c, trace_cap=0, trace_entry_cap=0) for c in PICKS]
    pack = sim.gather(PICKS)
    path = pack.save(tmp_path / "picked")
    loaded = ClusterPack.load(path)
    assert np.array_equal(loaded.data, pack.data) and loaded.clusters == list(PICKS)
    saved = [raftsim.fork(loaded, i, trace_cap=0, trace_entry_cap=0) for i in range(3)]
    for forks in (direct, saved):
        for f, c in zip(forks, PICKS):
            assert f.C == 1 and f.tick == 15000 and f.config.cluster_offset == c
            assert f.digest()[0] == sim.digest(c, 1)[0], c
    sim.step(8000)
    for forks in (direct, saved):
        for f, c in zip(forks, PICKS):
            f.step(8000)
            assert f.digest()[0] == sim.digest(c, 1)[0], c
            f.close()
    with pytest.raises(ValueError, match="outside the pack"):
        raftsim.fork(loaded, 3)
    sim.close()


def test_fork_works_where_replay_refuses():
    sim = helpers.gpu(**ROUNDTRIP)
    sim.step(3000)
    q = sim.read_queue(5, 2, 1)
    sim.write_queue(5, 2, 1, q)
    assert sim.host_written
    with pytest.raises(helpers.RaftSimError, match="written by the host"):
        raftsim.replay(sim, 5)
    f = raftsim.fork(sim, 5, trace_cap=0, trace_entry_cap=0)
    assert f.digest()[0] == sim.digest(5, 1)[0]
    sim.step(4000)
    f.step(4000)
    assert f.digest()[0] == sim.digest(5, 1)[0]
    f.close()
    sim.close()


def test_traced_fork_reports_the_events_of_the_replay():
    """A traced fork at tick 5000 stepped to 20000 records, per node, the events a replay from
    init-node records from tick 5000 on (seq and entries_seq start over in the fork), and its
    violation record is the cluster's when that cluster first violated after the fork."""
    n, t0, t1 = 48, 5000, 20000
    cfg = dict(CASES["fast_timers"], n_clusters=n)
    at_fork, at_end = viol_oracle.expected_records(cfg, n, (t0, t1))
    late = [c for c in sorted(at_end) if c not in at_fork]
    assert late and all(at_end[c][0] >= t0 for c in late)
    c = late[0]
    sim = helpers.gpu(**cfg)
    sim.step(t0)
    f = raftsim.fork(sim, c)
    assert f.config.trace_cap == 4096 and f.tick == t0 and f.violations() == (0, [])
    f.step(t1 - t0)
    r = raftsim.replay(sim, c, ticks=t1)
    sim.step(t1 - t0)
    assert sim.violations()[1] == viol_oracle.as_records(at_end)
    skip = ("seq", "entries_seq")
    events = 0
    for k in range(1, 6):
        want = [e for e in r.trace(0, k) if e["tick"] >= t0]
        got = f.trace(0, k)
        assert len(got) == len(want) and len(want) < 4096, k
        assert [e["seq"] for e in got] == list(range(len(got)))
        for a, b in zip(got, want):
            assert {x: v for x, v in a.items() if x not in skip} == \
                {x: v for x, v in b.items() if x not in skip}, (k, a, b)
        events += len(got)
    assert events > 100                                  # the comparison was of something
    first, counts = at_end[c]
    rec = dict(cluster=0, global_id=c, first_tick=first,
               kinds=tuple(k for k, v in zip(viol_oracle.KINDS, counts) if v))
    rec.update(zip(viol_oracle.KINDS, counts))
    assert f.violations() == (1, [rec])
    for h in (f, r, sim):
        h.close()
