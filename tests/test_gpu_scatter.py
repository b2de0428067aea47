"""Cluster packs written back on the GPU (include/raftsim.h, raft_scatter_write): a pack scattered
into a handle gives the state it was gathered from -- by digest, by a gather of the target, and by
the target's per-node reads (tests/gather_mirror.py) -- and the target then runs on as the source
and the oracle do; raftsim.resume, which continues a whole pack, and raftsim.fan_out, which places
one record at many cluster ids.

The cases of the round trip are tests/test_gather_abi.py's GPU_CASES: its witness test shows on the
oracle that they hold logs that cross the arena's end, wrapped commit-stream rings, queues of two
and more messages, payloads and full logs; they cover odd arena_cap, N = 2 and N = 9, and (c4_n9) a
record large enough for more than one workgroup. Every handle compared by digest has trace_cap 0."""
import ctypes

import numpy as np
import pytest

import gather_mirror as gm
import helpers
import pairing
import raftsim
from cases import CASES, GPU_CASES, ROUNDTRIP
from raftsim import ClusterPack, _abi

pytestmark = pytest.mark.gpu

ALL = _abi.GATHER_ALL
SUMS = ["node_ticks"] + _abi.COUNTER_NAMES


def raw_scatter(g, clusters, records, pack, n_records=None, data=None):
    """raft_scatter_write as the C ABI has it: (return code, message)."""
    idx = (ctypes.c_uint32 * max(1, len(clusters)))(*clusters)
    rec = None if records is None else (ctypes.c_uint32 * max(1, len(records)))(*records)
    data = pack.data if data is None else data
    mask = sum(_abi.GATHER_PARTS[p] for p in pack.parts)
    rc = g._scatter["write"](g._h, idx, rec, len(clusters), mask,
                             data.ctypes.data_as(ctypes.c_void_p),
                             len(pack) if n_records is None else n_records)
    return rc, g._fns["last_error"]().decode()


@pytest.mark.parametrize("name", list(GPU_CASES))
def test_round_trip(name):
    cfg, ticks = GPU_CASES[name]
    C = cfg["n_clusters"]
    ids = list(range(C))
    src, ref = helpers.gpu(**cfg), pairing.oracle(cfg, threads=8)
    src.step(ticks)
    pack = src.gather(ids)
    if name == "c4_n9":                                  # more than one workgroup per pair
        assert pack.layout["stride"] // 32768 >= 2, pack.layout["stride"]
    tgt = raftsim.resume(pack)
    assert (tgt.C, tgt.tick, tgt.config.trace_cap, tgt.config.n_devices) == (C, ticks, 0, 1)
    assert tgt.host_written and tgt.last_scatter_ms() > 0
    assert np.array_equal(tgt.digest(), src.digest())
    assert np.array_equal(tgt.gather(ids).data, pack.data), "a gather of the target"
    assert np.array_equal(gm.pack_bytes(tgt, ids), pack.data), "the target's per-node reads"
    before = src.counters()
    ref.step(ticks + 4000)
    for h in (src, tgt):
        h.step(4000)
    want = ref.digest()
    assert np.array_equal(src.digest(), want) and np.array_equal(tgt.digest(), want)
    after, got = src.counters(), tgt.counters()
    assert {k: after[k] - before[k] for k in SUMS} == {k: got[k] for k in SUMS}
    for h in (src, tgt, ref):
        h.close()


def test_part_of_a_running_handle_permuted():
    cfg = dict(CASES["fast_timers"], n_clusters=3001)
    g, twin = helpers.gpu(**cfg), helpers.gpu(**cfg)
    g.step(2000)
    twin.step(4000)
    touched = list(range(2999, 0, -10))                  # 300 scattered clusters, reversed
    assert len(touched) == 300
    rest = np.setdiff1d(np.arange(3001), touched)
    before = g.digest()
    pack = twin.gather(touched)
    assert g.scatter(pack) == 300
    now, want = g.digest(), twin.digest()
    assert np.array_equal(now[rest], before[rest]), "untouched clusters"
    assert np.array_equal(now[touched], want[touched]) and (now[touched] != before[touched]).all()
    # a handle has one clock: at the twin's, the touched clusters run on as the twin's do
    g.set_tick(4000)
    for h in (g, twin):
        h.step(1000)
    assert np.array_equal(g.digest()[touched], twin.digest()[touched])
    g.close()
    twin.close()


def test_fan_out():
    sim = helpers.gpu(**ROUNDTRIP)
    sim.step(15000)
    c, copies = 31, 300
    pack = sim.gather([c])
    fan = raftsim.fan_out(sim, c, copies)
    assert (fan.C, fan.tick, fan.config.cluster_offset) == (copies, 15000, c)
    assert fan.config.trace_cap == 0
    assert (fan.digest() == sim.digest(c, 1)[0]).all()
    picks = (1, 150, 299)
    refs = []
    for j in picks:                                      # the same state under another global id
        one = helpers.oracle(**dict(ROUNDTRIP, n_clusters=1, cluster_offset=c + j))
        one.restore_cluster(pack, 0)
        one.step(8000)
        refs.append(one.digest()[0])
    for h in (sim, fan):
        h.step(8000)
    d = fan.digest()
    assert d[0] == sim.digest(c, 1)[0], "the copy at the state's own id is its continuation"
    assert [d[j] for j in picks] == refs
    assert len(np.unique(d)) >= 2, "the futures differ"
    # from a pack, by position
    again = raftsim.fan_out(pack, 0, 3)
    again.step(8000)
    assert np.array_equal(again.digest(), d[:3])
    for h in (sim, fan, again):
        h.close()


def test_more_pairs_than_workgroups_in_flight():
    cfg = dict(CASES["n2"], n_clusters=8)
    src = helpers.gpu(**cfg)
    src.step(3000)
    fan = raftsim.fan_out(src, 5, 4097)
    assert fan.C == 4097 and (fan.digest() == src.digest(5, 1)[0]).all()
    src.close()
    fan.close()


def test_shards():
    cfg = dict(CASES["fast_timers"], n_clusters=3001)
    src = helpers.gpu(**cfg)
    src.step(2000)
    inter = [c for t in zip(range(0, 1000), range(1000, 2000), range(2000, 3000)) for c in t][::5]
    inter += [3000, 999, 1000, 1999, 2000, 1]
    assert len(set(inter)) == len(inter)
    pack = src.gather(inter)
    one, three = helpers.gpu(**cfg), helpers.gpu(**cfg, n_devices=3)
    for h in (one, three):
        h.set_tick(2000)
        assert h.scatter(pack) == len(inter)
    assert np.array_equal(three.digest()[inter], src.digest()[inter])
    assert np.array_equal(one.gather(range(3001)).data, three.gather(range(3001)).data)
    # one record to targets on every shard
    far = [0, 999, 1000, 1500, 2000, 3000]
    for h in (one, three):
        assert h.scatter(pack, far, [7] * len(far)) == len(far)
        assert (h.digest()[far] == src.digest(inter[7], 1)[0]).all()
    assert np.array_equal(one.digest(), three.digest())
    for h in (src, one, three):
        h.close()


def test_chunks():
    """tests/test_gpu_gather.py's test_chunks shape with every part: 128 records of 1,485,040 bytes,
    190 MB, three trips through the 64-MiB scratch (45 + 45 + 38 records), the arenas of the first
    and the last cluster and of those around the chunk boundaries marked."""
    g = helpers.gpu(n_clusters=128, nodes=9, log_cap=4096)
    A = 4 * 4096
    stride = g.gather_layout()["stride"]
    per_chunk = (64 << 20) // (stride + 8)
    assert stride == 1485040 and per_chunk == 45
    marked = [0, per_chunk - 1, per_chunk, per_chunk + 1, 2 * per_chunk - 1, 2 * per_chunk, 126, 127]

    def pattern(c, k):
        p = np.arange(A, dtype=np.uint32)
        return np.stack([p * 9 + k + (c << 20), ~p ^ (c * 131 + k)], axis=1).astype(np.uint32)

    for c in marked:
        for k in range(1, 10):
            ar = np.ascontiguousarray(pattern(c, k))
            g._check(g._fns["write_arena"](g._h, c, k, (_abi.Entry * A).from_buffer(ar), A))
    pack = g.gather(range(128))
    assert np.array_equal(pack.part(per_chunk, "arenas").view(np.uint32).reshape(9, A, 2)[8],
                          pattern(per_chunk, 9))
    t = helpers.gpu(n_clusters=128, nodes=9, log_cap=4096)
    assert t.scatter(pack) == 128
    assert np.array_equal(t.gather(range(128)).data, pack.data)
    # a shorter scatter afterwards reuses the scratch
    assert t.scatter(pack, [3, 100], [127, per_chunk]) == 2
    back = t.gather([3, 100, 127])
    for i, r in enumerate((127, per_chunk, 127)):
        assert np.array_equal(back.part(i, "arenas"), pack.part(r, "arenas"))
    g.close()
    t.close()


def test_steady_path_is_earned_again():
    """A C2-shaped handle after three steady launches: certificates are set and the followers'
    draws are owed. The resumed handle gets neither (exact deadlines, no certificate) and runs on as
    the source does, on the steady path again by its second step."""
    cfg = dict(n_clusters=1024, nodes=5, hb=300, el_base=500, el_span=500)
    src = helpers.gpu(**cfg)
    for _ in range(3):
        src.step(10000)
    assert src.diag_last_bails() >= 0                    # the steady path ran
    tgt = raftsim.resume(src.gather(range(1024)))
    assert np.array_equal(tgt.digest(), src.digest())
    for _ in range(2):
        for h in (src, tgt):
            h.step(10000)
        assert np.array_equal(tgt.digest(), src.digest())
    assert tgt.diag_last_bails() >= 0
    src.close()
    tgt.close()


def test_a_queued_client_set_ends_lite():
    cfg = dict(n_clusters=64, nodes=5, hb=300, el_base=500, el_span=500)
    src, ref = helpers.gpu(**cfg), pairing.oracle(cfg, threads=8)
    for h in (src, ref):
        h.step(3000)
        for c, node in ((2, 1), (40, 3)):
            helpers.client_set_into(h, c, node, 700 + c)
    tgt = helpers.gpu(**cfg)                             # a LITE handle until the scatter
    tgt.set_tick(3000)
    assert tgt.scatter(src.gather(range(64))) == 64
    pairing.step(tgt, ref, 3000, "the scatter's target")
    assert tgt.counters()["ev_cs"] >= 2                  # the two client-sets were handled
    for h in (src, ref, tgt):
        h.close()


def test_refusals_that_need_the_config():
    cfg = dict(CASES["fast_timers"], n_clusters=8)
    g, t = helpers.gpu(**cfg), helpers.gpu(**cfg)
    g.step(500)
    t.step(100)
    pack = g.gather(range(8))
    before = t.digest()
    rc, msg = raw_scatter(t, [0, 7, 8, 9], None, pack)
    assert rc == -22 and "clusters[2] = 8" in msg        # the first offending position
    rc, msg = raw_scatter(t, [0, 3, 5, 3, 5], [0, 0, 0, 0, 0], pack)
    assert rc == -22 and "clusters[3] = 3" in msg and "twice" in msg
    rc, msg = raw_scatter(t, [0, 1, 2, 3], [0, 1, 8, 9], pack)
    assert rc == -22 and "records[2] = 8" in msg
    rc, msg = raw_scatter(t, list(range(8)), None, pack, n_records=7)
    assert rc == -22 and "records[7] = 7" in msg
    assert raw_scatter(t, [], [], pack)[0] == 0 and raw_scatter(t, [], None, pack)[0] == 0
    # a corrupted node record, a mis-ordered queue: record 5 of 8; nothing is written
    bad = ClusterPack(pack.config, pack.tick, pack.clusters, pack.layout, pack.data.copy())
    bad.nodes[5][1].log_len = cfg["log_cap"] + 1
    with pytest.raises(helpers.RaftSimError,
                       match=r"records\[5\] = 5: invalid node record \(node 2"):
        t.scatter(bad)
    rc, msg = raw_scatter(t, [6, 1], [0, 5], bad)
    assert rc == -22 and "records[1] = 5" in msg
    assert raw_scatter(t, [6, 1], [0, 4], bad)[0] == 2    # only referenced records are checked
    assert np.array_equal(t.digest()[[6, 1]], g.digest()[[0, 4]])
    before[[6, 1]] = g.digest()[[0, 4]]
    bad = ClusterPack(pack.config, pack.tick, pack.clusters, pack.layout, pack.data.copy())
    q = bad.part(5, "queues").view(np.uint32).reshape(5, 2, bad.Q, 8)
    q[0, 1, 0] = [520, 5 | 2 << 3, 1, 0, 0, 0, 0, 0]
    q[0, 1, 1] = [510, 5 | 3 << 3, 1, 0, 0, 0, 0, 0]
    bad.nodes[5][0].res_count = 2
    with pytest.raises(helpers.RaftSimError, match=r"records\[5\] = 5: invalid message or order"):
        t.scatter(bad)
    bad.nodes[5][0].res_count = bad.Q + 1
    with pytest.raises(helpers.RaftSimError, match=r"records\[5\] = 5: invalid message or order"):
        t.scatter(bad)
    assert np.array_equal(t.digest(), before), "a refused scatter wrote nothing"
    # through Python: ranges, a pack of another shape, a missing part
    with pytest.raises(ValueError, match=r"clusters\[1\] = 8"):
        t.scatter(pack, [0, 8], [0, 1])
    with pytest.raises(ValueError, match=r"records\[0\] = 8"):
        t.scatter(pack, [0], [8])
    with pytest.raises(ValueError, match="2 records for 1 clusters"):
        t.scatter(pack, [0], [1, 2])
    with helpers.gpu(**dict(cfg, log_cap=64)) as other:
        with pytest.raises(ValueError, match="scatter: the handle's nodes.*log_cap"):
            other.scatter(pack)
    with pytest.raises(ValueError, match="needs the 'cluster' part"):
        t.scatter(g.gather([0], parts=("nodes", "queues", "arenas")))
    assert np.array_equal(t.digest(), before)
    g.close()
    t.close()


def test_what_a_scatter_leaves_alone():
    cfg = dict(CASES["fast_timers"], n_clusters=333)
    g, src = helpers.gpu(**cfg), helpers.gpu(**cfg)
    g.step(2000)
    src.step(3000)
    a0 = g.audit()                                       # the audit's records are valid now
    before = g.violations(), g.counters()
    assert before[0][0] > 0 and a0 != src.audit()
    assert g.scatter(src.gather(range(333))) == 333
    assert (g.violations(), g.counters()) == before
    assert g.audit() == src.audit(), "the scatter dropped the audit's records"
    assert np.array_equal(g.digest(), src.digest())
    g.close()
    src.close()
