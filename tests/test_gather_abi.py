"""Cluster packs without a GPU: the ABI extension (raft_gather_*: layouts, exported symbols,
argument checks, the Clojure facade's view), the reference tests/test_gpu_gather.py rests on
(tests/gather_mirror.py), raftsim.ClusterPack over the mirror's bytes of oracle runs, the restore
that raftsim.fork is made of, and the witnesses: the cases the GPU tests run do reach the states a
gather kernel can get wrong."""
import ctypes
import re

import numpy as np
import pytest

import gather_mirror as gm
import helpers
import hostprog
import pairing
import raftsim
from cases import CASES, GPU_CASES, ROUNDTRIP
from hostprog import HEADER, ROOT
from raftsim import ClusterPack, _abi

CLJ = (ROOT / "clojure" / "src" / "raft" / "sim.clj").read_text()
NONE64 = 2 ** 64 - 1


def test_layouts_match_the_c_compiler(tmp_path):
    names = [f"RAFT_GATHER_{k.upper()}" for k in _abi.GATHER_PARTS]
    out = hostprog.c_layout(tmp_path, {"raft_gather_layout_t": _abi.GatherLayout}, [
        'printf("parts' + " %d" * (len(names) + 1) + '\\n", ' + ", ".join(names) + ", RAFT_GATHER_ALL);",
        'printf("records %zu %zu %zu %zu\\n", sizeof(raft_cluster_t), '
        'sizeof(raft_node_t), sizeof(raft_msg_t), sizeof(raft_entry_t));'])
    assert ctypes.sizeof(_abi.GatherLayout) == 104
    off = 0
    for f, t in _abi.GatherLayout._fields_:              # all u64, tiling the structure in order
        assert getattr(_abi.GatherLayout, f).offset == off, f
        assert (t._type_ if hasattr(t, "_length_") else t) is ctypes.c_uint64, f
        off += ctypes.sizeof(t)
    assert off == 104
    bits = [int(x) for x in out[-2].split()[1:]]
    assert bits[:-1] == list(_abi.GATHER_PARTS.values()) == [1 << i for i in range(6)]
    assert bits[-1] == _abi.GATHER_ALL == sum(_abi.GATHER_PARTS.values()) == 63
    assert [int(x) for x in out[-1].split()[1:]] == [
        ctypes.sizeof(t) for t in (_abi.Cluster, _abi.Node, _abi.Msg, _abi.Entry)] == [32, 136, 32, 8]


# Hand-computed: part -> (offset, size); every part starts on the next 16-byte boundary.
#   N = 2, Q = 1, L = 4, A = 9, SC = 0: cluster 32; nodes 2 * 136 = 272; queues 2 * 2 * 1 * 32 = 128;
#   logs 2 * 4 * 8 = 64; arenas 2 * 9 * 8 = 144; streams 0 bytes at the record's end.
#   N = 9, Q = 16, L = 48, A = 101, SC = 8: nodes 9 * 136 = 1224 (padded to 1232); queues 9 * 2 * 16
#   * 32 = 9216; logs 9 * 48 * 8 = 3456; arenas 9 * 101 * 8 = 7272 (padded to 7280); streams 288.
HAND_LAYOUTS = [
    ((2, 1, 4, 9, 0), 63, dict(stride=640, cluster=(0, 32), nodes=(32, 272), queues=(304, 128),
                               logs=(432, 64), arenas=(496, 144), streams=(640, 0))),
    ((9, 16, 48, 101, 8), 63, dict(stride=21504, cluster=(0, 32), nodes=(32, 1224),
                                   queues=(1264, 9216), logs=(10480, 3456), arenas=(13936, 7272),
                                   streams=(21216, 288))),
    ((9, 16, 48, 101, 8), 2 | 16, dict(stride=8512, nodes=(0, 1224), arenas=(1232, 7272))),
    ((9, 16, 48, 101, 8), 32, dict(stride=288, streams=(0, 288))),
    ((2, 1, 4, 9, 0), 32, dict(stride=0, streams=(0, 0))),
    ((2, 1, 4, 0, 0), 16, dict(stride=256, arenas=(0, 256))),       # arena_cap 0: 4 L slots
]


@pytest.mark.parametrize("shape,parts,want", HAND_LAYOUTS)
def test_layout_arithmetic(shape, parts, want):
    got = _abi.gather_layout(*shape, parts)
    assert got == want and list(got) == list(want)      # the parts in bit order
    assert all(v % 16 == 0 for v in [got["stride"]] + [got[k][0] for k in got if k != "stride"])
    # the structure's view: absent parts have offset UINT64_MAX and size 0
    lay = _abi.GatherLayout()
    lay.stride = want["stride"]
    for b, k in enumerate(_abi.GATHER_PARTS):
        lay.off[b], lay.size[b] = want.get(k, (NONE64, 0))
    assert lay.as_dict() == want


def test_library_exports_exactly_the_gather_entry_points():
    assert hostprog.exported(r"raft_gather_\w+") == set(_abi.GATHER_SYMBOLS) == \
        {"raft_gather_layout", "raft_gather_read"}
    assert hostprog.exported("raftsim_diag_gather_ms")
    # the older sets are what they were
    assert hostprog.exported(r"raft_audit_\w+") == set(_abi.AUDIT_SYMBOLS)
    assert hostprog.exported(r"raft_census_\w+") == set(_abi.CENSUS_SYMBOLS)
    assert hostprog.exported(r"raft_viol_\w+") == set(_abi.VIOL_SYMBOLS)
    assert hostprog.exported(r"raft_sim_\w+") == set(_abi.PRODUCT_SYMBOLS)


def test_header_declares_the_gather():
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"\b(raft_gather_\w+)\s*\(", text))) == sorted(_abi.GATHER_SYMBOLS)
    assert "#define RAFT_SIM_ABI_VERSION 2" in text and "#define RAFT_GATHER_ALL 63" in text
    enum = re.search(r"enum raft_gather_part \{(.*?)\};", text, re.S).group(1)
    table = {k.lower(): int(v) for k, v in re.findall(r"RAFT_GATHER_(\w+)\s*= (\d+)", enum)}
    assert table == _abi.GATHER_PARTS and list(table) == list(_abi.GATHER_PARTS)
    for prefix, names in (("raft_sim_", _abi.PRODUCT_SYMBOLS), ("raft_viol_", _abi.VIOL_SYMBOLS),
                          ("raft_census_", _abi.CENSUS_SYMBOLS), ("raft_audit_", _abi.AUDIT_SYMBOLS)):
        assert sorted(set(re.findall(rf"\b({prefix}\w+)\s*\(", text))) == sorted(names), prefix
    # no oracle counterpart: the oracle Backend binds the first table only, and restores all the same
    with helpers.oracle(n_clusters=1) as h:
        assert not hasattr(h, "gather") and hasattr(h, "restore_cluster")
    assert not hasattr(ctypes.CDLL(str(helpers.ORACLE_LIB)), "raft_ref_gather_read")
    # the kernel is part of the build and of its hash
    from raftsim import _build
    assert "raft-simulation_amd/csrc/gather_kernel.hip" in _build.KERNEL_SOURCES


def test_bad_arguments_are_refused_without_a_device():
    lib = ctypes.CDLL(str(raftsim.LIB_PATH))        # loads without a GPU
    fns = _abi.bind(lib, "raft_gather_", sigs=_abi._GATHER_SIGS)
    assert set(fns) == {"layout", "read"}
    last_error = _abi.bind(lib, "raft_sim_")["last_error"]
    lay = _abi.GatherLayout()
    idx = (ctypes.c_uint32 * 4)(0, 1, 2, 3)
    buf = ctypes.create_string_buffer(64)
    assert fns["layout"](None, 63, ctypes.byref(lay)) == -22 and b"null" in last_error()
    assert fns["read"](None, idx, 4, 63, buf, 64) == -22 and b"null sim" in last_error()
    # parts and the pointers are checked before the handle is looked at: a handle that is never
    # dereferenced stands in for a live one
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    for parts in (0, 64, 2 ** 32 - 1):
        assert fns["layout"](fake, parts, ctypes.byref(lay)) == -22, parts
        assert b"RAFT_GATHER_ALL" in last_error()
        assert fns["read"](fake, idx, 4, parts, buf, 64) == -22, parts
        assert b"RAFT_GATHER_ALL" in last_error()
    assert fns["layout"](fake, 63, None) == -22
    assert fns["read"](fake, None, 4, 63, buf, 64) == -22 and b"null cluster list" in last_error()
    assert fns["read"](fake, idx, 4, 63, None, 64) == -22 and b"null output" in last_error()
    ms = ctypes.c_double()
    lib.raftsim_diag_gather_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    assert lib.raftsim_diag_gather_ms(None, ctypes.byref(ms)) == -22


def test_clojure_facade_names_the_entry_points():
    size = lambda name: int(re.search(rf"\(def {name} (\d+)\)", CLJ).group(1))  # noqa: E731
    assert size("gather-layout-size") == ctypes.sizeof(_abi.GatherLayout)
    assert set(re.findall(r'"(raft_gather_\w+)"', CLJ)) == set(_abi.GATHER_SYMBOLS)
    for name in ("(defn gather-layout\n", "(defn gather\n"):
        assert name in CLJ, name
    parts = dict(re.findall(r":([a-z]+) (\d+)", re.search(r"gather-parts\s*\{([^}]*)\}",
                                                          CLJ).group(1)))
    assert {k: int(v) for k, v in parts.items()} == _abi.GATHER_PARTS
    order = re.search(r"gather-part-order\s*\[([^\]]*)\]", CLJ).group(1).split()
    assert [s[1:] for s in order] == list(_abi.GATHER_PARTS)
    # the offsets the facade reads at are the structure's
    assert _abi.GatherLayout.stride.offset == 0 and "(.getLong m 0)" in CLJ
    assert f"(.getLong m (+ {_abi.GatherLayout.off.offset} (* 8 b)))" in CLJ
    assert f"(.getLong m (+ {_abi.GatherLayout.size.offset} (* 8 b)))" in CLJ


def test_python_refusals():
    with pytest.raises(ValueError, match="unknown pack part"):
        raftsim.GpuBackend._mask(("trace",), _abi.GATHER_PARTS, "pack part")
    h = pairing.oracle(dict(ROUNDTRIP, n_clusters=2), threads=8, ticks=100)
    with pytest.raises(ValueError, match="not len"):
        ClusterPack({f: getattr(h.config, f) for f, _ in _abi.Config._fields_}, 0, [0],
                    gm.layout_of(h), np.zeros(3, dtype=np.uint8))
    for missing in ("cluster", "queues", "arenas"):
        pack = gm.pack_of(h, [0, 1], [p for p in gm.PARTS if p != missing])
        with helpers.oracle(**dict(ROUNDTRIP, n_clusters=1)) as one:
            with pytest.raises(ValueError, match=f"'{missing}'"):
                one.restore_cluster(pack, 0)
            assert one.tick == 0 and not one.host_written
        read = {"cluster": lambda p: p.cluster(0), "queues": lambda p: p.queue(0, 1, 0),
                "arenas": lambda p: p.arena(0, 1)}[missing]
        with pytest.raises(ValueError, match=missing):
            read(pack)
    pack = gm.pack_of(h, [0, 1])
    with pytest.raises(IndexError):
        pack.log(2, 1)
    with pytest.raises(IndexError):
        pack.log(0, 6)
    with helpers.oracle(**dict(ROUNDTRIP, n_clusters=1, log_cap=32)) as other:
        with pytest.raises(ValueError, match="log_cap"):
            other.restore_cluster(pack, 0)
    # a stream-keeping config needs the streams
    s = pairing.oracle(dict(ROUNDTRIP, n_clusters=1, commit_stream_cap=4), threads=8, ticks=100)
    with helpers.oracle(**dict(ROUNDTRIP, n_clusters=1, commit_stream_cap=4)) as one:
        with pytest.raises(ValueError, match="'streams'"):
            one.restore_cluster(gm.pack_of(s, [0], gm.PARTS[:-1]), 0)


PACK_CASES = {"arena_odd": dict(CASES["arena_odd"], n_clusters=32),
              "spec_c3": dict(CASES["spec_c3"], n_clusters=32, commit_stream_cap=8)}


@pytest.mark.parametrize("name", list(PACK_CASES))
def test_cluster_pack_over_the_mirror(name, tmp_path):
    cfg = PACK_CASES[name]
    h = pairing.oracle(cfg, threads=8, ticks=6000)
    order = list(range(31, -1, -1)) + [5, 5]
    pack = gm.pack_of(h, order)
    assert len(pack) == 34 and pack.tick == 6000 and pack.parts == gm.PARTS
    assert pack.global_ids == [cfg.get("cluster_offset", 0) + c for c in order]
    assert pack.config["seed"] == cfg["seed"] and pack.layout == gm.layout_of(h)
    raw = h.read_nodes_raw()
    N = cfg["nodes"]
    for i, c in enumerate(order):
        assert pack.cluster(i) == h.read_clusters(c, 1)[0]
        assert pack.node_dicts(i) == h.read_nodes(c, 1)
        assert bytes(pack.nodes[i]) == bytes(raw)[c * N * 136:(c + 1) * N * 136]
        for k in range(1, N + 1):
            assert pack.nodes[i][k - 1].current_term == raw[c * N + k - 1].current_term
            assert pack.log(i, k) == h.log(c, k), (c, k)
            assert pack.arena(i, k) == h.read_arena(c, k), (c, k)
            assert pack.commit_stream(i, k) == h.commit_stream(c, k), (c, k)
            for which in (0, 1):
                assert pack.queue(i, k, which) == h.read_queue(c, k, which), (c, k, which)
    # the views are views: no accessor copied the buffer
    assert np.shares_memory(pack.part(3, "arenas"), pack.data)
    # a subset of the parts holds the same bytes at its own offsets
    sub = gm.pack_of(h, order, ("nodes", "logs"))
    assert sub.parts == ("nodes", "logs") and sub.layout["stride"] < pack.layout["stride"]
    for i in (0, 17, 33):
        for p in sub.parts:
            assert np.array_equal(sub.part(i, p), pack.part(i, p))
    # save / load
    path = pack.save(tmp_path / "pack")
    assert path.endswith("pack.npz")
    back = ClusterPack.load(tmp_path / "pack")
    assert np.array_equal(back.data, pack.data) and back.data.dtype == np.uint8
    assert (back.config, back.tick, back.clusters, back.layout) == \
        (pack.config, pack.tick, pack.clusters, pack.layout)
    assert back.log(2, 3) == pack.log(2, 3)
    with np.load(path, allow_pickle=False) as z:         # loads with pickle refused
        assert set(z.files) == {"data", "clusters", "meta"}


@pytest.mark.parametrize("cfg,t0", [
    (ROUNDTRIP, 15000),
    (dict(CASES["spec_c3"], n_clusters=64, commit_stream_cap=8), 15000),
], ids=["roundtrip", "spec_c3_streams"])
def test_restore_continues_bit_exactly_on_the_oracle(cfg, t0):
    src = pairing.oracle(cfg, threads=8, ticks=t0)
    picks = [0, 31, 63]
    pack = gm.pack_of(src, picks)
    if cfg.get("commit_stream_cap"):
        assert any(pack.commit_stream(i, k) for i in range(3) for k in range(1, 6))
    forks = []
    for i, c in enumerate(picks):
        one = helpers.oracle(**dict(cfg, n_clusters=1, cluster_offset=c))
        one.restore_cluster(pack, i)
        assert one.tick == t0 and one.host_written
        assert one.digest()[0] == src.digest(c, 1)[0], c
        forks.append(one)
    # a restore into cluster 1 of a larger handle (global id 31 there too)
    two = helpers.oracle(**dict(cfg, n_clusters=2, cluster_offset=30))
    two.restore_cluster(pack, 1, cluster=1)
    assert two.digest(1, 1)[0] == src.digest(31, 1)[0] and two.tick == t0
    src.step(8000)
    for one, c in zip(forks, picks):
        one.step(8000)
        assert one.digest()[0] == src.digest(c, 1)[0], c
        for k in range(1, cfg["nodes"] + 1):
            assert one.commit_stream(0, k) == src.commit_stream(c, k)


def test_witnesses_the_gpu_cases_reach_the_states():
    """What a gather kernel can get wrong shows only in states that have it: a log that crosses
    its arena's end, a commit-stream ring that has wrapped, a queue with two messages or more, a
    message with a payload, a full log. The cases of tests/test_gpu_gather.py have them all."""
    seen = {}
    for name, (cfg, ticks) in GPU_CASES.items():
        assert cfg["n_clusters"] <= 96 and 6000 <= ticks <= 20000
        h = pairing.oracle(cfg, threads=8, ticks=ticks)
        N, A, SC = cfg["nodes"], h.config.arena_cap or 4 * h.config.log_cap, \
            h.config.commit_stream_cap
        recs = h.read_nodes()
        msgs = [m for c in range(cfg["n_clusters"]) for k in range(1, N + 1)
                if recs[c * N + k - 1]["req_count"] for m in h.read_queue(c, k, 0)]
        seen[name] = dict(
            log_wrap=sum(r["arena_base"] % A + r["log_len"] > A for r in recs),
            stream_wrap=sum(bool(SC) and r["commit_count"] > SC for r in recs),
            req2=sum(r["req_count"] >= 2 for r in recs),
            res2=sum(r["res_count"] >= 2 for r in recs),
            payload=sum((m[1] >> 16) > 0 for m in msgs),
            full_log=sum(r["log_len"] == cfg.get("log_cap", 64) for r in recs),
            empty_log=sum(r["log_len"] == 0 for r in recs),
            halted=sum(r["fault"] != 0 for r in recs))
    a = seen["arena_odd"]
    assert a["log_wrap"] >= 5 and a["stream_wrap"] >= 50 and a["req2"] >= 3 and a["res2"] >= 3
    assert a["payload"] >= 5 and a["halted"] and a["empty_log"]
    assert seen["spec_c3"]["stream_wrap"] >= 1
    assert seen["burst_arena_odd_n7"]["full_log"] >= 1 and seen["burst_arena_odd_n7"]["res2"] >= 1
