"""The state census without a GPU: the ABI extension (raft_census_*: layouts, exported symbols,
argument checks, the Clojure facade's view) and the reference tests/test_gpu_census.py rests on,
tests/census_oracle.py, checked on hand-written node records and on the oracle's populations."""
import ctypes
import re

import pytest

import census_oracle as co
import helpers
import hostprog
import raftsim
from cases import CASES
from hostprog import HEADER, ROOT
from raftsim import _abi

CLJ = (ROOT / "clojure" / "src" / "raft" / "sim.clj").read_text()


def test_layouts_match_the_c_compiler(tmp_path):
    structs = {"raft_census_t": _abi.Census, "raft_cluster_state_t": _abi.ClusterState}
    names = [f"RAFT_CLS_{k.upper()}" for k in _abi.CLUSTER_CLASSES]
    out = hostprog.c_layout(tmp_path, structs, ['printf("classes' + " %d" * (len(names) + 1) + '\\n", '
                                                + ", ".join(names) + ", RAFT_CLS_ALL);"])
    assert ctypes.sizeof(_abi.ClusterState) == 32
    # all of raft_census_t is u64: its fields tile it in 8-byte words, in order
    off = 0
    for f, t in _abi.Census._fields_:
        assert getattr(_abi.Census, f).offset == off and ctypes.sizeof(t) % 8 == 0, f
        assert (t._type_ if hasattr(t, "_length_") else t) is ctypes.c_uint64, f
        off += ctypes.sizeof(t)
    assert off == ctypes.sizeof(_abi.Census) == 464
    bits = [int(x) for x in out[-1].split()[1:]]
    assert bits[:-1] == list(_abi.CLUSTER_CLASSES.values()) == [1 << i for i in range(9)]
    assert bits[-1] == _abi.CLS_ALL == sum(_abi.CLUSTER_CLASSES.values()) == 511
    assert _abi.CLUSTER_CLASSES == co.CLASSES and _abi.MAX_NODES == co.MAX_NODES


def test_library_exports_exactly_the_census_entry_points():
    assert hostprog.exported(r"raft_census_\w+") == set(_abi.CENSUS_SYMBOLS) == \
        {"raft_census_read", "raft_census_select"}
    assert hostprog.exported(r"raft_viol_\w+") == {"raft_viol_read", "raft_viol_clear"}
    assert hostprog.exported(r"raft_sim_\w+") == set(_abi.PRODUCT_SYMBOLS)
    assert hostprog.exported("raftsim_diag_census_ms")


def test_header_declares_the_three_symbol_sets():
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"\b(raft_census_\w+)\s*\(", text))) == \
        sorted(_abi.CENSUS_SYMBOLS)
    assert sorted(set(re.findall(r"\b(raft_viol_\w+)\s*\(", text))) == sorted(_abi.VIOL_SYMBOLS)
    assert sorted(set(re.findall(r"\b(raft_sim_\w+)\s*\(", text))) == sorted(_abi.PRODUCT_SYMBOLS)
    assert "#define RAFT_SIM_ABI_VERSION 2" in text and "#define RAFT_CLS_ALL 511" in text
    assert "no reference counterpart, none in the oracle" in text
    # the header's class table is _abi's, names and bits
    enum = re.search(r"enum raft_cluster_class \{(.*?)\};", text, re.S).group(1)
    table = {k.lower(): int(v) for k, v in re.findall(r"RAFT_CLS_(\w+) = (\d+)", enum)}
    assert table == _abi.CLUSTER_CLASSES
    # the census has no oracle counterpart: the oracle Backend binds the first table only
    with helpers.oracle(n_clusters=1) as h:
        assert not hasattr(h, "census") and not hasattr(h, "select")
    lib = ctypes.CDLL(str(helpers.ORACLE_LIB))
    assert not hasattr(lib, "raft_ref_census_read")


def test_bad_arguments_are_refused_without_a_device():
    lib = ctypes.CDLL(str(raftsim.LIB_PATH))        # loads without a GPU
    fns = _abi.bind(lib, "raft_census_", sigs=_abi._CENSUS_SIGS)
    assert set(fns) == {"read", "select"}
    last_error = _abi.bind(lib, "raft_sim_")["last_error"]
    cen = _abi.Census()
    buf = (_abi.ClusterState * 4)()
    assert fns["read"](None, ctypes.byref(cen)) == -22 and b"null" in last_error()
    assert fns["select"](None, 0, 0, 0, buf, 4) == -22 and b"null" in last_error()
    # the masks and the output are checked before the handle is looked at: a handle that is never
    # dereferenced stands in for a live one
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    for any_, all_, none_ in ((512, 0, 0), (0, 512, 0), (0, 0, 512), (0, 2 ** 32 - 1, 0)):
        assert fns["select"](fake, any_, all_, none_, buf, 4) == -22, (any_, all_, none_)
        assert b"RAFT_CLS_ALL" in last_error()
    assert fns["select"](fake, 0, 2 | 8, 8, buf, 4) == -22 and b"share" in last_error()
    assert fns["select"](fake, 1, 0, 0, None, 4) == -22 and b"null output" in last_error()
    assert fns["read"](fake, None) == -22


def test_clojure_facade_names_the_entry_points():
    size = lambda name: int(re.search(rf"\(def {name} (\d+)\)", CLJ).group(1))  # noqa: E731
    assert size("census-size") == ctypes.sizeof(_abi.Census)
    assert size("cluster-state-size") == ctypes.sizeof(_abi.ClusterState)
    assert size("abi-version") == 2
    assert set(re.findall(r'"(raft_census_\w+)"', CLJ)) == set(_abi.CENSUS_SYMBOLS)
    for name in ("(defn census", "(defn select-clusters"):
        assert name in CLJ, name
    # the offsets the facade reads at are the structures'
    for f, how in (("classes", "getInt"), ("leaders", "getShort"), ("halted", "getShort"),
                   ("term_max", "getInt"), ("term_min", "getInt"), ("commit_max", "getInt"),
                   ("len_max", "getInt"), ("queued", "getInt")):
        off = getattr(_abi.ClusterState, f).offset
        assert f"(.{how} m (+ b {off}))" in CLJ, f
    assert _abi.ClusterState.cluster.offset == 0 and "(.getInt m b)" in CLJ
    for f, call in (("by_class", "(u64s 16 9)"), ("leaders_hist", "(u64s 144 n)"),
                    ("live_hist", "(u64s 224 n)"), ("role_nodes", "(u64s 304 4)"),
                    ("fault_nodes", "(u64s 336 5)"), ("term_min", "(u64s 376 11)")):
        assert call in CLJ and int(call.split()[1]) == getattr(_abi.Census, f).offset, f
    scalars = re.search(r"census-scalars\s*\[([^\]]*)\]", CLJ).group(1).split()
    assert [s[1:].replace("-", "_") for s in scalars] == list(co.SCALARS) == \
        [f for f, _ in _abi.Census._fields_[-11:]]
    classes = dict(re.findall(r":([a-z-]+) (\d+)", re.search(r"cluster-classes\s*\{([^}]*)\}",
                                                              CLJ).group(1)))
    assert {k.replace("-", "_"): int(v) for k, v in classes.items()} == _abi.CLUSTER_CLASSES
    order = re.search(r"class-order\s*\[([^\]]*)\]", CLJ).group(1).split()
    assert [s[1:].replace("-", "_") for s in order] == list(_abi.CLUSTER_CLASSES)


def test_census_as_dict_shapes():
    c = _abi.Census()
    c.clusters, c.nodes, c.term_min, c.hwm_sum = 3, 15, 7, 99
    for i in range(16):
        c.by_class[i] = 100 + i
    for i in range(10):
        c.leaders_hist[i], c.live_hist[i] = i, 10 + i
    d = c.as_dict(5)
    assert list(d["by_class"]) == list(_abi.CLUSTER_CLASSES)
    assert list(d["by_class"].values()) == list(range(100, 109))
    assert d["leaders_hist"] == list(range(6)) and d["live_hist"] == list(range(10, 16))
    assert len(d["role_nodes"]) == 4 and len(d["fault_nodes"]) == 5
    assert (d["clusters"], d["nodes"], d["term_min"], d["hwm_sum"]) == (3, 15, 7, 99)
    assert list(d) == [f for f, _ in _abi.Census._fields_]      # the helper's order too
    one = [node(2, lid=1)] + [node(lid=1) for _ in range(4)]
    assert list(co.census_of(one, [{"hwm": (0, 0, 0)}], 5, 8, 0)) == list(d)
    with pytest.raises(ValueError):
        raftsim.GpuBackend._class_mask(("leaderless",))
    assert raftsim.GpuBackend._class_mask(("no_leader", "settled")) == 257


def node(role=0, fault=0, term=1, lid=0, log_len=0, commit=0, rq=0, rs=0):
    return dict(role=role, fault=fault, current_term=term, leader_id=lid, log_len=log_len,
                commit_index=commit, req_count=rq, res_count=rs)


# One hand-written cluster per class bit at N = 5, log_cap 8: (nodes, the classes it is in).
HAND = {
    "no_leader": ([node() for _ in range(5)], ("no_leader",)),
    "one_leader": ([node(2, term=3, lid=1)] + [node(term=2, lid=1) for _ in range(4)],
                   ("one_leader",)),                                   # a follower's term lags
    "multi_leader": ([node(2, term=3, lid=1), node(2, term=4, lid=2)] + [node(lid=2)] * 3,
                     ("multi_leader",)),
    "halted": ([node(fault=1)] + [node() for _ in range(4)], ("no_leader", "halted")),
    # a halted leader is no leader; three halted of five leave no quorum
    "no_quorum": ([node(2, fault=2, term=5, lid=1), node(fault=3), node(fault=4), node(), node()],
                  ("no_leader", "halted", "no_quorum")),
    "same_term_leaders": ([node(2, term=6, lid=1), node(), node(2, term=6, lid=3), node(),
                           node()], ("multi_leader", "same_term_leaders")),
    # log_len == log_cap on a halted node counts
    "log_full": ([node(fault=4, log_len=8)] + [node(log_len=7) for _ in range(4)],
                 ("no_leader", "halted", "log_full")),
    "candidate": ([node(1, term=2)] + [node() for _ in range(4)], ("no_leader", "candidate")),
    # settled: the halted node's stale term and leader_id do not count
    "settled": ([node(term=9, lid=2), node(2, term=9, lid=2), node(fault=1, term=3, lid=5),
                 node(3, term=9, lid=2), node(term=9, lid=2)],
                ("one_leader", "halted", "settled")),
}


@pytest.mark.parametrize("name", list(HAND))
def test_helper_on_hand_written_clusters(name):
    nodes, want = HAND[name]
    got = co.cluster_state(nodes, 8, 0)
    assert name in got["classes"]
    assert got["classes"] == tuple(k for k in co.CLASSES if k in want), name
    # a halted candidate is no candidate, a halted leader no leader
    dead = [dict(n, fault=1) for n in nodes]
    assert co.cluster_state(dead, 8, 0)["classes"][:3] == ("no_leader", "halted", "no_quorum")


def test_helper_record_fields_and_census():
    nodes = [node(2, term=7, lid=1, log_len=3, commit=2, rq=1, rs=2),
             node(term=7, lid=1, log_len=8, commit=1, rq=3),
             node(fault=2, term=4, lid=3, log_len=1, commit=1),
             node(1, term=8), node(3, term=7, lid=1, rs=5)]
    r = co.cluster_state(nodes, 8, 0)
    assert r == dict(classes=("one_leader", "halted", "log_full", "candidate"), leaders=[1],
                     halted=[3], term_max=8, term_min=4, commit_max=2, len_max=8, queued=11)
    two = nodes + HAND["same_term_leaders"][0]
    cen = co.census_of(two, [{"hwm": (5, 1, 1)}, {"hwm": (2, 1, 1)}], 5, 8, 0)
    assert cen["clusters"] == 2 and cen["nodes"] == 10
    assert cen["by_class"] == dict(no_leader=0, one_leader=1, multi_leader=1, halted=1,
                                   no_quorum=0, same_term_leaders=1, log_full=1, candidate=1,
                                   settled=0)
    assert cen["leaders_hist"] == [0, 1, 1, 0, 0, 0] and cen["live_hist"] == [0, 0, 0, 0, 1, 1]
    assert cen["role_nodes"] == [4, 1, 3, 1] and cen["fault_nodes"] == [9, 0, 1, 0, 0]
    assert (cen["term_min"], cen["term_max"], cen["term_sum"]) == (1, 8, 33 + 15)
    assert (cen["commit_max"], cen["commit_sum"], cen["len_max"], cen["len_sum"]) == (2, 4, 8, 12)
    assert (cen["req_queued"], cen["res_queued"], cen["hwm_max"], cen["hwm_sum"]) == (4, 7, 5, 7)
    recs = co.records_of(two, 5, 8, 0, cluster_offset=40)
    assert [(x["cluster"], x["global_id"]) for x in recs] == [(0, 40), (1, 41)]
    assert co.select_of(recs, any=("multi_leader", "candidate")) == (2, recs)
    assert co.select_of(recs, all=("halted", "log_full"), none=("settled",)) == (1, recs[:1])
    assert co.select_of(recs, any=("halted",), all=("multi_leader",)) == (0, [])
    assert co.select_of(recs, limit=1) == (2, recs[:1])


def test_helper_spec_quorum_at_even_n():
    """N = 4 with two live nodes: a quorum under the faithful (N+1)>>1 = 2, none under Spec-Raft's
    N/2+1 = 3; at odd N both give the same."""
    nodes = [node(), node(), node(fault=1), node(fault=1)]
    assert "no_quorum" not in co.cluster_state(nodes, 8, 0)["classes"]
    assert "no_quorum" not in co.cluster_state(nodes, 8, 1)["classes"]      # the vote variant
    assert "no_quorum" in co.cluster_state(nodes, 8, 2)["classes"]
    assert "no_quorum" in co.cluster_state(nodes, 8, 3)["classes"]
    assert [co.quorum(n, 0) for n in range(2, 10)] == [1, 2, 2, 3, 3, 4, 4, 5]
    assert [co.quorum(n, 2) for n in range(2, 10)] == [2, 2, 3, 3, 4, 4, 5, 5]


# The populations the GPU tests run on, measured on the oracle (no / one / multi / halted / noq /
# same / full / cand / settled): every class occurs, so no GPU comparison passes on empty sets.
POPULATIONS = [
    ("arena_odd", 4133, (750, 1500), ([489, 3617, 27, 1025, 525, 1, 1, 556, 3480],
                                      [1566, 2557, 10, 2957, 2320, 0, 322, 1586, 2497])),
    ("c5_variant", 3001, (4500, 9000), ([3001, 0, 0, 0, 0, 0, 0, 0, 0],
                                        [701, 2296, 4, 0, 0, 4, 0, 160, 1601])),
    ("fast_timers", 333, (2000,), ([306, 26, 1, 238, 113, 1, 0, 319, 10],)),
    ("n2", 333, (20000,), ([111, 222, 0, 0, 0, 0, 0, 61, 218],)),
    ("n3", 333, (20000,), ([23, 305, 5, 3, 0, 1, 0, 28, 291],)),
    ("n4", 333, (20000,), ([3, 326, 4, 4, 0, 0, 0, 4, 315],)),
    ("n6", 333, (20000,), ([11, 316, 6, 11, 0, 0, 0, 13, 297],)),
    ("burst_faults_mid_n7", 96, (5000,), ([86, 10, 0, 87, 82, 0, 0, 89, 7],)),
    ("burst_variant_mid_n8", 96, (2500,), ([10, 83, 3, 94, 86, 0, 0, 13, 76],)),
    ("burst_faults_mid_n9", 96, (5000,), ([87, 9, 0, 88, 87, 0, 0, 92, 4],)),
    ("lite_n3", 333, (3000,), ([0, 333, 0, 0, 0, 0, 0, 0, 333],)),
    ("lite_n4", 333, (12000,), ([0, 333, 0, 0, 0, 0, 0, 0, 333],)),
    ("lite_elections", 333, (6000,), ([0, 331, 2, 0, 0, 0, 0, 2, 329],)),
]


@pytest.mark.parametrize("name,n,ticks,want", POPULATIONS, ids=[p[0] for p in POPULATIONS])
def test_oracle_populations(name, n, ticks, want):
    got = co.oracle_at(dict(CASES[name], n_clusters=n), ticks)
    for t, w, (cen, recs) in zip(ticks, want, got):
        assert co.population(cen) == w, (name, t)
        assert cen["clusters"] == n == len(recs)
        # the identities the GPU census is held to hold for the reference
        assert sum(cen["leaders_hist"]) == sum(cen["live_hist"]) == n
        assert sum(w[:3]) == n and sum(cen["fault_nodes"]) == cen["nodes"]
        assert sum(cen["role_nodes"]) == cen["nodes"] - sum(cen["fault_nodes"][1:])
