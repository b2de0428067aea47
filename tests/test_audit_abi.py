"""The log audit without a GPU: the ABI extension (raft_audit_*: layouts, exported symbols, argument
checks, the Clojure facade's view) and the reference tests/test_gpu_audit.py rests on,
tests/audit_oracle.py, checked on hand-written logs (one case per class bit and per boundary of
its definition) and on the oracle's populations."""
import ctypes
import re

import pytest

import audit_oracle as ao
import helpers
import hostprog
import raftsim
from cases import CASES
from hostprog import HEADER, ROOT
from raftsim import _abi

CLJ = (ROOT / "clojure" / "src" / "raft" / "sim.clj").read_text()


def test_layouts_match_the_c_compiler(tmp_path):
    structs = {"raft_audit_t": _abi.Audit, "raft_audit_record_t": _abi.AuditRecord}
    names = [f"RAFT_AUD_{k.upper()}" for k in _abi.AUDIT_CLASSES]
    out = hostprog.c_layout(tmp_path, structs, ['printf("classes' + " %d" * (len(names) + 1) + '\\n", '
                                                + ", ".join(names) + ", RAFT_AUD_ALL);"])
    assert ctypes.sizeof(_abi.AuditRecord) == 32
    # all of raft_audit_t is u64: its fields tile it in 8-byte words, in order
    off = 0
    for f, t in _abi.Audit._fields_:
        assert getattr(_abi.Audit, f).offset == off and ctypes.sizeof(t) % 8 == 0, f
        assert (t._type_ if hasattr(t, "_length_") else t) is ctypes.c_uint64, f
        off += ctypes.sizeof(t)
    assert off == ctypes.sizeof(_abi.Audit) == 136
    bits = [int(x) for x in out[-1].split()[1:]]
    assert bits[:-1] == list(_abi.AUDIT_CLASSES.values()) == [1 << i for i in range(5)]
    assert bits[-1] == _abi.AUD_ALL == sum(_abi.AUDIT_CLASSES.values()) == 31
    assert _abi.AUDIT_CLASSES == ao.CLASSES
    assert tuple(f for f, _ in _abi.Audit._fields_[2:]) == ao.SCALARS


def test_library_exports_exactly_the_audit_entry_points():
    assert hostprog.exported(r"raft_audit_\w+") == set(_abi.AUDIT_SYMBOLS) == \
        {"raft_audit_read", "raft_audit_select"}
    assert hostprog.exported("raftsim_diag_audit_ms")
    # the older sets are what they were
    assert hostprog.exported(r"raft_census_\w+") == set(_abi.CENSUS_SYMBOLS)
    assert hostprog.exported(r"raft_sim_\w+") == set(_abi.PRODUCT_SYMBOLS)


def test_header_declares_the_audit():
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"\b(raft_audit_\w+)\s*\(", text))) == sorted(_abi.AUDIT_SYMBOLS)
    assert "#define RAFT_SIM_ABI_VERSION 2" in text and "#define RAFT_AUD_ALL 31" in text
    enum = re.search(r"enum raft_audit_class \{(.*?)\};", text, re.S).group(1)
    table = {k.lower(): int(v) for k, v in re.findall(r"RAFT_AUD_(\w+) = (\d+)", enum)}
    assert table == _abi.AUDIT_CLASSES
    # the audit has no oracle counterpart: the oracle Backend binds the first table only
    with helpers.oracle(n_clusters=1) as h:
        assert not hasattr(h, "audit") and not hasattr(h, "audit_select")
    lib = ctypes.CDLL(str(helpers.ORACLE_LIB))
    assert not hasattr(lib, "raft_ref_audit_read")


def test_bad_arguments_are_refused_without_a_device():
    lib = ctypes.CDLL(str(raftsim.LIB_PATH))        # loads without a GPU
    fns = _abi.bind(lib, "raft_audit_", sigs=_abi._AUDIT_SIGS)
    assert set(fns) == {"read", "select"}
    last_error = _abi.bind(lib, "raft_sim_")["last_error"]
    aud = _abi.Audit()
    buf = (_abi.AuditRecord * 4)()
    assert fns["read"](None, ctypes.byref(aud)) == -22 and b"null" in last_error()
    assert fns["select"](None, 0, 0, 0, buf, 4) == -22 and b"null" in last_error()
    # the masks and the output are checked before the handle is looked at: a handle that is never
    # dereferenced stands in for a live one
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    for any_, all_, none_ in ((32, 0, 0), (0, 32, 0), (0, 0, 32), (0, 2 ** 32 - 1, 0)):
        assert fns["select"](fake, any_, all_, none_, buf, 4) == -22, (any_, all_, none_)
        assert b"RAFT_AUD_ALL" in last_error()
    assert fns["select"](fake, 0, 1 | 16, 16, buf, 4) == -22 and b"share" in last_error()
    assert fns["select"](fake, 1, 0, 0, None, 4) == -22 and b"null output" in last_error()
    assert fns["read"](fake, None) == -22
    ms = ctypes.c_double()
    lib.raftsim_diag_audit_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    assert lib.raftsim_diag_audit_ms(None, ctypes.byref(ms)) == -22


def test_clojure_facade_names_the_entry_points():
    size = lambda name: int(re.search(rf"\(def {name} (\d+)\)", CLJ).group(1))  # noqa: E731
    assert size("audit-size") == ctypes.sizeof(_abi.Audit)
    assert size("audit-record-size") == ctypes.sizeof(_abi.AuditRecord)
    assert size("abi-version") == 2
    assert set(re.findall(r'"(raft_audit_\w+)"', CLJ)) == set(_abi.AUDIT_SYMBOLS)
    for name in ("(defn audit\n", "(defn audit-select"):
        assert name in CLJ, name
    # the offsets the facade reads at are the structures'
    for f, how in (("classes", "getInt"), ("agree_len", "getInt"), ("diverge_index", "getInt"),
                   ("commit_diverge_index", "getInt"), ("order_index", "getInt"),
                   ("diverged", "getShort"), ("commit_diverged", "getShort"),
                   ("len_min", "getInt")):
        off = getattr(_abi.AuditRecord, f).offset
        assert f"(.{how} m (+ r {off}))" in CLJ, f
    assert _abi.AuditRecord.cluster.offset == 0 and "(.getInt m r)" in CLJ
    for f, call in (("by_class", "(a64s 8 5)"), ("entries", "(a64s 72 8)")):
        assert call in CLJ and int(call.split()[1]) == getattr(_abi.Audit, f).offset, f
    scalars = re.search(r"audit-scalars\s*\[([^\]]*)\]", CLJ).group(1).split()
    assert [s[1:].replace("-", "_") for s in scalars] == list(ao.SCALARS)
    classes = dict(re.findall(r":([a-z-]+) (\d+)", re.search(r"audit-classes\s*\{([^}]*)\}",
                                                              CLJ).group(1)))
    assert {k.replace("-", "_"): int(v) for k, v in classes.items()} == _abi.AUDIT_CLASSES
    order = re.search(r"audit-class-order\s*\[([^\]]*)\]", CLJ).group(1).split()
    assert [s[1:].replace("-", "_") for s in order] == list(_abi.AUDIT_CLASSES)


def test_as_dict_shapes():
    a = _abi.Audit()
    a.clusters, a.entries, a.agree_min, a.diverge_index_min = 3, 40, 2, 7
    a.commit_diverge_index_min = 2 ** 64 - 1
    for i in range(8):
        a.by_class[i] = 100 + i
    d = a.as_dict()
    assert list(d["by_class"]) == list(_abi.AUDIT_CLASSES)
    assert list(d["by_class"].values()) == list(range(100, 105))
    assert (d["clusters"], d["entries"], d["agree_min"]) == (3, 40, 2)
    assert d["diverge_index_min"] == 7 and d["commit_diverge_index_min"] is None
    logs = [[(1, 1)], [(1, 1)]]
    recs = ao.records_of(logs, [0, 0], 2)
    assert list(ao.summary_of(recs, logs)) == list(d) == [f for f, _ in _abi.Audit._fields_]
    r = _abi.AuditRecord(5, 1 | 2 | 8, 3, 3, 3, 2 ** 32 - 1, 0b0110, 0b0110, 4)
    assert r.as_dict(3, 10) == dict(cluster=5, global_id=15,
                                    classes=("diverged", "commit_diverged", "term_order"),
                                    agree_len=3, diverge_index=3, commit_diverge_index=3,
                                    order_index=None, diverged=[1, 2], commit_diverged=[1, 2],
                                    len_min=4)
    assert list(r.as_dict(3, 10)) == list(dict(cluster=0, global_id=0, **ao.cluster_audit(logs, [0, 0])))
    with pytest.raises(ValueError):
        raftsim.GpuBackend._audit_mask(("forked",))
    assert raftsim.GpuBackend._audit_mask(("diverged", "identical")) == 17


def seq(*terms, val=7):
    """A log of entries (term, val + position)."""
    return [(t, val + p) for p, t in enumerate(terms)]


# Hand-written clusters: (logs, commits, classes, fields of the record that the case is about).
A, B = seq(1, 1, 2, 2), seq(1, 1, 3, 3)            # differ from position 2 on, in the term
HAND = {
    # equal lengths, no difference: the init state and a replicated log
    "identical_empty": ([[], [], []], [0, 0, 0], ("identical",),
                        dict(agree_len=0, diverge_index=None, len_min=0)),
    "identical_full": ([A, A, A], [4, 2, 0], ("identical",), dict(agree_len=4, len_min=4)),
    # one log longer: a prefix is no divergence, but it is not identical either
    "prefix": ([A, A[:3], A], [9, 9, 9], (), dict(agree_len=3, diverge_index=None, len_min=3)),
    # bit 1 alone: a difference above the commit indices with no equal term after it
    "diverged": ([A, B], [2, 2], ("diverged",),
                 dict(agree_len=2, diverge_index=2, commit_diverge_index=None, diverged=[1, 2],
                      commit_diverged=[])),
    # bit 2: the difference at p = min(commit) - 1 counts, at p = min(commit) it does not
    "commit_at_boundary": ([A, B], [3, 9], ("diverged", "commit_diverged"),
                           dict(commit_diverge_index=2, commit_diverged=[1, 2])),
    "commit_below_boundary": ([A, B], [2, 9], ("diverged",), dict(commit_diverge_index=None)),
    # a commit index beyond the log: only positions in both logs are compared
    "commit_beyond_log": ([A[:2], B], [50, 60], (), dict(agree_len=2, len_min=2)),
    "commit_beyond_log_diverged": ([A[:3], B], [50, 60], ("diverged", "commit_diverged"),
                                   dict(commit_diverge_index=2, len_min=3)),
    # bit 4: the same term with another val at d itself
    "match_at_d": ([seq(1, 2), [(1, 7), (2, 99)]], [0, 0], ("diverged", "match_broken"),
                   dict(diverge_index=1)),
    # ... and an equal term after the difference
    "match_after_d": ([seq(1, 2, 4), seq(1, 3, 4)], [0, 0], ("diverged", "match_broken"),
                      dict(diverge_index=1)),
    # an equal term only before the difference breaks nothing (the control of the two above)
    "match_before_d": ([seq(1, 2, 4), seq(1, 3, 5, 5)], [0, 0], ("diverged",), dict(agree_len=1)),
    # bit 8: an inversion at the last pair only, in one node; the logs agree where both have one
    "order_last_pair": ([seq(1, 2, 3, 2), seq(1, 2, 3)], [0, 0], ("term_order",),
                        dict(order_index=2, agree_len=3)),
    "order_equal_terms_ok": ([seq(1, 1, 1), seq(1, 1, 1)], [0, 0], ("identical",),
                             dict(order_index=None)),
    # three nodes: the masks name the nodes of diverging pairs, the indices are minima over pairs
    "three_nodes": ([A, B, seq(1, 5, 2, 2)], [4, 4, 2],
                    ("diverged", "commit_diverged", "match_broken", "term_order"),
                    dict(agree_len=1, diverge_index=1, commit_diverge_index=1, order_index=1,
                         diverged=[1, 2, 3], commit_diverged=[1, 2, 3])),
    # ... and a pair that differs only above the lower of its commits is left out of bit 2's mask
    "three_nodes_partial": ([A, B, A], [4, 2, 4], ("diverged",),
                            dict(diverged=[1, 2, 3], commit_diverged=[], agree_len=2)),
}


@pytest.mark.parametrize("name", list(HAND))
def test_mirror_on_hand_written_logs(name):
    logs, commits, want, fields = HAND[name]
    got = ao.cluster_audit(logs, commits)
    assert got["classes"] == tuple(k for k in ao.CLASSES if k in want), name
    for k, v in fields.items():
        assert got[k] == v, (name, k)
    # the order of the nodes changes the ids, nothing else
    rev = ao.cluster_audit(logs[::-1], commits[::-1])
    n = len(logs)
    assert rev["classes"] == got["classes"] and rev["agree_len"] == got["agree_len"]
    assert rev["diverged"] == sorted(n + 1 - i for i in got["diverged"])
    # every hand-written bit occurs in some case
    assert {k for c in HAND.values() for k in c[2]} == set(ao.CLASSES)


def test_mirror_summary_and_selection():
    with pytest.raises(ValueError):
        ao.cluster_audit([], [])
    logs = [HAND["diverged"][0][0], HAND["diverged"][0][1], A, A]
    recs = ao.records_of(logs, [3, 3, 0, 0], 2, cluster_offset=40)
    assert [(r["cluster"], r["global_id"]) for r in recs] == [(0, 40), (1, 41)]
    s = ao.summary_of(recs, logs)
    assert s == dict(clusters=2, by_class=dict(diverged=1, commit_diverged=1, match_broken=0,
                                               term_order=0, identical=1),
                     entries=16, agree_sum=6, agree_min=2, agree_max=4, diverged_nodes=2,
                     commit_diverged_nodes=2, diverge_index_min=2, commit_diverge_index_min=2)
    assert ao.select_of(recs, any=("identical", "diverged")) == (2, recs)
    assert ao.select_of(recs, all=("diverged",), none=("match_broken",)) == (1, recs[:1])
    assert ao.select_of(recs, all=("identical", "diverged")) == (0, [])
    assert ao.select_of(recs, limit=1) == (2, recs[:1])


# The populations measured on the oracle (diverged / commit_diverged / match_broken / term_order /
# identical), then entries. The faithful handlers break State Machine Safety (bit 2) in a large
# share of clusters; the Spec-Raft control (spec_c3, spec_arena_odd) diverges above the commit
# index only, as Raft allows: its bits 2 and 4 are empty. Spec-Raft with the vote bug (spec_nolog)
# breaks bit 2 in 2 of 200 clusters.
POPULATIONS = [
    ("arena_odd", 300, (750, 1500), ([192, 97, 112, 1, 29], [276, 185, 182, 1, 4]), (2254, 5020)),
    ("fast_timers", 333, (1000, 2000), ([75, 26, 33, 0, 190], [104, 38, 47, 0, 132]), (418, 582)),
    ("burst_variant_mid_n8", 96, (1250, 2500), ([87, 68, 46, 0, 3], [94, 80, 61, 5, 1]),
     (1985, 2857)),
    ("spec_c3", 200, (20000,), ([6, 0, 0, 0, 54],), (4074,)),
    ("spec_arena_odd", 300, (1500,), ([24, 0, 0, 0, 75],), (6036,)),
    ("spec_nolog", 200, (20000,), ([8, 2, 0, 0, 119],), (14784,)),
]
FAITHFUL = ("arena_odd", "fast_timers", "burst_variant_mid_n8")
CONTROL = ("spec_c3", "spec_arena_odd")


@pytest.mark.parametrize("name,n,ticks,want,entries", POPULATIONS, ids=[p[0] for p in POPULATIONS])
def test_oracle_populations(name, n, ticks, want, entries):
    got = ao.oracle_at(dict(CASES[name], n_clusters=n), ticks)
    for t, w, e, (s, recs) in zip(ticks, want, entries, got):
        assert ao.population(s) == w, (name, t)
        assert s["clusters"] == n == len(recs) and s["entries"] == e
        # identities of the definitions
        assert w[1] <= w[0] and w[2] <= w[0] and w[0] + w[4] <= n
        assert s["diverged_nodes"] >= 2 * w[0] and s["commit_diverged_nodes"] >= 2 * w[1]
        assert (s["diverge_index_min"] is None) == (w[0] == 0)
        assert s["agree_min"] <= s["agree_max"] and s["agree_sum"] <= s["entries"]
        if name in CONTROL:
            assert w[1] == 0 and w[2] == 0 and w[0] > 0, "Spec-Raft diverges above commit only"
    if name == "spec_nolog":
        assert want[0][1] == 2


def test_every_bit_is_populated_by_the_faithful_runs():
    total = [0] * 5
    for name, n, ticks, want, _ in POPULATIONS:
        if name in FAITHFUL:
            for w in want:
                total = [a + b for a, b in zip(total, w)]
    assert all(total), total
    assert dict(zip(ao.CLASSES, total))["term_order"] >= 6      # the rare one: 1 + 5


@pytest.mark.parametrize("nodes,log_cap,arena", [(2, 256, 1024), (5, 256, 1024), (9, 256, 1024),
                                                 (5, 24, 51)])
def test_mirror_on_the_gpu_tests_shapes(nodes, log_cap, arena):
    """The clusters tests/test_gpu_audit.py writes into a handle (tests/audit_shapes.py): the
    mirror gives the classes written down there, every bit occurs, and every index field occurs
    both with a position and without one, so no GPU comparison passes on an empty set."""
    import audit_shapes

    shapes = audit_shapes.shapes(nodes, log_cap)
    assert len(shapes) % 4 and len(shapes) > 32          # no multiple of a wave's clusters
    recs = []
    for c, sh in enumerate(shapes):
        assert len(sh["logs"]) == len(sh["commits"]) == nodes
        assert max(len(x) for x in sh["logs"]) <= log_cap
        got = ao.cluster_audit(sh["logs"], sh["commits"])
        assert got["classes"] == tuple(k for k in ao.CLASSES if k in sh["want"]), sh["name"]
        recs.append(got)
        # the arenas hold the logs where Backend.log looks for them, and poison elsewhere
        for k, b in enumerate(audit_shapes.bases(nodes, arena, c, sh)):
            ar = audit_shapes.arena_of(sh["logs"][k], b, arena, k)
            assert [ar[(b + p) % arena] for p in range(len(sh["logs"][k]))] == sh["logs"][k]
            assert sum(e[0] == audit_shapes.POISON_TERM for e in ar) == arena - len(sh["logs"][k])
    assert {k for r in recs for k in r["classes"]} == set(ao.CLASSES)
    for f in ("diverge_index", "commit_diverge_index", "order_index"):
        assert any(r[f] is None for r in recs) and any(r[f] is not None for r in recs), f
    assert {r["diverge_index"] for r in recs} >= {0, 15, 16, 17, None}
    if log_cap == 256:
        assert {r["diverge_index"] for r in recs} >= {63, 64, 65, 129}
        assert {r["order_index"] for r in recs} >= {15, 63, 128}
        assert {r["len_min"] for r in recs} >= {0, 1, 2, 15, 16, 17, 63, 64, 65, 129, 256}
    # a log that crosses its arena's end at the difference, one before it, and one that never does
    wraps = [[(arena - b % arena) % arena for b in audit_shapes.bases(nodes, arena, c, sh)]
             for c, sh in enumerate(shapes)]
    sh = next(c for c, s in enumerate(shapes) if s["name"] == "diff_term_16")
    if nodes > 2 and audit_shapes.pairs_of(nodes)[0] != (0, nodes - 1):
        sh = next(c for c, s in enumerate(shapes) if s["name"] == "match_step16")
    assert any(0 in w for w in wraps) and all(len(set(w)) > 1 for w in wraps)
    assert max(len(x) for x in shapes[sh]["logs"]) > max(wraps[sh])
