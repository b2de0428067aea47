"""Node restarts without a GPU: the ABI extension (raft_restart_write, raft_restart_where: the
header, the exported symbols, the argument checks that come before a handle is looked at, the
Clojure facade's view), the pure restatement raftsim.restart_record, the package's Philox, and the
list conversion of GpuBackend.restart, which needs no library."""
import ctypes
import re

import numpy as np
import pytest

import helpers
import hostprog
import pyref
import raftsim
from raftsim import _abi, _build

HEADER = (hostprog.ROOT / "include" / "raftsim.h").read_text()
CLJ = (hostprog.ROOT / "clojure" / "src" / "raft" / "sim.clj").read_text()


def test_header_declares_the_restarts():
    assert sorted(set(re.findall(r"\b(raft_restart_\w+)\s*\(", HEADER))) == \
        sorted(_abi.RESTART_SYMBOLS) == ["raft_restart_where", "raft_restart_write"]
    assert "#define RAFT_SIM_ABI_VERSION 2" in HEADER      # an addition
    assert re.search(r"enum raft_restart_mode \{ RAFT_RESTART_AMNESIA = 0, "
                     r"RAFT_RESTART_DURABLE = 1 \};", HEADER)
    assert _abi.RESTART_MODES == {"amnesia": 0, "durable": 1}
    decl = re.search(r"int64_t raft_restart_write\((.*?)\);", HEADER, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == \
        ["sim", "clusters", "nodes", "n", "mode"]
    assert "const uint16_t* nodes" in decl
    decl = re.search(r"int64_t raft_restart_where\((.*?)\);", HEADER, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["sim", "fault_mask", "mode"]
    for name, n_args in (("write", 5), ("where", 3)):
        res, args = _abi._RESTART_SIGS[name]
        assert res is ctypes.c_int64 and len(args) == n_args
    # the fault codes by name are raft_node_t.fault's
    assert _abi.FAULT_CODES == {"running": 0, "ioobe": 1, "npe": 2, "cce": 3, "overflow": 4}
    # the host header is part of the build and of its hash; the kernels live in an existing unit
    assert "raft-simulation_amd/csrc/restart_host.hpp" in _build.KERNEL_SOURCES
    assert len(_build.UNITS) == 9
    units = [(hostprog.ROOT / u).read_text() for u in _build.UNITS]
    for kernel in ("restart_kernel", "restart_where_kernel"):
        assert sum(len(re.findall(rf"\n{kernel}\(", t)) for t in units) == 1, kernel
    scatter_unit = units[[u.rsplit("/", 1)[1].split("_")[0] for u in _build.UNITS].index("scatter")]
    assert "\nrestart_kernel(" in scatter_unit and "\nrestart_where_kernel(" in scatter_unit
    assert sum('#include "restart_host.hpp"' in t for t in units) == 1
    text = (hostprog.CSRC / "restart_host.hpp").read_text()
    includes = re.findall(r"#include [<\"](.*?)[>\"]", text)
    assert includes and not any("hip" in inc for inc in includes)
    assert "first_outside" in text and "first_duplicate" in text
    # one hot-word function, beside hot_clone, called by both kernels' shared lane function
    codec = (hostprog.CSRC / "node_codec.hpp").read_text()
    assert len(re.findall(r"uint32_t hot_restart\(", codec)) == 1
    assert len(re.findall(r"hot_restart\(", scatter_unit)) == 1
    plan = (hostprog.CSRC / "launch_plan.hpp").read_text()
    assert "constexpr uint32_t ON_RESTART = ON_SCATTER;" in plan
    # no oracle counterpart: the oracle's Backend restarts through restart_by_writes
    assert not hasattr(raftsim.Backend, "restart") and hasattr(raftsim.GpuBackend, "restart")
    assert hasattr(raftsim.GpuBackend, "restart_where")
    assert hasattr(raftsim.GpuBackend, "last_restart_ms")


def test_library_exports_exactly_the_restart_entry_points():
    assert hostprog.exported(r"raft_restart_\w+") == set(_abi.RESTART_SYMBOLS)
    assert hostprog.exported("raftsim_diag_restart_ms") == {"raftsim_diag_restart_ms"}


def test_clojure_facade_names_the_entry_points():
    assert set(re.findall(r'"(raft_restart_\w+)"', CLJ)) == set(_abi.RESTART_SYMBOLS)
    assert "(defn restart\n" in CLJ and "(defn restart-where\n" in CLJ


def test_bad_arguments_are_refused_without_a_device():
    lib = ctypes.CDLL(str(raftsim.LIB_PATH))        # loads without a GPU
    fns = _abi.bind(lib, "raft_restart_", sigs=_abi._RESTART_SIGS)
    write, where = fns["write"], fns["where"]
    last_error = _abi.bind(lib, "raft_sim_")["last_error"]
    cl = (ctypes.c_uint32 * 2)(0, 1)
    masks = (ctypes.c_uint16 * 2)(2, 4)
    # the mode, the fault mask and the lists are checked before a handle is looked at: a handle
    # that is never dereferenced stands in for a live one
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert write(None, cl, masks, 2, 0) == -22 and b"null sim" in last_error()
    assert write(None, None, None, 0, 1) == -22 and b"null sim" in last_error()
    assert write(fake, cl, masks, 2, 2) == -22 and b"mode" in last_error()
    assert write(fake, None, masks, 2, 0) == -22 and b"null cluster list" in last_error()
    assert write(fake, cl, None, 2, 1) == -22 and b"null node mask list" in last_error()
    assert where(None, 1, 0) == -22 and b"null sim" in last_error()
    assert where(fake, 30, 2) == -22 and b"mode" in last_error()
    assert where(fake, 0, 0) == -22 and b"fault_mask" in last_error()
    assert where(fake, 32, 1) == -22 and b"fault_mask" in last_error()
    ms = ctypes.c_double()
    lib.raftsim_diag_restart_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    assert lib.raftsim_diag_restart_ms(None, ctypes.byref(ms)) == -22
    assert lib.raftsim_diag_restart_ms(fake, None) == -22


def test_the_packages_philox_passes_the_kat():
    # Random123's known answers for Philox4x32-10 (SIM_SPEC §5) ...
    assert raftsim.philox((0, 0, 0, 0), (0, 0)) == \
        (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert raftsim.philox((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == \
        (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert raftsim.philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
                          (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    # ... and the oracle's own restatement on random counters and keys
    rng = np.random.default_rng(5)
    for _ in range(200):
        w = [int(x) for x in rng.integers(0, 2 ** 32, 6)]
        assert raftsim.philox(w[:4], w[4:]) == pyref.philox(w[:4], w[4:])


def _init_record(N, k, cfg, g):
    """The record of init-node k + 1 with an empty log, as a fresh handle's read_nodes gives it."""
    w = pyref.philox((g, (k + 1) | pyref.INIT << 8, 0, 0), (cfg["seed"] & 0xFFFFFFFF,
                                                           cfg["seed"] >> 32))
    rec = _abi.Node().as_dict(N)
    rec.update(current_term=1, deadline=cfg["el_base"] + ((w[1] * cfg["el_span"]) >> 32),
               trace_hash=0xCBF29CE484222325)
    return rec


@pytest.mark.parametrize("N", [2, 5, 9])
def test_amnesia_at_tick_0_is_the_identity_on_init_node(N):
    cfg = dict(seed=0x1234567890ABCDEF, el_base=500, el_span=700)
    with helpers.oracle(n_clusters=2, nodes=N, cluster_offset=40, **cfg) as h:
        fresh = h.read_nodes(1, 1)                 # the oracle's own init-node, global id 41
    for k in range(N):
        rec = _init_record(N, k, cfg, 41)
        assert rec == fresh[k]
        assert raftsim.restart_record(rec, 0, cfg, 41, "amnesia", node_id=k + 1) == rec
        assert raftsim.restart_record(rec, 0, _abi.Config(**cfg), 41, 0, node_id=k + 1) == rec
        assert raftsim.restart_record(dict(rec, id=k + 1), 0, cfg, 41)["deadline"] == rec["deadline"]


def _busy_record(N, rng):
    """A record with every member set to something a restart would have to clear or keep."""
    rec = _abi.Node().as_dict(N)
    rec.update(role=2, voted_for=N, leader_id=1, fault=int(rng.integers(1, 5)), entries_is_seq=1,
               ls_present=1, votes=6, ls_keys=4, current_term=77, commit_index=9, log_len=11,
               deadline=123, next_index=[5] * N, match_index=[4] * N, last_led_term=70,
               arena_base=30, arena_frontier=44, req_count=3, res_count=2, commit_count=8,
               trace_hash=int(rng.integers(1, 2 ** 63)))
    return rec


@pytest.mark.parametrize("mode", ["amnesia", "durable"])
def test_restart_record_clears_and_keeps(mode):
    rng = np.random.default_rng(11)
    cfg = dict(seed=99, el_base=150, el_span=150)
    N, T, g, k = 5, 31337, 1000, 2
    rec = _busy_record(N, rng)
    before = dict(rec)
    got = raftsim.restart_record(rec, T, cfg, g, mode, node_id=k + 1)
    assert rec == before                                    # pure
    changed = {f for f in rec if got[f] != rec[f]}
    kept_by_durable = {"current_term", "voted_for", "log_len", "arena_base"}
    cleared = {"role", "leader_id", "fault", "entries_is_seq", "ls_present", "votes", "ls_keys",
               "commit_index", "deadline", "next_index", "match_index", "req_count", "res_count"}
    assert changed == (cleared if mode == "durable" else cleared | kept_by_durable)
    for f in cleared - {"deadline", "next_index", "match_index"}:
        assert got[f] == 0, f
    assert got["next_index"] == [0] * N and got["match_index"] == [0] * N
    if mode == "amnesia":
        assert (got["current_term"], got["voted_for"], got["log_len"]) == (1, 0, 0)
        assert got["arena_base"] == got["arena_frontier"] == 44
    # both keep the checker's memory, the trace, the commit stream's count, and clear the fault
    for f in ("commit_count", "last_led_term", "trace_hash", "arena_frontier"):
        assert got[f] == rec[f], f
    assert got["fault"] == 0
    # the deadline: SIM_SPEC §4's INIT draw with the restart tick in the counter's tick word
    w = pyref.philox((g, (k + 1) | pyref.INIT << 8, T, 0), (99, 0))
    assert got["deadline"] == T + 150 + ((w[1] * 150) >> 32) == \
        raftsim.restart_deadline(T, cfg, g, k + 1)
    assert T + 150 <= got["deadline"] < T + 300
    with pytest.raises(ValueError, match="unknown restart mode"):
        raftsim.restart_record(rec, T, cfg, g, "lazarus", node_id=1)


def test_restart_lists_name_the_position():
    sel = [{"cluster": 4, "halted": [1, 3]}, {"cluster": 2, "halted": [5]}]
    cl, masks = raftsim.restart_lists(sel, None, 8, 5)
    assert cl.dtype == np.uint32 and masks.dtype == np.uint16
    assert cl.tolist() == [4, 2] and masks.tolist() == [0b1010, 0b100000]
    assert [m.tolist() for m in raftsim.restart_lists([1, 0], [0b110, [2, 2, 5]], 8, 5)] == \
        [[1, 0], [0b110, 0b100100]]
    assert [m.tolist() for m in raftsim.restart_lists(sel, [[2], 62], 8, 5)] == [[4, 2], [4, 62]]
    assert [m.size for m in raftsim.restart_lists([], None, 8, 5)] == [0, 0]
    for targets, nodes, text in (
            ([1, 8], [2, 2], r"targets\[1\] = 8 is outside"),
            ([1, -1], [2, 2], r"targets\[1\] = -1 is outside"),
            ([3, 1, 3], [2, 2, 2], r"targets\[2\] = 3 is named twice"),
            ([1, 2], [2], "1 node masks for 2 targets"),
            ([1, 2], None, r"targets\[0\] = 1 has no node mask"),
            ([1, 2], [2, 0], r"nodes\[1\] = 0x0 names no node"),
            ([1, 2], [2, []], r"nodes\[1\] = 0x0 names no node"),
            ([1, 2], [3, 2], r"nodes\[0\] = 0x3 names no node or a node outside ids 1..5"),
            ([1, 2], [2, 64], r"nodes\[1\] = 0x40 names"),
            ([1, 2], [[1, 6], 2], r"nodes\[0\] names node id 6 outside 1..5"),
            ([{"cluster": 1, "halted": []}], None, r"nodes\[0\] = 0x0 names no node")):
        with pytest.raises(ValueError, match=text):
            raftsim.restart_lists(targets, nodes, 8, 5)
