"""Cluster clones without a GPU: the ABI extension (raft_clone_write: the header, the exported
symbols, the argument checks that come before a handle is looked at, the Clojure facade's view),
raftsim.split_plan, which needs no library, and the config check of GpuBackend.clone."""
import ctypes
import re

import pytest

import helpers
import hostprog
import raftsim
from raftsim import _abi, _build

HEADER = (hostprog.ROOT / "include" / "raftsim.h").read_text()
CLJ = (hostprog.ROOT / "clojure" / "src" / "raft" / "sim.clj").read_text()


def test_header_declares_the_clone():
    assert sorted(set(re.findall(r"\b(raft_clone_\w+)\s*\(", HEADER))) == \
        sorted(_abi.CLONE_SYMBOLS) == ["raft_clone_write"]
    assert "#define RAFT_SIM_ABI_VERSION 2" in HEADER      # an addition
    decl = re.search(r"int64_t raft_clone_write\((.*?)\);", HEADER, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == \
        ["dst", "targets", "src", "sources", "n"]
    res, args = _abi._CLONE_SIGS["write"]
    assert res is ctypes.c_int64 and len(args) == 5
    assert "Cluster clones" in HEADER and "EXDEV" in HEADER
    # the host header is part of the build and of its hash; the kernel lives in an existing unit
    assert "raft-simulation_amd/csrc/clone_host.hpp" in _build.KERNEL_SOURCES
    assert len(_build.UNITS) == 9
    units = [(hostprog.ROOT / u).read_text() for u in _build.UNITS]
    assert sum("void clone_kernel(" in t or "\nclone_kernel(" in t for t in units) == 1
    assert sum('#include "clone_host.hpp"' in t for t in units) == 1
    includes = re.findall(r"#include [<\"](.*?)[>\"]", (hostprog.CSRC / "clone_host.hpp").read_text())
    assert includes and not any("hip" in inc for inc in includes)
    # no oracle counterpart
    with helpers.oracle(n_clusters=1) as h:
        assert not hasattr(h, "clone") and hasattr(h, "restore_cluster")
    assert not hasattr(raftsim.Backend, "clone") and hasattr(raftsim.GpuBackend, "clone")


def test_library_exports_exactly_the_clone_entry_point():
    assert hostprog.exported(r"raft_clone_\w+") == set(_abi.CLONE_SYMBOLS)
    assert hostprog.exported("raftsim_diag_clone_ms") == {"raftsim_diag_clone_ms"}


def test_clojure_facade_names_the_entry_point():
    assert set(re.findall(r'"(raft_clone_\w+)"', CLJ)) == set(_abi.CLONE_SYMBOLS)
    assert "(defn clone\n" in CLJ


def test_bad_arguments_are_refused_without_a_device():
    lib = ctypes.CDLL(str(raftsim.LIB_PATH))        # loads without a GPU
    write = _abi.bind(lib, "raft_clone_", sigs=_abi._CLONE_SIGS)["write"]
    last_error = _abi.bind(lib, "raft_sim_")["last_error"]
    idx = (ctypes.c_uint32 * 4)(0, 1, 2, 3)
    # the handles and the lists are checked before a handle is looked at: a handle that is never
    # dereferenced stands in for a live one
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert write(None, idx, fake, idx, 4) == -22 and b"null sim" in last_error()
    assert write(fake, idx, None, idx, 4) == -22 and b"null sim" in last_error()
    assert write(None, None, None, None, 0) == -22 and b"null sim" in last_error()
    assert write(fake, None, fake, idx, 4) == -22 and b"null target list" in last_error()
    assert write(fake, idx, fake, None, 4) == -22 and b"null source list" in last_error()
    ms = ctypes.c_double()
    lib.raftsim_diag_clone_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    assert lib.raftsim_diag_clone_ms(None, ctypes.byref(ms)) == -22
    assert lib.raftsim_diag_clone_ms(fake, None) == -22


def test_split_plan():
    assert raftsim.split_plan([7], []) == ([], [])
    assert raftsim.split_plan([7, 9], [1, 2, 3, 4, 5]) == ([7, 9, 7, 9, 7], [1, 2, 3, 4, 5])
    assert raftsim.split_plan([3, 1, 2], [9, 8]) == ([3, 1], [9, 8])
    # the record dicts the queries return
    recs = [{"cluster": 4, "classes": ()}, {"cluster": 6}]
    assert raftsim.split_plan(recs, [{"cluster": 0}, 1, 2]) == ([4, 6, 4], [0, 1, 2])
    # a survivor named twice gets twice the victims
    assert raftsim.split_plan([5, 5, 6], [0, 1, 2]) == ([5, 5, 6], [0, 1, 2])
    with pytest.raises(ValueError, match="no survivors"):
        raftsim.split_plan([], [1])
    with pytest.raises(ValueError, match=r"victims\[2\] = 7 is also a survivor"):
        raftsim.split_plan([7, 8], [1, 2, 7, 8])
    with pytest.raises(ValueError, match=r"victims\[3\] = 2 is a victim twice"):
        raftsim.split_plan([7], [1, 2, 3, 2, 1])


def test_the_config_check_names_the_field():
    base = dict(nodes=5, inbox_cap=16, log_cap=64, arena_cap=0, commit_stream_cap=0)
    cfg = lambda **kw: _abi.Config(**dict(base, **kw))  # noqa: E731
    raftsim.check_clone_fits(cfg(), cfg(seed=9, hb=5, trace_cap=4, n_devices=3, el_span=1))
    raftsim.check_clone_fits(cfg(), cfg(arena_cap=256))     # 0 means 4 * log_cap
    for field, other in (("nodes", 3), ("inbox_cap", 8), ("log_cap", 32), ("arena_cap", 255),
                         ("commit_stream_cap", 8)):
        with pytest.raises(ValueError, match=f"differ in {field}: the target's is .*source's {other}"):
            raftsim.check_clone_fits(cfg(), cfg(**{field: other, "arena_cap": 255 if field ==
                                                   "arena_cap" else 256}))
    assert _abi.CLONE_SHAPE == ("nodes", "inbox_cap", "log_cap", "arena_cap", "commit_stream_cap")
