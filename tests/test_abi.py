"""The C ABI: header <-> ctypes layouts, exported symbols, loud failure without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

import hostprog
import raftsim
from hostprog import CSRC, HEADER, ROOT
from raftsim import _abi


def header_functions():
    text = HEADER.read_text()
    return sorted(set(re.findall(r"\b(raft_sim_\w+)\s*\(", text)))


def test_header_declares_exactly_the_bound_symbols():
    assert header_functions() == sorted(_abi.PRODUCT_SYMBOLS)


def test_library_exports_every_header_symbol():
    missing = set(header_functions()) - hostprog.exported(r"raft_sim_\w+")
    assert not missing, missing
    lib = ctypes.CDLL(str(raftsim.LIB_PATH))        # loads without a GPU
    for sym in header_functions():
        assert hasattr(lib, sym)


def test_library_is_built_from_these_sources():
    """libraftsim.so embeds the hash of the kernel sources it was compiled from; it must be this
    tree's (a stale binary would ship to the GPU box beside newer sources, and Simulator refuses
    it there). build_lib() rebuilds on a mismatch."""
    from raftsim import _build

    assert raftsim.LIB_PATH.exists(), "run __graft_entry__.build() first"
    assert _build.embedded_hash(raftsim.LIB_PATH) == _build.source_hash()
    lib = ctypes.CDLL(str(raftsim.LIB_PATH))
    lib.raftsim_src_hash.restype = ctypes.c_char_p
    assert lib.raftsim_src_hash().decode() == _build.source_hash()


def test_source_hash_covers_every_included_project_file():
    """Every project file that a file of KERNEL_SOURCES includes (#include "...") is itself in
    KERNEL_SOURCES: a header left out could change without the hash, and with it the stale-binary
    check, noticing."""
    from raftsim import _build

    listed = {(ROOT / f).resolve() for f in _build.KERNEL_SOURCES}
    includes = 0
    for src in sorted(listed):
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', src.read_text(), re.M):
            includes += 1
            assert (src.parent / inc).resolve() in listed, f"{src.name} includes {inc}"
    assert includes >= 6, "every .hip file includes a project header: the pattern misses them"


# the compile-time switches csrc/device.hpp declares (diagnostic builds only)
SWITCHES = ["RS_BURST", "RS_BURST_MIN", "RS_BURST_SKIP", "RS_BURST_DIAG", "RS_WAVELOG"]


@pytest.mark.parametrize("switch", SWITCHES)
def test_switches_need_a_diagnostic_build(switch):
    """Setting a kernel switch without RS_DIAG_BUILD is a compile error that names the switch
    (preprocessing only); with RS_DIAG_BUILD it is accepted."""
    from raftsim import _build

    cmd = [hostprog.HIPCC, "-E", "--cuda-host-only", "-std=c++17", f"-D{switch}=0", "-o", os.devnull,
           str(ROOT / _build.UNITS[0])]
    plain = subprocess.run(cmd, capture_output=True, text=True)
    assert plain.returncode != 0
    assert re.search(rf"\b{switch}\b", plain.stderr), plain.stderr
    diag = subprocess.run(cmd + ["-DRS_DIAG_BUILD"], capture_output=True, text=True)
    assert diag.returncode == 0, diag.stderr


def test_embedded_hash_recognises_a_diagnostic_tag(tmp_path):
    from raftsim import _build

    f = tmp_path / "lib.so"
    f.write_bytes(b"\x7fELF\0junk RAFTSIM_SRC_HASH=diag\0 more")
    assert _build.embedded_hash(f) == "diag"
    f.write_bytes(b"\x7fELF\0junk RAFTSIM_SRC_HASH=0123456789abcdef\0 more")
    assert _build.embedded_hash(f) == "0123456789abcdef"


def test_check_build_refuses_a_diagnostic_library(tmp_path, monkeypatch):
    """A library tagged "diag" (built with RS_DIAG_BUILD: its results or counters may be wrong) is
    never taken for the product; RAFTSIM_LIB, how variants are loaded, still skips the check."""
    f = tmp_path / "libraftsim.so"
    f.write_bytes(b"RAFTSIM_SRC_HASH=diag\0")
    monkeypatch.setattr(raftsim, "LIB_PATH", f)
    monkeypatch.setattr(raftsim, "_checked", [])
    monkeypatch.delenv("RAFTSIM_LIB", raising=False)
    with pytest.raises(raftsim.RaftSimError, match="diagnostic"):
        raftsim.check_build()
    assert not raftsim._checked
    monkeypatch.setenv("RAFTSIM_LIB", str(f))
    raftsim.check_build()


def test_kernel_sources_name_only_the_declared_switches():
    """Every RS_* token in the kernel sources is one of device.hpp's switches, RS_DIAG_BUILD or a
    function-like helper macro: a new knob has to be added to the fenced block in device.hpp and
    to this list on purpose, and a retired one cannot linger in a condition."""
    allowed = set(SWITCHES) | {"RS_DIAG_BUILD", "RS_PLAN", "RS_SB", "RS_STORM", "RS_CFG",
                               "RS_LANE", "RS_PHASE", "RS_PX", "RS_LPH"}
    found = {}
    for f in sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.hpp")):
        for tok in re.findall(r"\bRS_[A-Z0-9_]+\b", f.read_text()):
            found.setdefault(tok, f.name)
    assert len(found) >= len(SWITCHES)
    stray = {t: n for t, n in found.items() if t not in allowed}
    assert not stray, stray


def test_oracle_mirrors_the_abi():
    import helpers
    lib = ctypes.CDLL(str(helpers.ORACLE_LIB))
    for sym in header_functions():
        if sym in ("raft_sim_last_step_timing", "raft_sim_last_span"):   # device timing only
            continue
        assert hasattr(lib, sym.replace("raft_sim_", "raft_ref_")), sym


def test_struct_layouts_match_the_c_compiler(tmp_path):
    structs = {"raft_sim_config_t": _abi.Config, "raft_node_t": _abi.Node,
               "raft_msg_t": _abi.Msg, "raft_entry_t": _abi.Entry, "raft_cluster_t": _abi.Cluster,
               "raft_counters_t": _abi.Counters}
    assert hostprog.c_layout(tmp_path, structs) == []


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(raftsim.RaftSimError, match="gfx950|HIP|device"):
        raftsim.Simulator(n_clusters=4)


def test_config_validation_matches_oracle():
    import helpers
    bad = [dict(nodes=1), dict(nodes=10), dict(inbox_cap=0), dict(inbox_cap=17),
           dict(log_cap=8, arena_cap=15), dict(dmin=0), dict(dmin=5, dmax=4), dict(dmax=256),
           dict(drop_ppm=1000001), dict(hb=0), dict(part_epoch=0)]
    for b in bad:
        with pytest.raises(raftsim.RaftSimError):
            helpers.oracle(n_clusters=2, **b)
