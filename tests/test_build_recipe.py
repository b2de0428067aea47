"""The build recipe (raftsim/_build.py): the compiled units are csrc/'s, the command lines are the
ones written out here, build_lib runs exactly the product command, the unit list links without an
undefined project symbol, and nothing under scripts/ or tests/ keeps a unit list or a device
compile line of its own."""
import ast
import importlib.util
import re
import subprocess
from pathlib import Path

import hostprog
from raftsim import _build

ROOT = hostprog.ROOT
NAMES = ["tick_kernel.hip", "steady_kernel.hip", "storm_kernel.hip", "violations_kernel.hip",
         "census_kernel.hip", "audit_kernel.hip", "gather_kernel.hip", "scatter_kernel.hip",
         "raftsim.hip"]


def test_the_units_are_the_hip_files_of_csrc():
    assert sorted(ROOT / u for u in _build.UNITS) == sorted(hostprog.CSRC.glob("*.hip"))
    assert set(_build.UNITS) <= set(_build.KERNEL_SOURCES) and len(set(_build.UNITS)) == 9


def test_the_commands_are_these(monkeypatch):
    monkeypatch.setattr(_build, "HIPCC", "/x/hipcc")
    units = [f"/r/raft-simulation_amd/csrc/{n}" for n in NAMES]
    assert _build.lib_command("/o/lib.so", "0123456789abcdef", Path("/r")) == [
        "/x/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall",
        '-DRAFTSIM_SRC_HASH="0123456789abcdef"', "-o", "/o/lib.so", *units]
    assert _build.variant_command("/o/v.so", ["-DRS_BURST=0", "-DRS_WAVELOG"], Path("/r")) == [
        "/x/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall",
        "-DRS_DIAG_BUILD", "-DRS_BURST=0", "-DRS_WAVELOG", "-o", "/o/v.so", *units]
    assert _build.asm_command(_build.UNITS[2], "/o/u.s", Path("/r")) == [
        "/x/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
        "-o", "/o/u.s", units[2]]


def test_build_lib_runs_the_product_command(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("entry_under_test", ROOT / "__graft_entry__.py")
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    ran = []

    def record(cmd, cwd=None):
        ran.append([str(c) for c in cmd])
        Path(cmd[cmd.index("-o") + 1]).write_bytes(b"built")

    lib = tmp_path / "build" / "libraftsim.so"
    monkeypatch.setattr(entry, "LIB", lib)
    monkeypatch.setattr(entry, "_run", record)
    assert entry.build_lib(force=True) == lib and lib.read_bytes() == b"built"
    assert ran == [_build.lib_command(str(lib) + ".tmp", _build.source_hash(), ROOT)]
    assert not list(tmp_path.rglob("*.tmp"))


def undefined(tmp_path, units):
    """The project symbols (rs::, raft_) that a shared object of these units, compiled for the host
    alone and unoptimised, leaves undefined."""
    lib = tmp_path / "host.so"
    subprocess.run([_build.HIPCC, "--cuda-host-only", "-O0", "-std=c++17", "-fPIC", "-shared", "-o",
                    str(lib), *[str(ROOT / u) for u in units]], check=True)
    out = subprocess.run(["nm", "-uC", str(lib)], capture_output=True, text=True, check=True).stdout
    assert "__hip_fatbin" in out            # the device side, absent from a host-only link
    return [s for s in re.findall(r"^\s+U (.+)$", out, re.M) if re.match(r"rs::|raft_", s)]


def test_the_units_link_without_an_undefined_project_symbol(tmp_path):
    assert undefined(tmp_path, _build.UNITS) == []


def test_a_missing_unit_is_an_undefined_symbol(tmp_path):
    rest = [u for u in _build.UNITS if not u.endswith("/gather_kernel.hip")]
    assert len(rest) == 8
    assert any(s.startswith("rs::launch_gather(") for s in undefined(tmp_path, rest))


def strings(tree):
    """The string constants of a Python module that are not docstrings."""
    docs = {id(n.body[0].value) for n in ast.walk(tree)
            if isinstance(n, (ast.Module, ast.FunctionDef, ast.ClassDef)) and n.body and
            isinstance(n.body[0], ast.Expr) and isinstance(n.body[0].value, ast.Constant)}
    return [n.value for n in ast.walk(tree)
            if isinstance(n, ast.Constant) and isinstance(n.value, str) and id(n) not in docs]


def test_no_script_and_no_test_has_a_recipe_of_its_own():
    """Outside raftsim/_build.py no file of scripts/ or tests/ spells --offload-arch, and none names
    a unit as a file: in Python a string (no docstring) whose last path component is a unit's name,
    in shell any mention outside a comment. Prose that points a reader at a source file -- a
    docstring, a comment, the C++ text of a check program -- builds nothing and is left alone. The
    stand-alone probes and the profile scripts that compile one of them are no part of the
    library."""
    exempt = {"fetch_probe.hip", "p0_probe.hip", "launch_probe.hip", "profile_all.sh"}
    units = {Path(u).name for u in _build.UNITS}
    assert units == set(NAMES)
    files = [f for d in ("scripts", "tests") for f in sorted((ROOT / d).iterdir())
             if f.is_file() and f.name not in exempt and f.name != Path(__file__).name]
    assert len(files) >= 60
    found = []
    for f in files:
        text = f.read_text(errors="replace")
        if "--offload-arch" in text:
            found.append((f.name, "--offload-arch"))
        if f.suffix == ".py":
            found += [(f.name, s) for s in strings(ast.parse(text)) if Path(s).name in units]
        elif f.suffix == ".sh":
            code = re.sub(r"#.*", "", text)
            found += [(f.name, n) for n in units if n in code]
    # the two asserts that a kernel's file is in KERNEL_SOURCES, and so in the hash
    member = [(f"test_{k}_abi.py", f"raft-simulation_amd/csrc/{k}_kernel.hip")
              for k in ("gather", "scatter")]
    assert sorted(found) == member, found
