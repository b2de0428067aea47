"""The build recipe of libraftsim.so: its sources, the hash that keys the build, the compiler, the
flags and the command lines. Everything that compiles the kernel sources takes them from here.

`__graft_entry__.build_lib()` compiles the library with the hash of these files embedded
(RAFTSIM_SRC_HASH) and rebuilds whenever the embedded hash differs from the sources' hash;
`raftsim.Simulator` refuses a library whose embedded hash is not the hash of the sources next to
it, so a box never runs a stale binary shipped beside newer sources. bench.py keys its PMC
traffic records (pmc_traffic.json) on the same hash.

The commands (argv lists): `lib_command` the product, `variant_command` a diagnostic variant
(scripts/build_variants.sh), `asm_command` one unit's device assembly (scripts/kernel_asm.py).
"""
from __future__ import annotations

import hashlib
import os
import re
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent.parent
KERNEL_SOURCES = ["raft-simulation_amd/csrc/tick_kernel.hip",
                  "raft-simulation_amd/csrc/steady_kernel.hip",
                  "raft-simulation_amd/csrc/storm_kernel.hip",
                  "raft-simulation_amd/csrc/violations_kernel.hip",
                  "raft-simulation_amd/csrc/census_kernel.hip",
                  "raft-simulation_amd/csrc/audit_kernel.hip",
                  "raft-simulation_amd/csrc/gather_kernel.hip",
                  "raft-simulation_amd/csrc/scatter_kernel.hip",
                  "raft-simulation_amd/csrc/scatter_host.hpp",
                  "raft-simulation_amd/csrc/clone_host.hpp",
                  "raft-simulation_amd/csrc/restart_host.hpp",
                  "raft-simulation_amd/csrc/launch_plan.hpp",
                  "raft-simulation_amd/csrc/node_codec.hpp",
                  "raft-simulation_amd/csrc/pack.hpp",
                  "raft-simulation_amd/csrc/tick_wave.hpp", "raft-simulation_amd/csrc/device.hpp",
                  "raft-simulation_amd/csrc/compact.hpp",
                  "raft-simulation_amd/csrc/summary.hpp",
                  "raft-simulation_amd/csrc/summary_host.hpp",
                  "raft-simulation_amd/csrc/fixed_point_affine.hpp",
                  "raft-simulation_amd/csrc/raftsim.hip", "include/raftsim.h"]
# the compiled units: the .hip files among them, in that order (the order of the command line)
UNITS = [f for f in KERNEL_SOURCES if f.endswith(".hip")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
LIB_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", "-Wall"]
ASM_FLAGS = ["-O3", "-std=c++17", "-S", "--cuda-device-only"]


def _link(out, defines, root) -> list[str]:
    return [HIPCC, f"--offload-arch={ARCH}", *LIB_FLAGS, *defines, "-o", str(out),
            *[str(Path(root) / u) for u in UNITS]]


def lib_command(out, src_hash: str, root: Path = REPO) -> list[str]:
    """The command that compiles the product library to `out` with `src_hash` embedded."""
    return _link(out, [f'-DRAFTSIM_SRC_HASH="{src_hash}"'], root)


def variant_command(out, defines, root: Path = REPO) -> list[str]:
    """The product command with -DRS_DIAG_BUILD and the caller's defines in place of the hash: a
    diagnostic variant, tagged "diag" (csrc/device.hpp lists the switches)."""
    return _link(out, ["-DRS_DIAG_BUILD", *defines], root)


def asm_command(unit: str, out, root: Path = REPO) -> list[str]:
    """The command that writes the device assembly of one of UNITS to `out`."""
    return [HIPCC, f"--offload-arch={ARCH}", *ASM_FLAGS, "-o", str(out), str(Path(root) / unit)]


# "diag": a diagnostic build (csrc/device.hpp's switches, RS_DIAG_BUILD), whatever its sources
_TAG = re.compile(rb"RAFTSIM_SRC_HASH=([0-9a-f]{16}|unknown|diag)")


def source_hash(root: Path = REPO) -> str | None:
    """sha256 of the kernel sources under root (first 16 hex digits); None if any is missing."""
    h = hashlib.sha256()
    for f in KERNEL_SOURCES:
        try:
            h.update((Path(root) / f).read_bytes())
        except OSError:
            return None
    return h.hexdigest()[:16]


def embedded_hash(lib: Path) -> str | None:
    """The source hash a built libraftsim.so carries ("diag" for a diagnostic build; None if it
    carries none)."""
    try:
        m = _TAG.search(Path(lib).read_bytes())
    except OSError:
        return None
    return m.group(1).decode() if m else None
