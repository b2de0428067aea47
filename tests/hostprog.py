"""What the CPU-side tests of the C and C++ sources share: the compilers, which sanitizer runtimes
each has on this machine, the compile-and-run of a stand-alone check program, the C compiler's view
of the ABI structures, and the product library's exported symbols."""
import ctypes
import glob
import os
import re
import subprocess
from pathlib import Path

import raftsim
from raftsim._build import HIPCC  # noqa: F401  (the tests' one source of the compiler)

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "raft-simulation_amd" / "csrc"
HEADER = ROOT / "include" / "raftsim.h"


def gcc_sanitizers():
    """The -fsanitize= names whose runtime gcc has here."""
    def runtime(lib):
        p = subprocess.run(["gcc", f"-print-file-name={lib}"], capture_output=True,
                           text=True).stdout.strip()
        return os.path.isabs(p) and os.path.exists(p)
    return {s for s, lib in (("undefined", "libubsan.so"), ("address", "libasan.so")) if runtime(lib)}


def hipcc_sanitizers():
    """The -fsanitize= names whose host runtime hipcc's clang has here."""
    rt = str(Path(os.path.realpath(HIPCC)).parent.parent / "lib/llvm/lib/clang/*/lib/linux")
    return {s for s, lib in (("undefined", "ubsan_standalone"), ("address", "asan"))
            if glob.glob(f"{rt}/libclang_rt.{lib}-x86_64.a")}


def run_cpp(tmp_path, name, program, compiler="g++", opt="-O1", sanitizers=("undefined",),
            timeout=120):
    """Write `program` to tmp_path/name.cpp, compile it with every warning an error and csrc/ on the
    include path -- with g++, or for the host alone with hipcc -- under those of `sanitizers` the
    compiler has a runtime for, and run it once: exit status 0 and nothing on stderr. Returns its
    stdout. The sanitizers applied are printed, so a failure's report shows what the run checked."""
    src, exe = tmp_path / f"{name}.cpp", tmp_path / name
    src.write_text(program)
    have = hipcc_sanitizers() if compiler == "hipcc" else gcc_sanitizers()
    applied = ",".join(s for s in sanitizers if s in have)
    if compiler == "hipcc":
        cmd = [HIPCC, "-x", "hip", "--offload-host-only"]
        san = ["-Xarch_host", f"-fsanitize={applied}", "-Xarch_host", "-fno-sanitize-recover=all"]
    else:
        cmd = [compiler]
        san = [f"-fsanitize={applied}", "-fno-sanitize-recover"]
    cmd += ["-std=c++17", opt, "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)]
    print(f"{name}: {compiler} {opt}, sanitizers applied: {applied or 'none'} of {sanitizers}")
    subprocess.run(cmd + (san if applied else []), check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def checks(out):
    """The N of a check program's last line, `checks N bad 0`."""
    last = out.strip().splitlines()[-1].split()
    assert last[0] == "checks" and last[2] == "bad" and last[3] == "0", out[-3000:]
    return int(last[1])


def c_layout(tmp_path, structs, extra_printf_lines=()):
    """Compile and run a C program over include/raftsim.h that prints the size and every member's
    offset of `structs` ({C name: ctypes class}) and then `extra_printf_lines` (C statements). The
    sizes and offsets must be the ctypes classes'; returns the lines the extra statements printed."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    want = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        want.append(f"{cname} sizeof {ctypes.sizeof(cls)}")
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
            want.append(f"{cname} {f} {getattr(cls, f).offset}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join([*lines, *extra_printf_lines, "return 0; }"]))
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[:len(want)] == want, [(c, py) for c, py in zip(out, want) if c != py]
    return out[len(want):]


def exported(pattern):
    """The names matching `pattern` that the product library defines and exports as functions."""
    assert raftsim.LIB_PATH.exists(), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", str(raftsim.LIB_PATH)],
                         capture_output=True, text=True, check=True).stdout
    return set(re.findall(rf"\bT ({pattern})$", out, re.M))
