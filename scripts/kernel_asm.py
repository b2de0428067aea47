"""The device assembly of every compiled unit (raftsim/_build.py: UNITS, asm_command): the table of
registers, scratch and occupancy as the compiler reports them, and the comparison of two trees'
assembly kernel by kernel -- the check that a change of the host side, or a refactor of a kernel
source, left the device code as it was.

  python3 scripts/kernel_asm.py [--asm-dir DIR]
      Compile every unit of this tree once (16 at a time at most) and print the table that
      scripts/kernel_resources.sh writes to profiles/TAG_kernel_resources.txt. The counts are the
      ISA comments of hipcc -S; rocprofv3's VGPR_Count column uses a different encoding. With
      --asm-dir, keep the normalised assembly as DIR/<unit>.s.
  python3 scripts/kernel_asm.py diff DIR_A DIR_B
      For every function of every unit of two --asm-dir runs: identical or not, and the same for
      what a unit holds outside its functions (data, metadata). Exit status 1 if anything differs.

Normalisation removes what differs between two compiles of the same file from two directories, and
nothing else. Found by compiling this tree's nine units from two directories and comparing: the
one difference is the name of the symbol __hip_cuid_<16 hex digits>, which clang derives from the
file's path (five lines of each unit: .type, .globl, the label, .size, .addrsig_sym). Its digits
are removed. The assembly has no .file directive, no path and no time.
"""
import argparse
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "raft-simulation_amd"))
from raftsim import _build  # noqa: E402

JOBS = 16
# a function: its "Begin function" line up to the resource comments that follow "End function"
FUNCTION = re.compile(r"^[^\n]*; -- Begin function (\S+)\n.*?; -- End function\n"
                      r"(?:\t\.set [^\n]*\n|\t\.section\t\.AMDGPU\.csdata[^\n]*\n|;[^\n]*\n)*",
                      re.M | re.S)
PRETTY = [
    (r"11tick_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)", lambda m:
     f"tick_kernel<N={m[1]}, TRACE={m[2]}, SPEC={m[3]}, LITE={m[4]}{', STORM' * (m[5] == '1')}>"),
    (r"\d+((?:steady|storm)_lane_kernel)ILi(\d)E", lambda m: f"{m[1]}<N={m[2]}>"),
    (r"\d+((?:census|viol|audit|gather|scatter|clone|restart)_\w*?kernel)E", lambda m: m[1]),
    (r"19summary_fold_kernelI\d+raft_([a-z]+)E", lambda m: f"summary_fold_kernel<{m[1]}>"),
    (r"12audit_kernelILj(\d)ELj(\d+)E", lambda m: f"audit_kernel<N={m[1]}, G={m[2]}>"),
    # the compaction (compact.hpp): compact_count<viol>; the scan, one copy per file that uses it
    (r"L?\d+(compact_[a-z]+)(?:INS_\d+(\w+?)EEE)?", lambda m: m[1] + (f"<{m[2]}>" if m[2] else "")),
]


def compile_unit(unit):
    """The normalised device assembly of one unit."""
    r = subprocess.run(_build.asm_command(unit, "-", ROOT), capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{unit}: compile failed\n{r.stderr}")
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", r.stdout)


def pretty(name):
    """The table's name of a mangled rs:: function: the first pattern that matches."""
    p = name.replace("_ZN2rs", "rs::")
    for pattern, fmt in PRETTY:
        m = re.match("rs::" + pattern, p)
        if m:
            return fmt(m)
    return p


def table(asm):
    """One row for every rs:: function of every unit, in the units' order."""
    rows = [f"{'kernel':48s} {'VGPRs':>5s} {'SGPRs':>5s} {'scratch':>7s} {'waves/SIMD':>10s}"]
    for text in asm.values():
        for m in FUNCTION.finditer(text):
            if not m[1].startswith("_ZN2rs"):
                continue
            info = m[0][m[0].index(".Lfunc_end"):]
            get = lambda k: (re.search(r"; " + k + r": (\d+)", info) or [None, "?"])[1]  # noqa: E731
            rows.append(f"{pretty(m[1])[:48]:48s} {get('NumVgprs'):>5s} {get('TotalNumSgprs'):>5s} "
                        f"{get('ScratchSize'):>7s} {get('Occupancy'):>10s}")
    return "\n".join(rows)


def parts(text):
    """{function name: its text}, and under "" everything outside the functions."""
    return {"": FUNCTION.sub("", text), **{m[1]: m[0] for m in FUNCTION.finditer(text)}}


def diff(dir_a, dir_b):
    differing = 0
    for f in sorted({p.name for d in (dir_a, dir_b) for p in Path(d).glob("*.s")}):
        a, b = (parts(p.read_text()) if p.exists() else {} for p in (Path(dir_a) / f, Path(dir_b) / f))
        for name in dict.fromkeys([*a, *b]):
            same = a.get(name) == b.get(name)
            differing += not same
            what = pretty(name) if name else "(outside the functions)"
            state = ("identical" if same else "DIFFERS" if name in a and name in b
                     else f"only in {dir_a if name in a else dir_b}")
            print(f"{Path(f).stem:18s} {what[:60]:60s} {state}")
    print(f"{differing} differ")
    return 1 if differing else 0


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--asm-dir", metavar="DIR", help="keep the normalised assembly as DIR/<unit>.s")
    p.add_argument("diff", nargs="*", metavar="diff DIR_A DIR_B",
                   help="compare two --asm-dir runs instead of compiling")
    args = p.parse_args(argv)
    if args.diff:
        if args.diff[0] != "diff" or len(args.diff) != 3 or args.asm_dir:
            p.error("expected: diff DIR_A DIR_B")
        return diff(*args.diff[1:])
    with ThreadPoolExecutor(JOBS) as pool:
        asm = dict(zip(_build.UNITS, pool.map(compile_unit, _build.UNITS)))
    if args.asm_dir:
        Path(args.asm_dir).mkdir(parents=True, exist_ok=True)
        for unit, text in asm.items():
            (Path(args.asm_dir) / (Path(unit).stem + ".s")).write_text(text)
    print(table(asm))
    return 0


if __name__ == "__main__":
    sys.exit(main())
