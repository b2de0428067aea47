"""Where the steady kernel's certified waves end, read from the gfx950 assembly in layout order
(steady_kernel.hip, "the wave ends here"): a line-0 wave stores its lines, adds its counters and
ends right behind its body, before the code of the paths it does not take. Compiles the steady
unit once with the recipe's asm_command (about 10 s); skipped where there is no hipcc.

For steady_lane_kernel<5> and <2>:
  * the kernel has at least two s_endpgm;
  * the first one stands before the first global_load_lds of line 1 (the ninth of the kernel: the
    first eight load line 0);
  * between the first `s_waitcnt vmcnt(0)` and that s_endpgm stand the eight unpredicated
    write-through stores of line 0: eight `global_store_dwordx4 ... sc1` in a row with no label,
    no branch and no write of exec between them.
Mnemonics only: no register, no count of instructions, no timing."""
import re
import subprocess
from pathlib import Path

import pytest

import hostprog
from raftsim import _build

pytestmark = pytest.mark.skipif(not Path(_build.HIPCC).exists(), reason="no hipcc")


@pytest.fixture(scope="module")
def kernels():
    """{N: the instructions and labels of steady_lane_kernel<N>, in layout order}."""
    unit = next(u for u in _build.UNITS if Path(u).stem == "steady_kernel")
    r = subprocess.run(_build.asm_command(unit, "-", hostprog.ROOT), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for m in re.finditer(r"^_ZN2rs\d+steady_lane_kernelILi(\d)E\w*:[^\n]*\n(.*?)^\.Lfunc_end",
                         r.stdout, re.M | re.S):
        lines = (ln.split(";")[0].strip() for ln in m[2].split("\n"))
        out[int(m[1])] = [ln for ln in lines if ln and (ln.endswith(":") or not ln.startswith("."))]
    return out


def first(stream, prefix, nth=0):
    return [i for i, x in enumerate(stream) if x.startswith(prefix)][nth]


def breaks_a_run(x):
    """A label, a branch, or an instruction that writes exec (v_cmpx among them)."""
    return (x.endswith(":") or x.startswith(("s_cbranch", "s_branch", "s_setpc", "v_cmpx")) or
            "saveexec" in x or re.match(r"s_\w+ exec\b", x) is not None)


@pytest.mark.parametrize("nodes", [5, 2])
def test_a_line0_wave_ends_behind_its_body(kernels, nodes):
    k = kernels[nodes]
    ends = [i for i, x in enumerate(k) if x.startswith("s_endpgm")]
    assert len(ends) >= 2, ends
    line1 = first(k, "global_load_lds", 8)
    assert ends[0] < line1, (ends[0], line1)
    wait = first(k, "s_waitcnt vmcnt(0)")
    assert wait < ends[0]
    best = run = 0
    for x in k[wait:ends[0]]:
        if x.startswith("global_store_dwordx4") and x.endswith("sc1"):
            run += 1
            best = max(best, run)
        elif breaks_a_run(x):
            run = 0
    print(f"N={nodes}: first s_endpgm at line {ends[0]} of {len(k)}, line 1 loaded from {line1}, "
          f"longest run of unpredicated sc1 stores before it {best}")
    assert best == 8, best
