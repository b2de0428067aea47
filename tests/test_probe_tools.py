"""The tools of scripts/ (CPU): each one parses its arguments without touching a library, the
handle configs of scripts/probe.py are bench.py's workloads, no script keeps a fault or client
table of its own, and the harness's launch loop, build comparison and one_case.py's comparison run
on oracle handles."""
import ast
import os
import subprocess
import sys
from pathlib import Path

import pytest

import cases
import pairing

ROOT = Path(__file__).resolve().parent.parent
SCRIPTS = ROOT / "scripts"
sys.path.insert(0, str(SCRIPTS))
import one_case  # noqa: E402
import probe  # noqa: E402

TOOLS = sorted(p.name for p in SCRIPTS.glob("*.py") if p.name != "probe.py")
# the fields of the tables the scripts no longer hold. client_burst is not among them: the
# probes of perf_probe.py that switch bench.py's bursts off say so as a plain override,
# client_burst=0, beside client_period=0 and client_redirects=0, and so does none of the rest.
TABLE_FIELDS = {"drop_ppm", "dup_ppm", "part_ppm"}


@pytest.mark.parametrize("tool", TOOLS)
def test_help_loads_no_library(tool, tmp_path):
    """--help exits 0 with a usage line while RAFTSIM_LIB names a file that does not exist: neither
    the import nor the argument parsing opens a library or makes a handle."""
    env = dict(os.environ, RAFTSIM_LIB=str(tmp_path / "no_such_library.so"))
    r = subprocess.run([sys.executable, str(SCRIPTS / tool), "--help"], capture_output=True,
                       text=True, env=env, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("usage: " + tool), r.stdout[:200]


def test_workload_is_the_bench_workload():
    assert set(probe.bench.WORKLOADS) >= {"c2", "c2_init", "c3", "c3_spec", "c4_n7", "c4_n9",
                                          "c4_spec", "c5"}
    for name, spec in probe.bench.WORKLOADS.items():
        cfg = probe.workload(name)
        want = spec["clusters"] if spec["scaling"] == "weak" else probe.SHARD
        assert cfg.pop("n_clusters") == want, name
        assert cfg == spec["cfg"], name
        assert probe.workload(name, 77)["n_clusters"] == 77
    assert probe.SHARD == 131072
    assert {n for n, s in probe.bench.WORKLOADS.items() if s["scaling"] == "strong"} == {
        "c3", "c3_spec"}


def test_workload_overrides_win_and_leave_the_bench_alone():
    before = dict(probe.bench.WORKLOADS["c3"]["cfg"])
    cfg = probe.workload("c3", 2048, client_ppm=10000, schedule=1)
    assert (cfg["client_ppm"], cfg["schedule"], cfg["n_clusters"]) == (10000, 1, 2048)
    assert {k: v for k, v in cfg.items() if k not in ("client_ppm", "schedule", "n_clusters")} == {
        k: v for k, v in before.items() if k != "client_ppm"}
    assert probe.bench.WORKLOADS["c3"]["cfg"] == before


def test_unknown_workload_names_the_choices():
    with pytest.raises(KeyError) as e:
        probe.workload("c9")
    assert all(name in str(e.value) for name in probe.bench.WORKLOADS)


def test_no_script_keeps_a_fault_table():
    """Outside docstrings no keyword argument and no string of scripts/*.py is one of
    TABLE_FIELDS (see there for client_burst): the workloads come from bench.py through
    probe.workload."""
    found = []
    for f in sorted(SCRIPTS.glob("*.py")):
        tree = ast.parse(f.read_text())
        docs = {id(n.body[0].value) for n in ast.walk(tree)
                if isinstance(n, (ast.Module, ast.FunctionDef, ast.ClassDef)) and n.body and
                isinstance(n.body[0], ast.Expr) and isinstance(n.body[0].value, ast.Constant)}
        for n in ast.walk(tree):
            if isinstance(n, ast.keyword) and n.arg in TABLE_FIELDS:
                found.append((f.name, n.arg))
            if isinstance(n, ast.Constant) and n.value in TABLE_FIELDS and id(n) not in docs:
                found.append((f.name, n.value))
    assert len(list(SCRIPTS.glob("*.py"))) >= 16
    assert found == []


@pytest.fixture
def oracles():
    cfg = cases.cfg_of("n3", 8)
    with pairing.closing(pairing.oracle(cfg), pairing.oracle(cfg)) as handles:
        yield handles


def test_launches_and_agree_on_oracle_handles(oracles):
    a, b = oracles
    recs = probe.launches(a, 3, ticks=500)
    assert len(recs) == 3 and a.tick == 1500
    # the oracle keeps no launch timing: zeros, and the wall time of the step
    assert all((r.ms, r.launches, r.span) == (0.0, 0, 0.0) and r.wall >= 0 for r in recs)
    assert not probe.agree([a, b])              # 1,500 ticks against none
    assert len(probe.launches(b, 1, ticks=1500)) == 1
    assert probe.agree([a, b]) and probe.agree([a, b], 2, 5) and probe.agree([a])
    b.step(1500)
    assert not probe.agree([a, b])


def test_one_case_compares_through_pairing():
    """one_case.py's comparison with an oracle in the GPU handle's place, in one step and in
    chunks that do not divide the ticks: nothing differs, the counters are equal, no report."""
    import helpers
    cfg = cases.CASES["n2"]
    assert one_case.compare(cfg, helpers.oracle, ticks=2000) == (0, True, "")
    assert one_case.compare(cfg, helpers.oracle, ticks=2000, chunk=700) == (0, True, "")
