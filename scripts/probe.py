"""What the scripts of this directory share (imported, never run): the import path, bench.py's
workloads as handle configs, a handle on the product library or on any build of it, the 10k-tick
launch loop, the comparison of builds, a -DRS_WAVELOG build's per-wave log and the reports' small
formatters. The comparison of a handle with the C oracle is tests/pairing.py's."""
import argparse
import collections
import ctypes
import importlib.util
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / d) for d in ("raft-simulation_amd", "tests", "oracle", "scripts")]
import raftsim  # noqa: E402  (loads no library: a handle does)

_spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
bench = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bench)
SHARD = 131072      # one GPU's share of a strong-scaled workload (1,048,576 clusters over 8 GPUs)
TICKS = bench.TICKS_PER_STEP
Launch = collections.namedtuple("Launch", "ms launches span wall")


def parser(doc, workloads=False):
    """A script's argument parser: its docstring as the help text; workloads: a --NAME selector
    (--c4_n9 ...) for every bench workload, the chosen names in args.only (None: none given)."""
    p = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawTextHelpFormatter)
    for name in bench.WORKLOADS if workloads else ():
        p.add_argument("--" + name, dest="only", action="append_const", const=name,
                       help="workload " + name)
    return p


def workload(name, clusters=None, **overrides):
    """The handle config of bench.py's workload `name`: its cfg, n_clusters (default: the
    workload's own count where it scales weakly, one GPU's SHARD where strongly), overrides."""
    if name not in bench.WORKLOADS:
        raise KeyError(f"unknown workload {name!r}: one of {', '.join(bench.WORKLOADS)}")
    spec = bench.WORKLOADS[name]
    if clusters is None:
        clusters = spec["clusters"] if spec["scaling"] == "weak" else SHARD
    return dict(spec["cfg"], n_clusters=clusters, **overrides)


def open_sim(lib=None, **cfg):
    """A handle on the build `lib`, whatever its tag; without one, on the product library
    (raftsim.Simulator: RAFTSIM_LIB, and the source-hash check)."""
    return raftsim.Simulator(**cfg) if lib is None else raftsim.GpuBackend(lib, "raft_sim_", **cfg)


def require_diag(lib, who, why):
    """End the script unless `lib` is a diagnostic variant (the product `why`)."""
    if raftsim._build.embedded_hash(Path(lib)) != "diag":
        sys.exit(f"{who}: {lib} is not a diagnostic build, so it {why}: build a variant with "
                 "scripts/build_variants.sh and pass it through RAFTSIM_LIB")


def launches(sim, k, ticks=TICKS):
    """Step `ticks` k times: per step the tick kernel's average ms, its launches, the step's device
    span and its wall ms. A backend that keeps no timing (the oracle) gives zeros."""
    out = []
    for _ in range(k):
        t0 = time.perf_counter()
        sim.step(ticks)
        wall = (time.perf_counter() - t0) * 1e3
        ms, n = sim.last_step_timing() if "last_step_timing" in sim._fns else (0.0, 0)
        out.append(Launch(ms, n, sim.last_span() if "last_span" in sim._fns else 0.0, wall))
    return out


def agree(sims, c0=0, nc=None):
    """Whether clusters [c0, c0 + nc) of every handle have the same digests (nc None: to the end)."""
    return len({bytes(s.digest(c0, nc)) for s in sims}) == 1


def wavelog(sim, waves, width=48):
    """The per-wave records of the last launch of a -DRS_WAVELOG build, `width` words each, of the
    waves that ran (padding waves exit first), and their start and end stamps (100 per us).
    raftsim_diag_wavelog copies 192 B per wave of its count (the general kernel's record);
    the steady kernel's records are 128 B apart (width 32) from the buffer's start."""
    f = sim._lib.raftsim_diag_wavelog
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    buf = (ctypes.c_uint32 * (waves * 48))()
    n = f(sim._h, buf, waves)
    a = np.frombuffer(buf, dtype=np.uint32)[:n * 48 // width * width].reshape(-1, width)
    a = a.astype(np.int64)
    a = a[(a[:, 0] | a[:, 1]) != 0]
    return a, a[:, 0] | (a[:, 1] << 32), a[:, 2] | (a[:, 3] << 32)


def pct(x, width=7):
    """p0/10/50/90/99/100 of x."""
    return " ".join(f"{v:{width}.1f}" for v in np.percentile(x, [0, 10, 50, 90, 99, 100]))


def simd_packing(hw, xcc):
    """The report line of how many waves each SIMD ran: hw the waves' HW_ID words (SIMD, CU, SH,
    SE), xcc their XCC ids; and the per-wave key that is distinct per SIMD of the chip."""
    simd, cu, sh, se = (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
    key = xcc * 10000 + se * 1000 + sh * 100 + cu * 4 + simd
    u, cnt = np.unique(key, return_counts=True)
    print("distinct SIMDs", len(u), "waves per SIMD p0/50/100", cnt.min(), np.median(cnt), cnt.max())
    return key


def emit(rec):
    print(json.dumps(rec), flush=True)


def best(fn, calls=4, keep=3):
    """(kernel ms, wall ms), each the minimum over the last `keep` of `calls` calls of fn, which
    returns its kernel ms."""
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        ms = fn()
        out.append((ms, (time.perf_counter() - t0) * 1e3))
    return min(k for k, _ in out[-keep:]), min(w for _, w in out[-keep:])
