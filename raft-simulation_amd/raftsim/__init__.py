"""raftsim — host side of the MI355X batched Raft simulator (libraftsim.so).

`Simulator` is the drop-in for the reference's per-process node loop (`-main`/`wait`,
src/raft/core.clj:176-203): it advances `n_clusters` independent N-node clusters in lockstep on one
GPU through the C ABI of include/raftsim.h. There is no CPU fallback: if libraftsim.so is missing,
was not built for this machine, or was built from other kernel sources than the ones beside it
(raftsim/_build.py), construction raises.
"""
from __future__ import annotations

import os
from pathlib import Path

from . import _build
from ._abi import COUNTER_NAMES  # noqa: F401
from . import _abi
from ._backend import (FAULT_NAMES, ROLE_NAMES, Backend, ClusterPack, GpuBackend,  # noqa: F401
                       RaftSimError, replay_config)

PKG_DIR = Path(__file__).resolve().parent.parent          # raft-simulation_amd/
LIB_PATH = Path(os.environ.get("RAFTSIM_LIB", PKG_DIR / "build" / "libraftsim.so"))


_checked = []


def check_build():
    """Refuse a libraftsim.so built from other kernel sources than the ones in this tree (the
    library embeds the hash of the sources it was compiled from; RAFTSIM_LIB overrides skip it)."""
    if _checked or "RAFTSIM_LIB" in os.environ:
        return
    want, got = _build.source_hash(), _build.embedded_hash(LIB_PATH)
    if want is None:
        raise RaftSimError("kernel sources missing beside the library: cannot check which sources "
                           f"{LIB_PATH} was built from")
    if got == "diag":
        raise RaftSimError(f"{LIB_PATH} is a diagnostic build (RS_DIAG_BUILD: its results or "
                           "counters may be wrong): load one only through RAFTSIM_LIB, and "
                           "rebuild the product with __graft_entry__.build_lib(force=True)")
    if got != want:
        raise RaftSimError(f"{LIB_PATH} was built from kernel sources {got}, the tree holds "
                           f"{want}: rebuild with __graft_entry__.build()")
    _checked.append(True)


class Simulator(GpuBackend):
    """Batched simulator on the GPU (HIP kernels for gfx950)."""

    def __init__(self, **config):
        if not LIB_PATH.exists():
            raise RaftSimError(f"{LIB_PATH} not built: run __graft_entry__.build()")
        check_build()
        super().__init__(LIB_PATH, "raft_sim_", **config)

    def diag_last_bails(self):
        """Diagnostic: clusters the steady kernel handed to the general kernel in the last tick
        launch (steady_kernel.hip), or -1 if that launch did not take the steady path."""
        import ctypes

        f = self._lib.raftsim_diag_last_bails
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p]
        return int(f(self._h))

    def diag_storm_bails(self):
        """Diagnostic: clusters the storm kernel (storm_kernel.hip) listed for the lane-per-node
        STORM body in the last storm launch, summed over shards; -1 if no storm-kernel launch ran
        on this handle."""
        import ctypes

        f = self._lib.raftsim_diag_storm_bails
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p]
        return int(f(self._h))

    def timed_launches(self):
        """Launches of the last sync window that carried HIP events: last_step_timing's average
        is over these (every general launch, the first steady launch after a sync)."""
        import ctypes

        f = self._lib.raftsim_last_timed_launches
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p]
        return int(f(self._h))


def replay(sim, cluster, ticks=None):
    """A one-cluster Simulator that reruns cluster `cluster` of `sim` with the trace rings on
    (sim.replay_config), stepped to `ticks` (default: sim's current tick) in sim's
    ticks_per_launch. Closes the loop search -> violations() -> replay -> edn_trace, and works the
    same on a cluster found by state: select() -> replay(sim, rec["cluster"]). Only a run
    from init-node is reproducible from its config: raises if the host ever wrote sim's state or
    clock (write_*, set_tick)."""
    if sim.host_written:
        raise RaftSimError("replay: the handle's state or clock was written by the host "
                           "(write_*, set_tick); only a run from init-node can be replayed")
    one = Simulator(**sim.replay_config(cluster))
    ticks = sim.tick if ticks is None else int(ticks)
    # (results do not depend on the step size; one step runs ticks_per_launch ticks per launch)
    if ticks:
        one.step(ticks)
    return one


def fork(source, cluster, **overrides):
    """A one-cluster Simulator that continues one cluster from a snapshot instead of rerunning it.
    `source` is a Simulator, whose cluster `cluster` is gathered with every part, or a ClusterPack
    (gather(), ClusterPack.load), of which `cluster` is the position in the pack. The new handle
    has the source's config with n_clusters=1 at the cluster's global id and the trace rings on
    (replay_config; `overrides` replace any field, e.g. trace_cap=0, trace_entry_cap=0), and is
    restored through restore_cluster: it starts at the pack's tick with the digest the cluster had
    there and continues bit-exactly as the cluster does in its source.

    Unlike replay(), fork works on handles the host has written (write_*, set_tick), and costs the
    snapshot, not the run so far. What it does not carry over, because neither is state: the
    fork's trace `seq` numbers (and entries_seq) start at 0 at the pack's tick, and its violation
    records start empty -- violations() of the fork reports what happens from the pack's tick on."""
    if isinstance(source, ClusterPack):
        pack, i = source, int(cluster)
        if not 0 <= i < len(pack):
            raise ValueError(f"position {i} outside the pack's {len(pack)} clusters")
    else:
        pack, i = source.gather([cluster]), 0
    cfg = replay_config(_abi.Config(**pack.config), pack.clusters[i], **overrides)
    one = Simulator(**cfg)
    one.restore_cluster(pack, i)
    return one
