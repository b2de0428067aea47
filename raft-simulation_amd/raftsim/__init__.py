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
                       RaftSimError, check_clone_fits, check_pack_fits, replay_config,
                       restart_lists, restart_mode)
from .restart import (philox, restart_by_writes, restart_deadline, restart_record,  # noqa: F401
                      supervise)

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


def _scattered(pack, who, cfg, records=None):
    """A Simulator of config `cfg` at the pack's tick whose clusters are the pack's `records`
    (default: record i for cluster i), written by one scatter."""
    check_pack_fits(_abi.Config(**cfg), pack, who)
    sim = Simulator(**cfg)
    try:
        sim.set_tick(pack.tick)
        sim.scatter(pack, range(cfg["n_clusters"]), records)
    except Exception:
        sim.close()
        raise
    return sim


def resume(pack, **overrides):
    """A Simulator that continues the clusters of a ClusterPack: the pack's config with n_clusters
    = len(pack) at the global id of the pack's first cluster, one device and the trace rings off
    (`overrides` replace any field, e.g. n_devices), set to the pack's tick and written by one
    scatter() on the device. The pack's clusters must be a run of consecutive ascending ids
    (gather(range(c0, c0 + n))): cluster i of the new handle then has the global id the i-th
    packed cluster had, so it continues bit-exactly as that cluster does in its source.

    resume(ClusterPack.load(path)) is the checkpoint path: gather(range(sim.C)).save(path) writes
    a handle's whole state to a file, and this loads it back into a running handle at the speed of
    the upload. Like fork(), it carries over neither violation records nor counters nor trace
    `seq` numbers, none of which is state; unlike fork(), it continues any number of clusters."""
    n = len(pack)
    if n == 0:
        raise ValueError("resume: the pack holds no cluster")
    c0 = pack.clusters[0]
    if pack.clusters != list(range(c0, c0 + n)):
        bad = next(i for i, c in enumerate(pack.clusters) if c != c0 + i)
        raise ValueError(f"resume: the pack's clusters must be consecutive ascending ids; "
                         f"clusters[{bad}] = {pack.clusters[bad]} follows {pack.clusters[bad - 1]}")
    cfg = replay_config(_abi.Config(**pack.config), c0, trace_cap=0, trace_entry_cap=0)
    cfg.update(n_clusters=n)
    return _scattered(pack, "resume", _override(cfg, overrides))


def fan_out(source, cluster, copies, **overrides):
    """A Simulator of `copies` clusters that all start as one cluster of a snapshot: `source` is a
    Simulator, whose cluster `cluster` is gathered, or a ClusterPack, of which `cluster` is the
    position in the pack (as fork() takes them). The new handle has the source's config with
    n_clusters = copies at cluster_offset = the cluster's global id g, one device and the trace
    rings off (`overrides` replace any field), is set to the pack's tick, and every cluster of it
    is scattered from the one record on the device. Philox is keyed by the global cluster id:
    cluster 0 continues bit-exactly as the original does, and cluster j is that state's future
    under id g + j -- `copies` independent futures of one state. g + copies must not exceed 2^32
    (the config's own limit)."""
    if isinstance(source, ClusterPack):
        pack, i = source, int(cluster)
        if not 0 <= i < len(pack):
            raise ValueError(f"position {i} outside the pack's {len(pack)} clusters")
    else:
        pack, i = source.gather([cluster]), 0
    copies = int(copies)
    if copies < 1:
        raise ValueError("fan_out: copies must be >= 1")
    cfg = replay_config(_abi.Config(**pack.config), pack.clusters[i], trace_cap=0,
                        trace_entry_cap=0)
    cfg.update(n_clusters=copies)
    return _scattered(pack, "fan_out", _override(cfg, overrides), [i] * copies)


def _override(cfg, overrides):
    for k in overrides:
        if k not in cfg:
            raise TypeError(f"unknown config field {k!r}")
    return dict(cfg, **overrides)


def _ids(xs):
    return [int(x["cluster"] if isinstance(x, dict) else x) for x in xs]


def split_plan(survivors, victims):
    """The (sources, targets) lists of an importance split (needs no library): victim j is to be
    overwritten with survivor j % len(survivors), so the survivors' states are spread evenly over
    the victims. Both take handle-local ids or the record dicts the queries return. Refuses (
    ValueError) an empty list of survivors, a victim that is also a survivor and a victim named
    twice; no victims gives two empty lists."""
    survivors, victims = _ids(survivors), _ids(victims)
    if not survivors:
        raise ValueError("split_plan: no survivors")
    alive, seen = set(survivors), set()
    for j, v in enumerate(victims):
        if v in alive:
            raise ValueError(f"split_plan: victims[{j}] = {v} is also a survivor")
        if v in seen:
            raise ValueError(f"split_plan: victims[{j}] = {v} is a victim twice")
        seen.add(v)
    return [survivors[j % len(survivors)] for j in range(len(victims))], victims


def split(sim, survivors, victims):
    """Respawn (importance splitting) inside one handle: overwrite the clusters `victims` of `sim`
    with copies of the clusters `survivors`, as split_plan pairs them, by one clone() on the
    device. Philox is keyed by the global cluster id, so every copy is an independent future of its
    survivor from sim's tick on. Returns the plan (sources, targets): the caller keeps the lineage.
    Violation records, counters and trace `seq` numbers are not state and are not carried: a
    victim's violation record stays the one of the cluster it was."""
    sources, targets = split_plan(survivors, victims)
    sim.clone(sources, targets)
    return sources, targets


def snapshot(sim, **overrides):
    """A new Simulator on the same GPU holding the state of every cluster of `sim` at sim.tick: a
    device-resident checkpoint, filled by one clone() with nothing passing through host memory. It
    has sim's config (`overrides` replace any field, as in resume(): with the same seed, timers,
    rates and cluster_offset it continues bit-exactly as sim does). Violation records, counters
    and trace `seq` numbers are not state and are not carried: the snapshot's start empty."""
    cfg = _override({f: getattr(sim.config, f) for f, _ in _abi.Config._fields_}, overrides)
    snap = Simulator(**cfg)
    try:
        snap.set_tick(sim.tick)
        snap.clone(range(sim.C), range(sim.C), source=sim)
    except Exception:
        snap.close()
        raise
    return snap


def rollback(sim, snap):
    """Take `sim` back to the snapshot `snap` (snapshot(sim) at an earlier tick): every cluster is
    cloned back on the device and sim's clock is set to snap.tick. sim then runs the window again
    exactly as it did the first time (a snapshot of sim's own config continues bit-exactly).
    Violation records, counters and trace `seq` numbers are not state and are not carried: sim's
    keep what the abandoned window added."""
    if sim.C != snap.C:
        raise ValueError(f"rollback: the snapshot holds {snap.C} clusters, the handle {sim.C}")
    sim.clone(range(snap.C), range(sim.C), source=snap)
    sim.set_tick(snap.tick)
