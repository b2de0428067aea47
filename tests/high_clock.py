"""Runs at high clocks (test infrastructure; tests/test_high_clock_oracle.py on the CPU,
tests/test_gpu_high_clock.py on the GPU).

The clock is a 32-bit absolute tick and a handle may resume at any tick (raft_sim_set_tick), up to
the horizon of SIM_SPEC D1: a step may end at last_end(cfg) = 2^32 - 2 - longest(cfg) at the
latest. Every run here starts from a fresh handle moved to a base tick T0, so every init-node
deadline is overdue and all N timers fire together at T0 (a legal state). The three bases:

  LOW            50,000: the control. A failure there points at the overdue-fresh start, a failure
                 only at a high base at the clock.
  SIGN(total, s) 2^31 - total // 2 - s: the run crosses 2^31 in its middle. s = 0 puts a launch
                 boundary on 2^31 exactly (total a multiple of twice the launch), s = 7 puts 2^31
                 inside a launch.
  TOP(cfg, total) last_end(cfg) - total: the run's last step ends on the last tick a step may end at.
"""
import numpy as np

import helpers
import pairing
import pyref

LOW = 50_000
BASES = ("low", "sign0", "sign7", "top")
_DEFAULTS = pyref.default_config()


def longest(cfg):
    """The longest timer or delay of cfg, with the defaults filled in (SIM_SPEC D1)."""
    c = dict(_DEFAULTS, **cfg)
    return max(c["hb"], c["el_base"] + c["el_span"], c["dmax"])


def last_end(cfg):
    """The last tick a step may end at: one more tick is refused with the 2^32-1 message."""
    return 2 ** 32 - 2 - longest(cfg)


def SIGN(total, skew=0):
    return 2 ** 31 - total // 2 - skew


def TOP(cfg, total):
    return last_end(cfg) - total


def base_tick(base, cfg, total):
    """T0 of a run of `total` ticks at the base named `base` (one of BASES)."""
    if base == "low":
        return LOW
    if base == "top":
        return TOP(cfg, total)
    return SIGN(total, {"sign0": 0, "sign7": 7}[base])


def first_on_tick(t, P, B):
    """The first tick >= t inside a client burst window (bursts of B ticks at the start of every
    P; P = 0: every tick). 2^32 - 1 (never) when that tick does not fit the clock."""
    if P == 0:
        return t
    if pyref.on_tick(pyref.on_index(t, P, B), P, B) == t:          # t % P < B
        return t
    return pyref.on_tick((t // P + 1) * B, P, B)


def cursor(cfg, T0, gid):
    """The client cursor start() writes for the cluster with global id `gid`."""
    P, B = cfg.get("client_period", 0), cfg.get("client_burst", 0)
    return dict(hwm=(0, 0, 0), client_next=first_on_tick(T0 + 1 + 3 * gid, P, B),
                client_count=gid)


def py_clusters(**cfg):
    """`make` for start(): the clusters of cfg as a list of pyref.PyCluster."""
    off = cfg.get("cluster_offset", 0)
    return [pyref.PyCluster(helpers.py_config(**cfg), off + c) for c in range(cfg["n_clusters"])]


def start(make, cfg, T0):
    """make(**cfg) moved to T0: set_tick, and where client_ppm is set every cluster's cursor is
    written too (after set_tick no injection comes otherwise). `make` gives an oracle handle, a
    GPU handle or a list of PyClusters (their clock is the argument of step: only the cursor)."""
    h = make(**cfg)
    clients = bool(cfg.get("client_ppm"))
    if isinstance(h, list):
        for pc in h:
            if clients:
                cur = cursor(cfg, T0, pc.gid)
                pc.hwm, pc.client_next, pc.client_count = (cur["hwm"], cur["client_next"],
                                                           cur["client_count"])
        return h
    h.set_tick(T0)
    if clients:
        off = cfg.get("cluster_offset", 0)
        h.write_clusters(0, [cursor(cfg, T0, off + c) for c in range(h.C)])
    return h


def setup_for(cfg, T0):
    """What start() does after set_tick, as the `setup(handle)` of helpers.burst_witness and
    viol_oracle (None where no cursor is written)."""
    if not cfg.get("client_ppm"):
        return None

    def setup(h):
        off = h.config.cluster_offset
        h.write_clusters(0, [cursor(cfg, T0, off + c) for c in range(h.C)])
    return setup


def oracle(**cfg):
    """`make` for start(): the oracle handle of cfg on every CPU."""
    return pairing.oracle(cfg)


def pair(cfg, T0):
    """(g, r): the GPU handle and the oracle handle of cfg, both moved to T0 by start() and closed
    on exit."""
    return pairing.closing(start(helpers.gpu, cfg, T0), start(oracle, cfg, T0))


def refused_at_the_end(h, cfg):
    """h stands on last_end(cfg): one more tick is refused, nothing changes, step(0) works."""
    import pytest

    assert h.tick == last_end(cfg)
    before = h.digest()
    with pytest.raises(helpers.RaftSimError, match=r"2\^32"):
        h.step(1)
    assert h.tick == last_end(cfg) and np.array_equal(h.digest(), before)
    h.step(0)
    assert np.array_equal(h.digest(), before)
