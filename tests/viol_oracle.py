"""What the per-cluster violation records must hold, from the oracle (test infrastructure).

The oracle library has no per-cluster records, but it can produce them: Philox is keyed by the
global cluster id (SIM_SPEC D13), so a one-cluster oracle handle at cluster_offset = c is cluster c
of any larger handle, and its own viol_* counters and first_violation_tick are that cluster's
record. tests/test_violations_abi.py checks the method on the oracle alone (the per-cluster values
sum to the whole handle's counters); tests/test_gpu_violations.py holds the GPU to them.
"""
from __future__ import annotations

import helpers

KINDS = ("election", "log", "complete")
_cache = {}


def _key(cfg, n_clusters):
    return tuple(sorted(cfg.items())), n_clusters


def _handles(cfg, n_clusters, tick0=0, setup=None):
    """One-cluster handles of the first n_clusters clusters of cfg; with tick0 each is moved there
    by set_tick, then given to setup(handle) (it writes the client cursor: high_clock.setup_for),
    as high_clock.start moves the whole handle."""
    off = cfg.get("cluster_offset", 0)
    for c in range(n_clusters):
        h = helpers.oracle(**dict(cfg, n_clusters=1, cluster_offset=off + c, n_devices=1))
        if tick0:
            h.set_tick(tick0)
        if setup is not None:
            setup(h)
        yield h


def _counts(h):
    c = h.counters()
    return tuple(c["viol_" + k] for k in KINDS), c["first_violation_tick"]


def expected_records(cfg, n_clusters, ticks, tick0=0, setup=None):
    """{cluster: (first_tick, (election, log, complete))} of the clusters with any violation at
    tick `ticks` of the first n_clusters clusters of cfg. `ticks` may be a tuple of increasing
    checkpoints: then a list with one such dict per checkpoint. With tick0 the run starts there
    (see _handles) and the checkpoints are absolute ticks. Computed once per argument set."""
    points = (ticks,) if isinstance(ticks, int) else tuple(ticks)
    key = _key(cfg, n_clusters) + (points, tick0, setup is not None)
    if key not in _cache:
        out = [dict() for _ in points]
        for c, h in enumerate(_handles(cfg, n_clusters, tick0, setup)):
            for i, t in enumerate(points):
                h.step(t - h.tick)
                counts, first = _counts(h)
                if any(counts):
                    out[i][c] = (first, counts)
            h.close()
        _cache[key] = out
    res = _cache[key]
    return res[0] if isinstance(ticks, int) else res


def expected_window(cfg, n_clusters, t0, t1, step=100, tick0=0, setup=None):
    """The records of the violations counted in ticks [t0, t1) alone (what a handle whose records
    were cleared at t0 holds at t1): {cluster: ((lo, hi), counts)}, counts the one-cluster
    handle's counter delta over [t0, t1) and [lo, hi) the `step`-tick stretch in which its
    counters first moved after t0 (the first violation tick of the window lies in it). With tick0
    the run starts there (see _handles); t0 and t1 are absolute ticks."""
    key = _key(cfg, n_clusters) + ("window", t0, t1, step, tick0, setup is not None)
    if key not in _cache:
        out = {}
        for c, h in enumerate(_handles(cfg, n_clusters, tick0, setup)):
            h.step(t0 - h.tick)
            base, _ = _counts(h)
            span = None
            while h.tick < t1:
                lo = h.tick
                h.step(min(step, t1 - lo))
                if span is None and _counts(h)[0] != base:
                    span = (lo, h.tick)
            delta = tuple(a - b for a, b in zip(_counts(h)[0], base))
            if any(delta):
                out[c] = (span, delta)
            h.close()
        _cache[key] = out
    return _cache[key]


def as_records(expected, cluster_offset=0):
    """expected_records' dict in the form Simulator.violations returns its records."""
    recs = []
    for c in sorted(expected):
        first, counts = expected[c]
        rec = {"cluster": c, "global_id": cluster_offset + c, "first_tick": first}
        rec.update(zip(KINDS, counts))
        rec["kinds"] = tuple(k for k, n in zip(KINDS, counts) if n)
        recs.append(rec)
    return recs
