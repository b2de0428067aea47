"""One handle under test against the C oracle (test infrastructure): the oracle handle with its
thread count, a pair of handles that is closed whatever the test does, and the one comparison of
two handles after a step."""
import contextlib

import numpy as np

import helpers


def oracle(cfg, threads=None, ticks=0, idle_skip=False):
    """An oracle handle of cfg on every CPU this process may use, or on at most `threads` of them
    (1: the library's own default), stepped `ticks` ticks."""
    r = helpers.oracle(**cfg)
    n = helpers.cpu_threads()
    helpers.oracle_threads(r, n if threads is None else min(n, threads))
    if idle_skip:
        helpers.oracle_idle_skip(r, True)
    if ticks:
        r.step(ticks)
    return r


@contextlib.contextmanager
def closing(*handles):
    """Handles the caller made itself (fuzz.load_batch, high_clock.start), closed on exit."""
    try:
        yield handles
    finally:
        for h in handles:
            h.close()


@contextlib.contextmanager
def pair(cfg, gpu_cfg=None, threads=None, make=helpers.gpu, idle_skip=False):
    """(g, r): make(**cfg, **gpu_cfg) and the oracle of cfg, both closed on exit, after a failure
    too. gpu_cfg: keys that only g gets (ticks_per_launch, schedule, ...)."""
    with closing(make(**cfg, **(gpu_cfg or {}))) as (g,):
        with closing(oracle(cfg, threads, idle_skip=idle_skip)) as (r,):
            yield g, r


def same(g, r, what, counters=False, nodes=False, bisect=None, lo=None):
    """The clocks and every cluster's digest are equal; counters: every counter too; nodes: the raw
    node records too. bisect: the handles' config, fresh handles only: on a digest mismatch the
    first differing cluster is re-run alone, tick by tick, up to the first divergent tick. lo: r
    holds g's clusters [lo, lo + r.C) alone, and only those are compared."""
    assert g.tick == r.tick, f"{what}: clocks differ: {g.tick} != {r.tick}"
    bad = np.nonzero((g.digest() if lo is None else g.digest(lo, r.C)) != r.digest())[0]
    if len(bad):
        c = int(bad[0])
        msg = (f"{what} (tick {r.tick}): {len(bad)} of {r.C} clusters differ, first "
               f"{(lo or 0) + c}:\n" + helpers.describe_cluster_diff(g, r, (lo or 0) + c, c))
        if bisect is not None:
            msg += "\n" + helpers.bisect_divergence(bisect, bisect.get("cluster_offset", 0) + c,
                                                    r.tick, helpers.gpu, helpers.oracle)
        raise AssertionError(msg)
    if counters:
        same_counters(g, r, what)
    if nodes:
        gw, rw = g.read_nodes_raw(), r.read_nodes_raw()
        if bytes(gw) != bytes(rw):
            for i, (x, y) in enumerate(zip(gw, rw)):
                x, y = x.as_dict(g.N), y.as_dict(r.N)
                assert x == y, f"{what}: cluster {i // g.N} node {i % g.N + 1}: {x} != {y}"


def same_counters(g, r, what="counters"):
    """Every counter is equal (same(counters=True) without the digests); returns them."""
    cg, cr = g.counters(), r.counters()
    assert cg == cr, (f"{what}: counters differ (g, r): "
                      f"{ {k: (cg[k], cr.get(k)) for k in cg if cg[k] != cr.get(k)} }")
    return cg


def step(g, r, n, what=None, **same_flags):
    """Step both handles n ticks, then same()."""
    g.step(n)
    r.step(n)
    same(g, r, what or f"step of {n}", **same_flags)


def chunks(ticks, n):
    """`ticks` in steps of n, the last one shorter where n does not divide them."""
    return [n] * (ticks // n) + [ticks % n] * bool(ticks % n)


def run(g, r, chunks, what="chunk", **same_flags):
    """step() over `chunks` (tick counts)."""
    for i, n in enumerate(chunks):
        step(g, r, n, f"{what} {i} of {n} ticks", **same_flags)
