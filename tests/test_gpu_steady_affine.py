"""The steady kernel's affine step (csrc/fixed_point_affine.hpp, rs::rounds): a launch's K
whole heartbeat rounds as one multiply-add per trace hash, for the two values of K a launch holds
for clusters on the schedule, and the loop over rounds for every other K. After every launch the
GPU is compared with the C oracle: digests, counters and every node record."""
import pytest

import helpers
import pairing
from cases import cut_cfg
from steady_pair import elected, launch, same, step

pytestmark = pytest.mark.gpu

ONE_LAUNCH = 65536       # the most ticks a launch fuses: every step below is one launch


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("nodes", [2, 3, 4, 5])
def test_k_sweep(nodes, d):
    """Launches of P - 1 ticks (K = 0 for every cluster), 2P (K = 1 or 2), 3P + 1 (the lanes of a
    wave on both counts of the band), 17P + 5 and 1000P + 3 (the doubling's longer chains)."""
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)
        for nt in (P - 1, 2 * P, 3 * P + 1, 17 * P + 5, 1000 * P + 3):
            assert nt <= ONE_LAUNCH
            launch(g, r, nt, f"launch of {nt}")


@pytest.mark.parametrize("nodes,d", [(5, 2), (3, 1)])
def test_outside_the_band(nodes, d, monkeypatch):
    """set_tick moves the clock under the certificates: back by 5P, every cluster's next heartbeat
    is five periods past the launch's start, so its K is five below the band's (the loop over
    rounds runs); forward by 5, heartbeats and deadlines lie in the past. A moved clock bails
    clusters by design, and in auto mode more than C/16 bails send the next launches to the general
    kernel (a choice of speed): the handle is created with RAFTSIM_STEADY=always, so that every
    launch here does run the steady kernel, whatever it bailed before."""
    monkeypatch.setenv("RAFTSIM_STEADY", "always")
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)
        launch(g, r, 2 * P + 3, "on the schedule")
        for be in (g, r):
            be.set_tick(be.tick - 5 * P)
        launch(g, r, 2 * P, "2P after the clock went back")
        launch(g, r, 9 * P + 1, "9P + 1 after the clock went back")
        for be in (g, r):
            be.set_tick(be.tick + 5)
        launch(g, r, 3 * P, "3P after the clock went forward")
        launch(g, r, 4 * P + 1, "after")


def test_near_the_horizon():
    """The whole run ends within a few hundred ticks of the last tick a step may reach (SIM_SPEC
    D1: tick + n + the longest timer < 2^32 - 1): the affine step's products of ticks just below
    2^32 are the event-by-event hash's."""
    cfg, P = cut_cfg(5, 2)
    longest = max(cfg["hb"], cfg["el_base"] + cfg["el_span"], cfg["dmax"])
    total = 300 * P + 6 + (P + 1) + 40 * P             # elected(), then the two launches
    top = 2 ** 32 - 1 - longest - 1                    # the last tick a step may end at
    start = top - 150 - total
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        for be in (g, r):
            be.set_tick(start)
        elected(g, r, P)
        launch(g, r, P + 1, "P + 1")
        launch(g, r, 40 * P, "40P")
        assert g.tick == r.tick == top - 150
        with pytest.raises(helpers.RaftSimError):
            g.step(152)


def test_default_timers():
    """Default timers (hb 3000: P = 3006). One handle fuses up to 65,536 ticks: four launches of
    10,000 (K = 3 or 4), then one of 65,536 (K = 21 or 22). A second handle runs the same ticks
    in launches of at most 3,500 (K = 0 or 1 or 2) and ends with no bailed cluster."""
    cfg = dict(n_clusters=256, nodes=5, seed=42)
    a = helpers.gpu(**cfg, ticks_per_launch=ONE_LAUNCH)
    b = helpers.gpu(**cfg, ticks_per_launch=3500)
    r = helpers.oracle(**cfg)
    helpers.oracle_idle_skip(r, True)
    for i in range(4):
        step(a, r, 10000, f"step {i} of 10000")
        assert a.diag_last_bails() >= 0
        b.step(10000)
        same(b, r, f"step {i} in launches of 3500")
    step(a, r, 65536, "one launch of 65536")
    assert a.diag_last_bails() >= 0
    b.step(10000)
    r2 = helpers.oracle(**cfg)
    helpers.oracle_idle_skip(r2, True)
    r2.step(50000)
    same(b, r2, "50000 ticks in launches of 3500")
    assert b.diag_last_bails() == 0
