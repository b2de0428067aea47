"""The band form of the steady kernel's line-0 body (steady_kernel.hip: the band test in the
decision, rounds() with K from one comparison, line 0 dirty by "ran an event", the full-wave line
stores): launches on both sides of rho, the first heartbeat outside the band, and full, partial
and mixed waves. After every launch the GPU is compared with the C oracle: digests, counters and
every node record. tests/test_steady_band_witness.py shows on the oracle alone that these runs hold
the clusters they are for (steady_band.py has the plans both files run)."""
import pytest

import pairing
import steady_band as sb
from cases import cut_cfg
from steady_pair import elected, launch, same

pytestmark = pytest.mark.gpu

ONE_LAUNCH = 65536       # the most ticks a launch fuses: every step below is one launch


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("nodes", [2, 3, 4, 5])
def test_both_sides_of_rho(nodes, d):
    """One launch each of last, last + 1, last + 2, last + P - 1, last + P, last + P + 1, 2P + last
    and 5P + last + 1 ticks: K1 = 0, then rho = 0, 1, P - 2 and P - 1, with clusters at
    delta <= rho (K1 rounds) and delta > rho (K1 - 1) in the same waves."""
    cfg, P = sb.band_cfg(nodes, d)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)
        for nt in sb.rho_launches(nodes, d, P):
            launch(g, r, nt, f"launch of {nt}")


@pytest.mark.parametrize("nodes,d", [(5, 2), (3, 1)])
def test_first_value_outside_the_band(nodes, d, monkeypatch):
    """set_tick moves the clock by one tick under the certificates. Back by one, the clusters at
    delta = P - 1 stand at delta = P, the first value outside the band, and share their waves with
    clusters inside it: the wave leaves the line-0 body for the two-line path. Back by P - 1 more,
    then forward by one (heartbeats before t0 fail the unsigned test). RAFTSIM_STEADY=always: a
    moved clock bails clusters by design, and every launch here is to run the steady kernel."""
    monkeypatch.setenv("RAFTSIM_STEADY", "always")
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)
        for be in (g, r):
            be.set_tick(be.tick - 1)
        launch(g, r, 2 * P + 1, "2P + 1 after the clock went back by 1")
        for be in (g, r):
            be.set_tick(be.tick - (P - 1))
        launch(g, r, P, "P after the clock went back by P - 1")
        launch(g, r, 3 * P + 1, "3P + 1 after the clock went back by P - 1")
        for be in (g, r):
            be.set_tick(be.tick + 1)
        launch(g, r, 2 * P, "2P after the clock went forward by 1")


@pytest.mark.parametrize("clusters", [64, 65, 129])
def test_full_partial_and_mixed_waves(clusters):
    """N = 5, d = 1 with one full wave, a full wave and one cluster, two full waves and one cluster.
    The full waves' clusters are written onto two heartbeat phases three ticks apart, so the 2P
    single-tick launches hold full waves in which no cluster, some clusters and every cluster ran
    an event (no store, the predicated stores, the unpredicated ones); the partial wave takes the
    predicated stores throughout. Then 3P + 1 ticks: every cluster of every wave is dirty."""
    cfg, P = cut_cfg(5, 1, clusters)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)
        sb.align_full_waves((g, r), P, 1)
        same(g, r, "aligned")
        for i in range(2 * P):
            launch(g, r, 1, f"single tick {i}")
        launch(g, r, 3 * P + 1, "launch of 3P + 1")
