"""The steady kernel's in-place exit (steady_kernel.hip, "the wave ends here"): a line-0 wave stores
its lines, adds its counters and ends right behind its body, while its siblings on the other paths
run on (the kernel has no workgroup barrier). After every launch the GPU is compared with the C
oracle: digests, counters and every node record. tests/test_steady_exit_witness.py shows on the
oracle alone that these runs hold the clusters they are for (steady_exit.py has the plans both
files run). Fault-free, client-free configs."""
import pytest

import pairing
import steady_band as sb
import steady_exit as sx
from cases import cut_cfg
from steady_pair import elected, launch, same

pytestmark = pytest.mark.gpu

ONE_LAUNCH = 65536       # the most ticks a launch fuses: every step below is one launch


@pytest.mark.parametrize("nodes,clusters", sx.PARTIAL)
def test_partial_waves_end_in_place(nodes, clusters):
    """64, 65, 129 and 257 clusters: the last wave of 65, 129 and 257 ends in place with 63
    inactive lanes; at 257 it is the only wave of a second workgroup. Three launches of 2P - 1."""
    cfg, P = cut_cfg(nodes, 1, clusters)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)
        for i, nt in enumerate(sx.partial_launches(P)):
            launch(g, r, nt, f"launch {i} of {nt}")


@pytest.mark.parametrize("kind", list(sx.SIBLINGS))
def test_siblings_outlive_a_line0_wave(kind, monkeypatch):
    """One workgroup of four full waves, N = 5. Before each launch the host writes one settled
    cluster: of wave 1 with its own node records (the certificate goes: that wave takes the
    two-line or the general path while waves 0, 2 and 3 end early), or a follower's deadline of a
    cluster of wave 2 onto the next tick (that cluster runs an election in the catch-up after its
    siblings have gone). The waves add to different copies of the counters: the totals are
    compared after every launch. RAFTSIM_STEADY=always: a written cluster is bailed by design,
    and every launch here is to run the steady kernel."""
    monkeypatch.setenv("RAFTSIM_STEADY", "always")
    cfg, P = cut_cfg(5, 1, sx.SIBLING_C)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)

        def check(what):
            same(g, r, what)
            assert g.diag_last_bails() >= 0, f"{what}: the steady kernel did not run"

        sx.run_siblings((g, r), P, kind, check)
        launch(g, r, 3 * P + 1, "launch of 3P + 1 after")


@pytest.mark.parametrize("clusters", sx.FORMS_CLUSTERS)
def test_the_in_place_stores_three_forms(clusters):
    """N = 5, d = 1, the full waves' clusters host-written onto two heartbeat phases three ticks
    apart (steady_band.align_full_waves): the 2P single-tick launches hold full waves in which no
    cluster, some clusters and all 64 ran an event -- no store, the predicated form, the eight
    plain stores -- each followed by the wave's counters and its end."""
    cfg, P = cut_cfg(5, 1, clusters)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)
        sb.align_full_waves((g, r), P, 1)
        same(g, r, "aligned")
        for i in range(2 * P):
            launch(g, r, 1, f"single tick {i}")


@pytest.mark.parametrize("nodes,d", sx.CUT)
def test_rare_stores_and_line_stores(nodes, d):
    """Launches of last + 1, P + 1 and 2P - 1 ticks: clusters of every leader position have a
    round in progress at the launch's start and at its end, so their waves store chunks past line
    0 and ring messages beside the line stores. A launch of one tick after each reads the rings
    and the chunks just written."""
    cfg, P = cut_cfg(nodes, d)
    with pairing.pair(cfg, dict(ticks_per_launch=ONE_LAUNCH), threads=1) as (g, r):
        elected(g, r, P)
        for i, nt in enumerate(sx.cut_launches(nodes, d, P)):
            launch(g, r, nt, f"launch {i} of {nt}")
