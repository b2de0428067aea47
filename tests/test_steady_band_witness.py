"""CPU witness for test_gpu_steady_band.py: on the C oracle alone, the runs of that file hold the
clusters they are for. A change of a seed, a timer or a launch length that moves them off the
band's edges fails here, without a GPU.

  * both sides of rho: before every launch with 0 <= rho < P - 1 some cluster stands at
    delta = rho (it runs K1 whole rounds) and some cluster at delta = rho + 1 (K1 - 1);
  * the first value outside the band: before the clock goes back by one tick some cluster stands
    at delta = P - 1;
  * full, partial and mixed waves: over the single-tick launches some full wave has no cluster
    that ran an event, some full wave has some, and some full wave has all 64."""
import pytest

import helpers
import pairing
import steady_band as sb
from cases import cut_cfg


def settle(r, P):
    """What elected() of test_gpu_steady_line0 steps."""
    r.step(300 * P)
    for _ in range(6):
        r.step(1)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("nodes", [2, 3, 4, 5])
def test_clusters_on_both_sides_of_rho(nodes, d):
    cfg, P = sb.band_cfg(nodes, d)
    with pairing.oracle(cfg) as r:
        settle(r, P)
        for nt in sb.rho_launches(nodes, d, P):
            dl = sb.deltas(r, d, cfg["hb"], P)
            assert all(0 <= x < P for x in dl), f"nt {nt}: a cluster off the schedule"
            K1, rho = sb.band_of(nodes, d, P, nt)
            print(f"N={nodes} d={d} nt={nt}: K1 {K1} rho {rho}, at rho {dl.count(rho)}, "
                  f"at rho + 1 {dl.count(rho + 1) if rho is not None else '-'}")
            if rho is not None and rho < P - 1:
                assert dl.count(rho) >= 1 and dl.count(rho + 1) >= 1, (nt, rho)
            r.step(nt)


@pytest.mark.parametrize("nodes,d", [(5, 2), (3, 1)])
def test_a_cluster_at_the_bands_last_value(nodes, d):
    cfg, P = cut_cfg(nodes, d)
    with pairing.oracle(cfg) as r:
        settle(r, P)
        dl = sb.deltas(r, d, cfg["hb"], P)
        print(f"N={nodes} d={d}: {dl.count(P - 1)} clusters at delta = P - 1")
        assert dl.count(P - 1) >= 1


@pytest.mark.parametrize("clusters", [64, 65, 129])
def test_waves_of_all_three_kinds(clusters):
    cfg, P = cut_cfg(5, 1, clusters)
    with helpers.oracle(**cfg) as r:
        settle(r, P)
        sb.align_full_waves((r,), P, 1)
        kinds = set()
        before = r.read_nodes()
        for _ in range(2 * P):
            r.step(1)
            after = r.read_nodes()
            kinds |= sb.wave_kinds(sb.ran_event(before, after, r.N))
            before = after
        assert kinds == {"none", "some", "all"}, kinds
