"""CPU witness for test_gpu_steady_exit.py: on the C oracle alone, the runs of that file hold the
clusters they are for. A change of a seed, a timer or a launch length that empties them fails here,
without a GPU.

  * siblings: every cluster the host writes is settled when it is written, lies in the wave the
    plan names, and no cluster is written twice; every cluster whose follower's deadline was
    written onto the next tick has a new term after the launches, and no cluster that was written
    with its own records has;
  * the three forms: every full wave of every single-tick launch is classed by how many of its 64
    clusters ran an event: none (no store), some (the predicated form) or all (the eight plain
    stores). A full wave takes one form per launch, so one launch cannot hold the three: every
    launch is asserted to hold as many classed waves as the shard has full waves, and the launches
    together to hold every form at every count of clusters;
  * rare stores: before and after every launch of the plan some cluster has a round in progress,
    and among those clusters every leader position 0 .. N - 1 occurs.
Every launch and every cluster is looked at: nothing is sampled."""
import pytest

import pairing
import steady_band as sb
import steady_exit as sx
from cases import cut_cfg


def settle(r, P):
    """What elected() of steady_pair steps."""
    r.step(300 * P)
    for _ in range(6):
        r.step(1)


@pytest.mark.parametrize("kind", list(sx.SIBLINGS))
def test_the_written_clusters_are_settled(kind):
    cfg, P = cut_cfg(5, 1, sx.SIBLING_C)
    wave = sx.SIBLINGS[kind][1]
    with pairing.closing(pairing.oracle(cfg, threads=1)) as (r,):
        settle(r, P)
        nodes = r.read_nodes()
        assert all(sx.settled(sx.cluster(nodes, r.N, c)) for c in range(r.C)), "before the writes"
        written = [c for c, _ in sx.sibling_launches(P, wave)]
        assert len(set(written)) == len(written) and all(c // 64 == wave for c in written)
        term = lambda c: max(n["current_term"] for n in r.read_nodes(c, 1))  # noqa: E731
        before = {c: term(c) for c in written}
        # run_siblings asserts `settled` for every cluster as it is written
        assert sx.run_siblings((r,), P, kind, lambda what: None) == written
        r.step(P)
        rose = [c for c in written if term(c) > before[c]]
        print(f"{kind}: wrote {written}; a new term in {rose}")
        # a timed-out follower starts an election (a new term); a cluster's own records change nothing
        assert rose == (written if kind == "follower_deadline" else [])


@pytest.mark.parametrize("clusters", sx.FORMS_CLUSTERS)
def test_waves_of_all_three_kinds(clusters):
    cfg, P = cut_cfg(5, 1, clusters)
    with pairing.closing(pairing.oracle(cfg, threads=1)) as (r,):
        settle(r, P)
        sb.align_full_waves((r,), P, 1)
        per_launch = []
        before = r.read_nodes()
        for _ in range(2 * P):
            r.step(1)
            after = r.read_nodes()
            ev = sb.ran_event(before, after, r.N)
            per_launch.append([sb.wave_kinds(ev[64 * w:64 * w + 64]).pop() for w in range(r.C // 64)])
            before = after
        print(f"{clusters} clusters:", per_launch)
        assert all(len(k) == clusters // 64 for k in per_launch), "a full wave was not classed"
        assert {x for k in per_launch for x in k} == {"none", "some", "all"}


@pytest.mark.parametrize("nodes,d", sx.CUT)
def test_every_leader_position_in_a_cut_round(nodes, d):
    cfg, P = cut_cfg(nodes, d)
    every = set(range(nodes))
    with pairing.closing(pairing.oracle(cfg, threads=1)) as (r,):
        settle(r, P)
        for i, nt in enumerate(sx.cut_launches(nodes, d, P)):
            at_start = sx.leaders_in_round(r)
            r.step(nt)
            at_end = sx.leaders_in_round(r)
            print(f"N={nodes} d={d} launch {i} of {nt}: leader positions in a round at the start "
                  f"{sorted(at_start)}, at the end {sorted(at_end)}")
            assert at_start == every and at_end == every, (i, nt)
