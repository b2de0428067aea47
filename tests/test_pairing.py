"""The pair harness (tests/pairing.py) on two oracle handles: what same() accepts, what it
refuses and what the refusal says, and that pair() closes its handles."""
import re

import pytest

import helpers
import pairing

CFG = dict(n_clusters=4, nodes=3, seed=7, hb=10, el_base=20, el_span=20, client_ppm=50000,
           log_cap=32, drop_ppm=50000, dmin=1, dmax=4)
TICKS = 200


def two(cfg_b=CFG):
    """Two oracle handles, the second of cfg_b, closed on exit."""
    return pairing.closing(pairing.oracle(CFG, threads=1), pairing.oracle(cfg_b, threads=1))


def test_equal_handles_pass_every_check():
    with two() as (a, b):
        pairing.same(a, b, "fresh", counters=True, nodes=True)
        pairing.run(a, b, pairing.chunks(TICKS, 90), counters=True, nodes=True)
        assert a.tick == b.tick == TICKS and pairing.same_counters(a, b)["leaders"] > 0


def test_another_seed_is_a_digest_mismatch_with_the_cluster_diff():
    with two(dict(CFG, seed=8)) as (a, b):
        with pytest.raises(AssertionError) as e:
            pairing.step(a, b, TICKS, "seeds 7 and 8")
        msg = str(e.value)
        bad = (a.digest() != b.digest()).nonzero()[0]
        assert len(bad) and f"seeds 7 and 8 (tick {TICKS}): {len(bad)} of 4 clusters differ" in msg
        assert f"first {bad[0]}:" in msg
        assert re.search(r"^  node \d \w+: .* != ", msg, re.M), msg


def test_a_step_ahead_is_a_clock_mismatch():
    with two() as (a, b):
        a.step(TICKS)
        b.step(TICKS + 1)
        with pytest.raises(AssertionError, match=f"clocks differ: {TICKS} != {TICKS + 1}"):
            pairing.same(a, b, "ahead")


def test_equal_digests_with_other_counters_are_refused_with_the_keys():
    """The second handle is moved to the first one's tick and given its state: the digests agree,
    the counters of the ticks it never ran do not."""
    with two() as (a, b):
        a.step(TICKS)
        b.set_tick(TICKS)
        b.write_nodes(0, a.read_nodes_raw())
        b.write_clusters(0, a.read_clusters())
        for c in range(a.C):
            for i in range(1, a.N + 1):
                b.write_arena(c, i, a.read_arena(c, i))
                for w in (0, 1):
                    b.write_queue(c, i, w, a.read_queue(c, i, w))
        pairing.same(a, b, "restored")
        with pytest.raises(AssertionError, match="counters differ") as e:
            pairing.same(a, b, "restored", counters=True)
        assert f"'node_ticks': ({a.C * a.N * TICKS}, 0)" in str(e.value)


def test_pair_closes_both_handles_when_its_body_raises():
    with pytest.raises(RuntimeError, match="in the body"):
        with pairing.pair(CFG, threads=1, make=helpers.oracle) as (g, r):
            assert g._h and r._h
            raise RuntimeError("in the body")
    assert g._h is None and r._h is None
