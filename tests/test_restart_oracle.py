"""Node restarts on the C oracle alone (no GPU): raftsim.restart_by_writes, the restart through
the read_* / write_* calls that the device-side restart is tested against, does what SIM_SPEC §4a
says and does a crash storm good.

The storm is tests/cases.py's `crash_storm_clients` cut to 64 clusters with the case table's own
seed (13): checked once on the oracle before these assertions were written -- at tick 20,000 it has
76 halted nodes (38 NPE, 38 OVERFLOW) in 55 clusters; 15,000 ticks after their restart `to_halted`
has grown by 7,064 against 9,770 on the unrestarted twin, and 75 of the restarted nodes hold
current_term > 1."""
import numpy as np
import pytest

import cases
import pairing
import raftsim

STORM_TICKS, AFTER = 20000, 15000


@pytest.mark.parametrize("N", [2, 5, 9])
def test_restart_by_writes_at_tick_0_changes_no_digest(N):
    cfg = dict(n_clusters=6, nodes=N, seed=7, cluster_offset=3, client_ppm=1000, commit_stream_cap=4)
    with pairing.closing(pairing.oracle(cfg), pairing.oracle(cfg)) as (h, twin):
        d0 = h.digest().copy()
        nodes0, clusters0 = h.read_nodes(), h.read_clusters()
        for c in range(h.C):
            assert raftsim.restart_by_writes(h, c, range(1, N + 1), "amnesia") == N
        assert (h.digest() == d0).all()
        assert h.read_nodes() == nodes0 and h.read_clusters() == clusters0
        assert raftsim.restart_by_writes(h, 0, []) == 0
        with pytest.raises(ValueError, match=f"node id {N + 1} outside"):
            raftsim.restart_by_writes(h, 0, [N + 1])
        # ... and the run goes on as the untouched twin's
        h.step(3000)
        twin.step(3000)
        assert (h.digest() == twin.digest()).all() and h.counters() == twin.counters()


def halted_of(h):
    """{cluster: [ids of its halted nodes]} and {fault code: nodes}."""
    halted, faults = {}, {}
    for i, r in enumerate(h.read_nodes()):
        if r["fault"]:
            halted.setdefault(i // h.N, []).append(i % h.N + 1)
            faults[r["fault"]] = faults.get(r["fault"], 0) + 1
    return halted, faults


@pytest.mark.parametrize("mode", ["amnesia", "durable"])
def test_restarted_storm_nodes_take_part_again(mode):
    cfg = cases.cfg_of("crash_storm_clients", 64)
    with pairing.closing(pairing.oracle(cfg, ticks=STORM_TICKS),
                         pairing.oracle(cfg, ticks=STORM_TICKS)) as (h, twin):
        assert (h.digest() == twin.digest()).all()
        halted, faults = halted_of(h)
        assert len(faults) >= 2 and sum(faults.values()) >= 40, faults    # a storm it is
        before = h.read_nodes()
        counters0, clusters0, digests0 = h.counters(), h.read_clusters(), h.digest().copy()
        T = h.tick
        for c, ids in halted.items():
            assert raftsim.restart_by_writes(h, c, ids, mode) == len(ids)
        # the restart itself: the records are restart_record's, nothing else moved
        after = h.read_nodes()
        for i, (b, a) in enumerate(zip(before, after)):
            c, k = divmod(i, h.N)
            if k + 1 in halted.get(c, ()):
                assert a == raftsim.restart_record(b, T, h.config, c, mode, node_id=k + 1)
                assert a["fault"] == 0 and a["req_count"] == a["res_count"] == 0
                assert T + cfg["el_base"] <= a["deadline"] < T + cfg["el_base"] + cfg["el_span"]
                assert h.read_queue(c, k + 1, 0) == [] and h.read_queue(c, k + 1, 1) == []
            else:
                assert a == b
        assert h.tick == T and h.counters() == counters0 and h.read_clusters() == clusters0
        untouched = np.array([c not in halted for c in range(h.C)])
        assert (h.digest()[untouched] == digests0[untouched]).all()
        assert (h.digest()[~untouched] != digests0[~untouched]).all()
        # 15,000 ticks on, past T + el_base + el_span: fewer messages reach halted nodes than on
        # the twin, and restarted nodes have voted or stood in elections
        h.step(AFTER)
        twin.step(AFTER)
        grown = h.counters()["to_halted"] - counters0["to_halted"]
        twin_grown = twin.counters()["to_halted"] - counters0["to_halted"]
        print(f"{mode}: to_halted grew by {grown}, on the unrestarted twin by {twin_grown}")
        assert grown < twin_grown
        end = h.read_nodes()
        risen = sum(end[c * h.N + i - 1]["current_term"] > (1 if mode == "amnesia" else
                                                            before[c * h.N + i - 1]["current_term"])
                    for c, ids in halted.items() for i in ids)
        print(f"{mode}: {risen} of {sum(map(len, halted.values()))} restarted nodes moved on in term")
        assert risen > 0
