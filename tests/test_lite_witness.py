"""CPU witness for the fault-free parity cases (test_gpu_parity.py CASES `lite_n6` ...
`traced_lite_n6`): the general body's LITE instance at N = 6..9, and the Spec-Raft and traced
kernels in handles with DevSim::lite set.

Which kernel a launch runs cannot be observed from outside, and a fault-free run that elects its
leaders once and then only exchanges heartbeats exercises little of it. These tests show on the C
oracle alone that each case reaches the states it is there for: ring overflows with leaders
elected all the same, a run in which every vote is lost, elections that keep interrupting the
rounds, NPE halts and messages to halted nodes, and Spec-Raft runs without halt or violation. A
change of a case's seed or timers that turns it into an idle run fails here, without a GPU.

MEASURED records what the oracle reached in 20,000 ticks (deterministic). Every condition asserted
is an inequality that leaves at least a factor of 2 below the measured figure, except the two
that hold by construction (no leader with one-slot inboxes; no halt or violation in Spec-Raft).
No figure here comes from the GPU.
"""
import pytest

import pairing
from cases import CASES

MEASURED = {
    "lite_n6": dict(leaders=700, ev_heartbeat=44000),
    "lite_n7_d4": dict(leaders=700),
    "lite_n8_elections": dict(leaders=21018, halt_npe=2, to_halted=52),
    "lite_n9_inbox4": dict(leaders=510, overflow=197000),
    "lite_n6_inbox1": dict(leaders=0, ev_timeout=184000, overflow=740000),
    "lite_n9_odd_launches": dict(leaders=400, ev_heartbeat=98000),
    "lite_n7_short_round": dict(leaders=12893, halt_npe=1979, to_halted=2600000),
    "spec_lite_n5": dict(leaders=700),
    "spec_lite_n6_elections": dict(leaders=16999),
    "spec_lite_n9_inbox4": dict(leaders=512, overflow=203000),
    "traced_lite_n6": dict(leaders=256, ev_heartbeat=106000),
}


@pytest.mark.parametrize("name", list(MEASURED))
def test_case_reaches_its_states(name):
    cfg = CASES[name]
    C = cfg["n_clusters"]
    # fault-free, client-free, fixed delay: DevSim::lite is set
    assert not any(cfg.get(k) for k in ("client_ppm", "drop_ppm", "dup_ppm", "part_ppm"))
    assert cfg.get("dmin", 1) == cfg.get("dmax", 1)
    r = pairing.oracle(cfg)
    r.step(20000)
    c = r.counters()
    r.close()
    print(name, {k: v for k, v in c.items() if v})
    assert c["ev_heartbeat"] > 0 or c["ev_timeout"] > C
    if name.endswith("_inbox4"):
        assert c["overflow"] > 0 and c["leaders"] >= C * 9 // 10
    if name == "lite_n6_inbox1":
        assert c["leaders"] == 0 and c["overflow"] > 0
    if name in ("lite_n8_elections", "lite_n7_short_round"):
        assert c["halt_npe"] > 0 and c["to_halted"] > 0
    if name.startswith("spec_lite_"):
        assert cfg["variant_flags"] == 2
        assert not [k for k in c if k.startswith(("halt_", "viol_")) and c[k]]
    if name.endswith("_elections"):
        assert c["leaders"] > 10 * C
    if name.startswith("traced_"):
        assert cfg["trace_cap"] and c["ev_heartbeat"] + c["ev_timeout"] > C * cfg["nodes"] * 16
    # the figures the cases were chosen by, as floors of half
    for k, m in MEASURED[name].items():
        assert c[k] >= m // 2, (k, c[k], m)
