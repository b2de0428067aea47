"""What the steady-kernel GPU tests share (test infrastructure): they compare everything after
every step (digests, counters and the raw node records of every cluster), start from settled
clusters, and check that the steady kernel ran."""
import functools

import pairing

same = functools.partial(pairing.same, counters=True, nodes=True)
step = functools.partial(pairing.step, counters=True, nodes=True)


def elected(g, r, P):
    """One long step: every cluster elects its leader and settles on its heartbeat schedule."""
    step(g, r, 300 * P, "election step")
    nodes = r.read_nodes()
    N = r.N
    for c in range(r.C):
        cl = nodes[c * N:(c + 1) * N]
        lead = [n for n in cl if n["role"] == 2]
        assert len(lead) == 1 and all(n["role"] == 3 and n["current_term"] == lead[0]["current_term"]
                                      for n in cl if n["role"] != 2), f"cluster {c} not settled"
    # The elections' bails send auto mode through its cool-down: the launch after next reports
    # them, then two launches take the general kernel. Six launches later the steady kernel runs
    # every launch (a cluster off the fixed point's schedule may still be bailed in each).
    for i in range(6):
        step(g, r, 1, f"settle {i}")
    assert g.diag_last_bails() >= 0, "the steady kernel does not run after the elections"


def launch(g, r, nt, what, mode="always"):
    """step(), and under RAFTSIM_STEADY=always the steady kernel ran."""
    step(g, r, nt, what)
    if mode == "always":
        assert g.diag_last_bails() >= 0, f"{what}: the steady kernel did not run"
