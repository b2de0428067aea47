"""Configs on the exact thresholds of the steady kernel's fast paths, and what a run must contain
for a parity test on them to mean something (test infrastructure).

The guards (steady_kernel.hip), with F = nodes - 1, Q = inbox_cap and the round's period
P = 2d + F - 1 + hb:
  certified paths          el_base >= P  and  hb >= 2d + F  and  Q >= F
  closed-form init election  Q >= 2F  and the two above (and D_k >= t1 + d, tlast < tend per cluster)
  per cluster              follower deadline >= nxt,  Ldl >= t0,  ta >= t0
edge_cfg puts a config on, or one off, each of the first two rows. What makes the equalities bite
is SIM_SPEC P1: in one tick an eligible message (arrival <= t) beats a timeout (t >= deadline).
With el_base == P a follower whose election draw is 0 has its deadline on the arrival of the next
append-entries; with hb == 2d the leader's deadline is on the arrival of its first response.

The helpers below read any Backend's records. The tests apply them to the oracle: they show that
a config reaches the ties (test_steady_edge_witness.py), so that the GPU comparison
(test_gpu_steady_edges.py) cannot pass without having met them.
"""
from __future__ import annotations

C_EDGE = 199            # three full waves and a partial one, as test_gpu_steady_line0.cut_cfg
VARIANTS = ("corner", "el-1", "hb-1", "hb=2d", "hb=2d-1", "Q-1", "Q2F", "Q2F-1")
LEADER, FOLLWER = 2, 3
REQ, RES = 0, 1


def edge_cfg(nodes, d, variant, clusters=C_EDGE):
    """(cfg, P) of one variant. P is computed from the variant's own hb."""
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    F = nodes - 1
    hb0 = 2 * d + F
    hb = {"hb-1": hb0 - 1, "hb=2d": 2 * d, "hb=2d-1": 2 * d - 1}.get(variant, hb0)
    P = 2 * d + F - 1 + hb
    el_base = P - 1 if variant == "el-1" else P
    Q = {"Q-1": max(1, F - 1), "Q2F": 2 * F, "Q2F-1": max(1, 2 * F - 1)}.get(variant, F)
    return dict(n_clusters=clusters, nodes=nodes, seed=100 + 10 * nodes + d, hb=hb,
                el_base=el_base, el_span=P, inbox_cap=Q, dmin=d, dmax=d), P


def cluster_settled(cl):
    """One leader, every other node a :follwer of its term (what test_gpu_steady_line0.elected
    asserts of every cluster). Returns the leader's position (0-based) or None."""
    lead = [k for k, n in enumerate(cl) if n["role"] == LEADER]
    if len(lead) != 1:
        return None
    term = cl[lead[0]]["current_term"]
    if all(n["role"] == FOLLWER and n["current_term"] == term
           for k, n in enumerate(cl) if k != lead[0]):
        return lead[0]
    return None


def settled(be):
    """(unsettled, led): the number of clusters that are not settled, and led[k] = the number of
    settled clusters whose leader is node k + 1."""
    nodes, N = be.read_nodes(), be.N
    led, unsettled = [0] * N, 0
    for c in range(be.C):
        k = cluster_settled(nodes[c * N:(c + 1) * N])
        if k is None:
            unsettled += 1
        else:
            led[k] += 1
    return unsettled, led


def deposed(be):
    """The number of settled clusters in which a non-leader still holds :leader-state: a leader
    that another leader's append-entries made a :follwer keeps it (append-entries-handler,
    core.clj:105-123, does not clear it). The steady kernel's model has leader-state on the leader
    alone, so it hands such a cluster to the general body in every launch: these bails are no
    threshold's."""
    nodes, N = be.read_nodes(), be.N
    n = 0
    for c in range(be.C):
        cl = nodes[c * N:(c + 1) * N]
        k = cluster_settled(cl)
        n += k is not None and any(x["ls_present"] for i, x in enumerate(cl) if i != k)
    return n


def ties(be):
    """(follower_ties, leader_ties) at the handle's current tick t, the tick its next step runs
    first. A follower tie: a live non-leader with deadline == t whose REQ head has arrival == t.
    A leader tie: a live leader with deadline == t whose RES head has arrival == t."""
    t, N = be.tick, be.N
    fol = lead = 0
    for i, n in enumerate(be.read_nodes()):
        if n["fault"] or n["deadline"] != t:
            continue
        which = RES if n["role"] == LEADER else REQ
        if not n["res_count" if which == RES else "req_count"]:
            continue
        q = be.read_queue(i // N, i % N + 1, which)
        if q and q[0][0] == t:
            if which == RES:
                lead += 1
            else:
                fol += 1
    return fol, lead


def late_round_timeouts(be):
    """The settled clusters in which, at the handle's current tick t, a follower's timer is due
    (deadline == t) and no request is queued for it: its round ran later than the period P that
    el_base >= P covers. (The first round after an election does: the new leader takes its
    remaining vote responses before the first append-response, max(0, F - i_L - 2d) ticks.)"""
    t, N = be.tick, be.N
    nodes = be.read_nodes()
    out = []
    for c in range(be.C):
        cl = nodes[c * N:(c + 1) * N]
        k = cluster_settled(cl)
        if k is not None and any(i != k and x["deadline"] == t and not x["req_count"]
                                 for i, x in enumerate(cl)):
            out.append(c)
    return out


def init_classes(be):
    """{single, tie, other} counts of a fresh handle's clusters (tick 0), by the sorted initial
    deadlines D: `single` when D[1] >= D[0] + d (the first candidate's request-votes arrive before
    any other timer), `tie` when D[0] == D[1], d == 1, N >= 3 and D[2] is later (the closed-form
    election's two-candidate case), `other` for the rest."""
    assert be.tick == 0
    nodes, N, d = be.read_nodes(), be.N, be.config.dmin
    out = dict(single=0, tie=0, other=0)
    for c in range(be.C):
        D = sorted(n["deadline"] for n in nodes[c * N:(c + 1) * N])
        if D[1] >= D[0] + d:
            out["single"] += 1
        elif D[0] == D[1] and d == 1 and N >= 3 and D[2] > D[1]:
            out["tie"] += 1
        else:
            out["other"] += 1
    return out


def leader_of(be, c):
    """The position (0-based) of cluster c's settled leader; asserts there is one."""
    k = cluster_settled(be.read_nodes(c, 1))
    assert k is not None, f"cluster {c} is not settled"
    return k


def next_ae_arrival(be, c):
    """(follower position, arrival) of the next append-entries at the follower after the leader of
    settled cluster c: its REQ head's arrival, or the leader's deadline + d when none is in flight."""
    lead = leader_of(be, c)
    fol = (lead + 1) % be.N
    q = be.read_queue(c, fol + 1, REQ)
    if q:
        return fol, q[0][0]
    return fol, be.read_nodes(c, 1)[lead]["deadline"] + be.config.dmin


def _set_deadline(be, c, k, deadline):
    raw = be.read_nodes_raw(c, 1)
    raw[k].deadline = deadline
    be.write_nodes(c, raw)


# Host writes of test_gpu_steady_edges.test_host_written_ties: each returns the deadline it wrote.
def write_follower_tie(be, c):
    fol, arr = next_ae_arrival(be, c)
    _set_deadline(be, c, fol, arr)               # a tie: the message wins
    return arr


def write_follower_early(be, c):
    fol, arr = next_ae_arrival(be, c)
    _set_deadline(be, c, fol, arr - 1)           # the timer wins by one tick
    return arr - 1


def write_leader_now(be, c):
    _set_deadline(be, c, leader_of(be, c), be.tick)
    return be.tick


def write_leader_next(be, c):
    _set_deadline(be, c, leader_of(be, c), be.tick + 1)
    return be.tick + 1


WRITES = dict(follower_tie=write_follower_tie, follower_early=write_follower_early,
              leader_now=write_leader_now, leader_next=write_leader_next)
WRITTEN = (5, 70, 130, 198)        # one cluster in each wave of the 199
