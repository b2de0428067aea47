"""What tests/test_gpu_steady_exit.py runs and tests/test_steady_exit_witness.py vouches for: the
plans around the steady kernel's in-place exit (steady_kernel.hip: a line-0 wave stores its lines,
adds its counters and ends where its body ends, while the waves on the other paths run on), and,
from the oracle's node records alone, what the clusters of a launch are.

Every function that steps takes a list of backends and does the same to each, so the GPU test runs
it on (gpu, oracle) and the witness on (oracle,); `check(what)` is called after every launch."""

# ---- partial waves: a line-0 wave ends in place with inactive lanes; at 257 clusters the second
# workgroup holds one wave of one lane
PARTIAL = [(nodes, clusters) for nodes in (2, 5) for clusters in (64, 65, 129, 257)]


def partial_launches(P):
    return [2 * P - 1] * 3


# ---- siblings that outlive a line-0 wave: one workgroup of four waves, one of them off the line-0
# path in every launch
SIBLING_C = 256


def rewrite_same(be, c):
    """The cluster's node records written back as read: the certificate goes, the state stays."""
    be.write_nodes(c, be.read_nodes_raw(c, 1))


def rewrite_deadline(be, c):
    """One follower's timer onto the next tick: it times out in the launch that follows."""
    raw = be.read_nodes_raw(c, 1)
    lead = next(i for i in range(be.N) if raw[i].role == 2)
    raw[(lead + 1) % be.N].deadline = be.tick + 1
    be.write_nodes(c, raw)


# kind -> (the host write, the wave of the workgroup it lands in)
SIBLINGS = {"same_records": (rewrite_same, 1), "follower_deadline": (rewrite_deadline, 2)}


def sibling_launches(P, wave):
    """(the cluster written before the launch, the launch's ticks): a cluster of `wave` that no
    other launch writes, single ticks and launches longer than a round."""
    return [(64 * wave + (11 * i + 3) % 64, 1 if i % 3 else P + 1) for i in range(P + 2)]


def cluster(nodes, N, c):
    return nodes[c * N:(c + 1) * N]


def settled(cl):
    """One leader, every other node its follower in its term."""
    lead = [n for n in cl if n["role"] == 2]
    return len(lead) == 1 and all(n["role"] == 3 and n["current_term"] == lead[0]["current_term"]
                                  for n in cl if n["role"] != 2)


def run_siblings(bes, P, kind, check):
    """Before every launch the host writes one settled cluster (asserted on the last backend, the
    oracle); returns the clusters written."""
    op, wave = SIBLINGS[kind]
    ref, written = bes[-1], []
    for i, (c, nt) in enumerate(sibling_launches(P, wave)):
        assert settled(ref.read_nodes(c, 1)), f"launch {i}: cluster {c} is not settled"
        for be in bes:
            op(be, c)
        for be in bes:
            be.step(nt)
        check(f"{kind}: launch {i} of {nt} ticks after the write of cluster {c}")
        written.append(c)
    return written


# ---- the in-place store's three forms: steady_band.align_full_waves at these cluster counts, then
# 2P single-tick launches (no store, the predicated form, the eight plain stores)
FORMS_CLUSTERS = [64, 129]

# ---- rare stores (chunks past line 0, ring messages) and the line stores of the same wave
CUT = [(nodes, d) for nodes in (3, 5) for d in (1, 3)]


def cut_launches(nodes, d, P):
    """last + 1, P + 1 and 2P - 1 ticks, each followed by one tick that reads the rings and the
    chunks past line 0 the launch before it wrote."""
    last = 2 * d + (nodes - 1) - 1
    return [last + 1, 1, P + 1, 1, 2 * P - 1, 1]


def in_round(cl):
    """A round in progress: the append-entries in flight or responses queued at the leader."""
    return any(n["req_count"] or n["res_count"] for n in cl)


def leaders_in_round(be):
    """The leader positions (0 .. N - 1) of the clusters with a round in progress now."""
    nodes, N = be.read_nodes(), be.N
    out = set()
    for c in range(be.C):
        cl = cluster(nodes, N, c)
        if in_round(cl):
            out |= {i for i, n in enumerate(cl) if n["role"] == 2}
    return out
