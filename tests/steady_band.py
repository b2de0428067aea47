"""What tests/test_gpu_steady_band.py runs and tests/test_steady_band_witness.py vouches for: the
launch plans around the steady kernel's band (fixed_point_affine.hpp, Band) and, from the oracle's
node records alone, where each cluster stands in it.

A cluster on the fixed point's schedule has its first heartbeat of a launch at th = t0 + delta,
0 <= delta < P; with last = 2d + F - 1 and a launch of nt > last ticks, R = nt - last - 1,
K1 = R / P + 1 and rho = R % P, it runs K1 whole rounds when delta <= rho and K1 - 1 otherwise.
Every function that steps takes a list of backends and does the same to each, so the GPU test runs
it on (gpu, oracle) and the witness on (oracle,)."""
from cases import cut_cfg

C_BAND = 199
# (nodes, d) -> clusters, where 199 do not put a cluster on both sides of every rho below
CLUSTERS = {}


def band_cfg(nodes, d, clusters=None):
    cfg, P = cut_cfg(nodes, d, clusters or CLUSTERS.get((nodes, d), C_BAND))
    return cfg, P


def rho_launches(nodes, d, P):
    """Launch lengths on both sides of rho: K1 = 0; then rho = 0, 1, P - 2, P - 1 at K1 = 1;
    rho = 0 and P - 1 at K1 = 2; rho = 0 at K1 = 6."""
    last = 2 * d + (nodes - 1) - 1
    return [last, last + 1, last + 2, last + P - 1, last + P, last + P + 1, 2 * P + last,
            5 * P + last + 1]


def band_of(nodes, d, P, nt):
    """(K1, rho) of a launch of nt ticks; rho None when no delta leaves the band's upper count."""
    last = 2 * d + (nodes - 1) - 1
    if nt <= last:
        return 0, None
    R = nt - last - 1
    return R // P + 1, R % P


def deltas(r, d, hb, P):
    """delta = (the first heartbeat a launch from r.tick would give rounds()) - r.tick, for every
    cluster, from the node records: the leader's deadline is that heartbeat when no round is in
    progress; with the append-entries in flight the round's heartbeat was at deadline - hb; with
    j0 of F responses taken it was at deadline - hb - (2d + j0 - 1) (j0 = 0: deadline - hb)."""
    nodes, N, t0 = r.read_nodes(), r.N, r.tick
    F = N - 1
    out = []
    for c in range(r.C):
        cl = nodes[c * N:(c + 1) * N]
        lead = [n for n in cl if n["role"] == 2]
        assert len(lead) == 1, f"cluster {c} has {len(lead)} leaders"
        ldl, rc = lead[0]["deadline"], lead[0]["res_count"]
        req = max(n["req_count"] for n in cl if n["role"] != 2)
        if req:
            th = ldl - hb + P
        elif rc:
            j0 = F - rc
            th = ldl - hb - (2 * d + j0 - 1 if j0 else 0) + P
        else:
            th = ldl
        out.append(th - t0)
    return out


def ran_event(before, after, N):
    """Per cluster: some node's trace hash changed between two reads of the node records."""
    return [any(before[c * N + k]["trace_hash"] != after[c * N + k]["trace_hash"] for k in range(N))
            for c in range(len(before) // N)]


def wave_kinds(ev):
    """The kinds of the full 64-cluster waves of one launch: 'none', 'some' or 'all' ran an event."""
    kinds = set()
    for w in range(len(ev) // 64):
        n = sum(ev[64 * w:64 * w + 64])
        kinds.add("none" if n == 0 else "all" if n == 64 else "some")
    return kinds


def align_full_waves(bes, P, d):
    """Host-write every cluster of a full wave onto one of two heartbeat phases, three ticks apart
    (even and odd cluster ids): with the elections' random phases no tick has all 64 clusters of a
    wave, or none of them, running an event. A cluster is written when it has no message in flight:
    every node's deadline moves by the same amount, so it stays at its fixed point. The writes clear
    the certificates; the launches that follow set them again. Returns the ticks stepped (one
    launch each), for the caller to compare after."""
    ref = bes[-1]                                    # the oracle decides; every backend gets the same
    N, full = ref.N, (ref.C // 64) * 64
    target = ref.tick + 2 * P                        # even ids heartbeat here, odd ids 3 ticks later
    todo, steps = set(range(full)), 0
    while todo:
        assert ref.tick + 4 < target, "alignment did not finish before its target"
        nodes = ref.read_nodes()
        for c in sorted(todo):
            cl = nodes[c * N:(c + 1) * N]
            if any(n["req_count"] or n["res_count"] for n in cl):
                continue
            lead = next(n for n in cl if n["role"] == 2)
            shift = target + 3 * (c & 1) - lead["deadline"]
            for be in bes:
                raw = be.read_nodes_raw(c, 1)
                for k in range(N):
                    raw[k].deadline = raw[k].deadline + shift
                be.write_nodes(c, raw)
            todo.discard(c)
        if todo:
            for be in bes:
                be.step(1)
            steps += 1
    return steps
