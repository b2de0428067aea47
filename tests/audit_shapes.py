"""Hand-built clusters for the log audit's tests (test infrastructure): logs that no run of the
parity cases reaches -- long ones, ones that cross an arena's end, single differences at the step
boundaries of both group widths of csrc/audit_kernel.hip (16 and 64 lanes) -- as plain Python
data. tests/test_audit_abi.py holds tests/audit_oracle.py to the classes written down here;
tests/test_gpu_audit.py writes the same shapes into a GPU handle."""
from __future__ import annotations

POISON_TERM = 0          # below every real term: read one past a log's end it inverts the order


def base_log(n):
    """Strictly rising terms, so a term one higher at one position inverts nothing."""
    return [(2 * p + 2, 1000 + p) for p in range(n)]


def pairs_of(N):
    """The pairs (0-based) whose bits are the first, a middle and the last of the pair mask."""
    return [(0, 1), (0, N - 1), (N - 2, N - 1)] if N > 2 else [(0, 1)]


def shapes(N, log_cap):
    """[dict(name, logs, commits, want)]: N logs and commit indices per cluster; want: the
    cluster's classes, written down from the definitions (SIM_SPEC.md)."""
    big = log_cap == 256
    full = 130 if big else log_cap                      # the length of the compared logs
    lengths = (0, 1, 2, 15, 16, 17, 63, 64, 65, 129, 256) if big else (0, 1, 2, 15, 16, 17, 24)
    spots = (0, 15, 16, 17, 63, 64, 65, full - 1) if big else (0, 15, 16, 17, full - 1)
    out = []

    def add(name, logs, commits, want):
        out.append(dict(name=name, logs=[list(x) for x in logs], commits=list(commits),
                        want=tuple(want)))

    def two(i, j, a, b, rest):
        """Node i holds a, node j holds b, the others `rest`."""
        return [a if k == i else b if k == j else rest for k in range(N)]

    # every length, all logs equal; a commit index beyond the log changes nothing
    for n in lengths:
        add(f"identical_{n}", [base_log(n)] * N, [n + 300] * N, ("identical",))
    # one log alone: nothing to compare (a single entry: nothing to order either)
    add("lone_1", two(0, 0, base_log(1), None, []), [1] * N, ())
    add("lone_2", two(1, 1, [(5, 1), (4, 2)], None, []), [2] * N, ("term_order",))
    add("lone_full", two(N - 1, N - 1, base_log(log_cap), None, []), [0] * N, ())
    # a single difference between one pair, the other nodes a prefix that ends before it
    for n, d in enumerate(spots):
        for field in (0, 1):
            i, j = pairs_of(N)[(n + field) % len(pairs_of(N))]
            a, b = base_log(full), base_log(full)
            b[d] = (b[d][0] + 1, b[d][1]) if field == 0 else (b[d][0], b[d][1] + 77)
            below = (n + field) % 2 == 0              # the commits straddle d
            commits = [d + 1 if below else d] * N
            commits[j] = d + 5
            want = ["diverged"]
            if below:
                want.append("commit_diverged")
            if field == 1 or d != full - 1:           # the same term at d, or equal terms after it
                want.append("match_broken")
            add(f"diff_{'term' if field == 0 else 'val'}_{d}", two(i, j, a, b, base_log(d)),
                commits, want)
    # unequal lengths: the short log ends one before, at and one after the difference
    d = 64 if big else 16
    for n in (d, d + 1, d + 2):
        i, j = pairs_of(N)[-1]
        a, b = base_log(full), base_log(n)
        if n > d:
            b[d] = (b[d][0] + 1, b[d][1])
        want = [] if n == d else ["diverged", "commit_diverged"] + (["match_broken"] if n > d + 1 else [])
        add(f"short_{n - d - 1:+d}", two(i, j, a, b, []), [full] * N, want)
    # bit 4: terms differ from d = 3 on, but for an equal term one step later (either width) or in
    # the last position only; the control has none
    for name, eq in (("step16", 3 + 16), ("step64", 3 + 64 if big else 3 + 8),
                     ("last", full - 1), ("never", None)):
        a = base_log(full)
        b = [(t + 1, v) if p >= 3 and p != eq else (t, v) for p, (t, v) in enumerate(a)]
        add(f"match_{name}", two(0, N - 1, a, b, a[:3]), [0] * N,
            ("diverged",) if eq is None else ("diverged", "match_broken"))
    # bit 8: an inversion at a step boundary of either width and at the last pair, shared by every
    # node (nothing diverges) and in one node alone
    for q in ((15, 63, full - 2) if big else (15, 7, full - 2)):
        a = base_log(full)
        a[q] = (a[q + 1][0] + 1, a[q][1])
        add(f"order_all_{q}", [a] * N, [0] * N, ("term_order", "identical"))
        add(f"order_one_{q}", two(N - 1, N - 1, a, None, base_log(full)), [0] * N,
            ("diverged", "match_broken", "term_order"))
    return out


def bases(N, A, c, sh):
    """arena_base of every node of cluster c: each log crosses the arena's end at another position
    (the nodes of a difference at it and one before it where the shape has one), the last but one
    node not at all, and with whole arenas added: the base counts up for ever."""
    lens = [len(x) for x in sh["logs"]]
    diff = next((p for p in range(min(lens[0], lens[-1]))
                 if sh["logs"][0][p] != sh["logs"][-1][p]), 5)
    out = []
    for k in range(N):
        cross = (diff, max(diff - 1, 1), 3 + 5 * k + c % 7)[0 if k == 0 else 1 if k == N - 1 else 2]
        b = (A - cross) % A if k != N - 2 or N == 2 else 0
        out.append(b + (k + c) % 3 * A)
    return out


def arena_of(log, base, A, k):
    """The A slots of a node's arena: the log from slot base mod A on, every other slot an entry
    that would raise every bit if read: another val on every node (a stale difference one past
    len), under a term equal on all of them and below the log's last (an inverted, matching
    term)."""
    arena = [(POISON_TERM, 0xDEAD0000 + k)] * A
    for p, e in enumerate(log):
        arena[(base + p) % A] = e
    return arena
