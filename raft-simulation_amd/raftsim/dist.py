"""Multi-GPU plumbing: cluster-range sharding and the counter all-reduce.

Clusters are independent and Philox streams are keyed by the global cluster id (SIM_SPEC D13),
so a rank simulates a contiguous range of clusters with no data-path exchange. The only
collective is the end-of-run reduction of the counter vector (SUM) and the first-violation tick
(MIN) and the largest append-entries payload (MAX): a few hundred bytes, latency-bound, over RCCL (torch.distributed backend "nccl") on the GPU
box or gloo in the CPU tests.
"""
from __future__ import annotations

NONE_TICK = 2 ** 63 - 1


def shard(total_clusters: int, rank: int, world: int) -> tuple[int, int]:
    """Contiguous [offset, offset + count) range of global cluster ids owned by `rank`."""
    lo = total_clusters * rank // world
    hi = total_clusters * (rank + 1) // world
    return lo, hi - lo


def reduce_counters(c: dict, device=None) -> dict:
    """All-reduce a counters dict (raftsim Backend.counters()) over the default process group."""
    import torch
    import torch.distributed as dist

    names = sorted(k for k in c if k not in ("first_violation_tick", "payload_max"))
    v = torch.tensor([int(c[k]) for k in names], dtype=torch.int64, device=device)
    dist.all_reduce(v, op=dist.ReduceOp.SUM)
    pm = None
    if "payload_max" in c:
        pm = torch.tensor([int(c["payload_max"])], dtype=torch.int64, device=device)
        dist.all_reduce(pm, op=dist.ReduceOp.MAX)
    fv = c.get("first_violation_tick")
    f = torch.tensor([NONE_TICK if fv is None else int(fv)], dtype=torch.int64, device=device)
    dist.all_reduce(f, op=dist.ReduceOp.MIN)
    out = dict(zip(names, (int(x) for x in v.tolist())))
    fmin = int(f.item())
    out["first_violation_tick"] = None if fmin == NONE_TICK else fmin
    if pm is not None:
        out["payload_max"] = int(pm.item())
    return out


def reduce_census(c: dict, device=None) -> dict:
    """All-reduce a census dict (Simulator.census()) over the default process group: SUM of the
    counts and sums (the histograms and per-class counts element by element), MIN of term_min, MAX
    of the *_max fields. Every rank must hold a census of the same `nodes` per cluster."""
    import torch
    import torch.distributed as dist

    maxes = sorted(k for k in c if k.endswith("_max"))
    lists = sorted(k for k, v in c.items() if isinstance(v, list))
    classes = list(c["by_class"])
    sums = sorted(k for k, v in c.items()
                  if k not in maxes and k != "term_min" and not isinstance(v, (list, dict)))
    flat = [int(c[k]) for k in sums] + [int(c["by_class"][k]) for k in classes]
    for k in lists:
        flat += [int(x) for x in c[k]]
    v = torch.tensor(flat, dtype=torch.int64, device=device)
    dist.all_reduce(v, op=dist.ReduceOp.SUM)
    mx = torch.tensor([int(c[k]) for k in maxes], dtype=torch.int64, device=device)
    dist.all_reduce(mx, op=dist.ReduceOp.MAX)
    mn = torch.tensor([int(c["term_min"])], dtype=torch.int64, device=device)
    dist.all_reduce(mn, op=dist.ReduceOp.MIN)
    it = iter(int(x) for x in v.tolist())
    out = {k: next(it) for k in sums}
    out["by_class"] = {k: next(it) for k in classes}
    for k in lists:
        out[k] = [next(it) for _ in c[k]]
    out.update(zip(maxes, (int(x) for x in mx.tolist())))
    out["term_min"] = int(mn.item())
    return {k: out[k] for k in c}


def reduce_audit(a: dict, device=None) -> dict:
    """All-reduce an audit dict (Simulator.audit()) over the default process group: SUM of the
    counts and sums (the per-class counts element by element), MIN of agree_min and the
    *_index_min fields (None: no cluster of the rank has one), MAX of agree_max."""
    import torch
    import torch.distributed as dist

    mins = sorted(k for k in a if k.endswith("_min"))
    maxes = sorted(k for k in a if k.endswith("_max"))
    classes = list(a["by_class"])
    sums = sorted(k for k in a if k not in mins and k not in maxes and k != "by_class")
    v = torch.tensor([int(a[k]) for k in sums] + [int(a["by_class"][k]) for k in classes],
                     dtype=torch.int64, device=device)
    dist.all_reduce(v, op=dist.ReduceOp.SUM)
    mx = torch.tensor([int(a[k]) for k in maxes], dtype=torch.int64, device=device)
    dist.all_reduce(mx, op=dist.ReduceOp.MAX)
    mn = torch.tensor([NONE_TICK if a[k] is None else int(a[k]) for k in mins],
                      dtype=torch.int64, device=device)
    dist.all_reduce(mn, op=dist.ReduceOp.MIN)
    it = iter(int(x) for x in v.tolist())
    out = {k: next(it) for k in sums}
    out["by_class"] = {k: next(it) for k in classes}
    out.update(zip(maxes, (int(x) for x in mx.tolist())))
    out.update((k, None if x == NONE_TICK else x) for k, x in zip(mins, (int(x) for x in mn.tolist())))
    return {k: out[k] for k in a}


def reduce_max(x: float, device=None) -> float:
    import torch
    import torch.distributed as dist

    t = torch.tensor([float(x)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def reduce_sum(x: float, device=None) -> float:
    import torch
    import torch.distributed as dist

    t = torch.tensor([float(x)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


def reduce_min(x: int, device=None) -> int:
    import torch
    import torch.distributed as dist

    t = torch.tensor([int(x)], dtype=torch.int64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return int(t.item())


def first_violation_search(sim, chunk: int, max_ticks: int, reduce_min_fn=None):
    """Step `sim` (any raftsim Backend) `chunk` ticks at a time until a safety violation has been
    counted anywhere in the job (BASELINE config 5: time to the first violation). With
    `reduce_min_fn` (a MIN all-reduce over the ranks, e.g. `lambda x: reduce_min(x, dev)`) every
    rank stops after the same chunk: the one in which any rank first counted a violation.
    Returns (job's first violation tick or None, ticks stepped, timing) with timing = (device ms
    of the steps, summed tick-kernel ms, tick-kernel launches) on a GPU backend, zeros otherwise."""
    done, span, kms, launches = 0, 0.0, 0.0, 0
    timed = "last_span" in getattr(sim, "_fns", {})
    fv = NONE_TICK
    while done < max_ticks and fv == NONE_TICK:
        n = min(chunk, max_ticks - done)
        sim.step(n)
        done += n
        if timed:
            span += sim.last_span()
            ms, nl = sim.last_step_timing()
            kms += ms * nl
            launches += nl
        fv = sim.counters()["first_violation_tick"]
        fv = NONE_TICK if fv is None else int(fv)
        if reduce_min_fn is not None:
            fv = reduce_min_fn(fv)
    return (None if fv == NONE_TICK else fv), done, (span, kms, launches)


def locate_first_violation(sim, reduce_min_fn=None):
    """After first_violation_search on a GPU handle: (the job's first violation tick or None, the
    global ids of this rank's clusters whose first violation is at that tick). The device-side
    query (Simulator.violations with the window [tick, tick + 1)) copies only those clusters'
    records. With `reduce_min_fn` (as in first_violation_search) the tick is the minimum over the
    ranks, and a rank whose own first violation is later returns an empty list."""
    fv = sim.counters()["first_violation_tick"]
    fv = NONE_TICK if fv is None else int(fv)
    if reduce_min_fn is not None:
        fv = reduce_min_fn(fv)
    if fv == NONE_TICK:
        return None, []
    _, recs = sim.violations(t_lo=fv, t_hi=fv + 1)
    return fv, [r["global_id"] for r in recs]
