"""A/B kernel builds in ONE process, interleaved (cdna_hip_programming.md §5.4 rule 24), on bench.py's
workloads at one GPU's size; whether the builds agree on the state.

  ab_probe.py LIB_A LIB_B ... [--sched=0|1] [--rounds=N] [--WORKLOAD ...]
      steady launches: a warm-up step, then N (5) interleaved rounds; median and min kernel ms
      per 10k-tick launch for each build
  ab_probe.py LIB_A LIB_B ... --by-launch [--clusters C] [--steps K] --WORKLOAD ...
      from init-node, launch by launch (K = 20): every build's kernel ms, then the totals
  ab_probe.py LIB ... --span [--WORKLOAD]
      device time per step (default C2): a fresh handle, 3 warm-up steps, 20 steps enqueued
      without waiting, one sync; span per step and launch us, 3 repetitions per build"""
import statistics
from pathlib import Path

import probe

STEADY = ("c2", "c3", "c4_n9", "c4_n7", "c4_spec", "c3_spec")


def steady(name, libs, cfg, rounds):
    sims = [probe.open_sim(lib, **cfg) for lib in libs]
    for s in sims:
        s.step(probe.TICKS)                             # warm up to a steady state
    recs = [[] for _ in libs]
    for _ in range(rounds):
        for i, s in enumerate(sims):
            recs[i] += probe.launches(s, 1)
    for lib, rs in zip(libs, recs):
        ts = [r.ms for r in rs]
        print(f"{name:6s} {Path(lib).name:28s} median {statistics.median(ts):8.3f} ms  "
              f"min {min(ts):8.3f} ms  sum {sum(ts):9.3f} ms  step wall median "
              f"{statistics.median(r.wall for r in rs):8.3f} ms", flush=True)
    print(f"{name:6s} builds agree on state: {probe.agree(sims, 0, 256)}", flush=True)
    for s in sims:
        s.close()


def by_launch(name, libs, cfg, steps):
    sims = [probe.open_sim(lib, **cfg) for lib in libs]
    tot = [0.0] * len(libs)
    for step in range(steps):
        row = [probe.launches(s, 1)[0].ms for s in sims]
        tot = [t + ms for t, ms in zip(tot, row)]
        print(f"{name} launch {step:2d} " + " ".join(f"{ms:8.3f}" for ms in row), flush=True)
    print(f"{name} total " + " ".join(f"{x:8.2f}" for x in tot), flush=True)
    print(f"{name} agree {probe.agree(sims, 0, min(sims[0].C, 2048))}", flush=True)
    for s in sims:
        s.close()


def span(libs, cfg):
    for lib in libs:
        for _ in range(3):
            sim = probe.open_sim(lib, **cfg)
            probe.launches(sim, 3)
            for _ in range(20):
                sim.step_async(probe.TICKS)
            sim.sync()
            ms, _ = sim.last_step_timing()
            print(f"{Path(lib).name:28s} step {sim.last_span() / 20 * 1e3:7.2f} us  launch "
                  f"{ms * 1e3:7.2f} us", flush=True)
            sim.close()


def main(argv=None):
    p = probe.parser(__doc__, workloads=True)
    p.add_argument("libs", nargs="+", metavar="LIB")
    p.add_argument("--by-launch", action="store_true")
    p.add_argument("--span", action="store_true")
    p.add_argument("--sched", type=int, help="the handles' schedule (0 aligned, 1 fixed)")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--clusters", type=int, help="default: the workload's at one GPU")
    p.add_argument("--steps", type=int, default=20)
    args = p.parse_args(argv)
    extra = {} if args.sched is None else {"schedule": args.sched}
    for name in args.only or (("c2",) if args.span else STEADY):
        cfg = probe.workload(name, args.clusters, **extra)
        if args.span:
            span(args.libs, cfg)
        elif args.by_launch:
            by_launch(name, args.libs, cfg, args.steps)
        else:
            steady(name, args.libs, cfg, args.rounds)


if __name__ == "__main__":
    main()
