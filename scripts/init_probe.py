"""c2_init probe (diagnostic): the first 10k-tick launch of fresh handles of bench.py's c2_init
(65,536 clusters unless --clusters): device span of the step (HIP events, packing kernels
included) and the tick kernel's own time.
  init_probe.py [LIB]           both packing modes (RAFT_SCHED_ALIGNED = 0, RAFT_SCHED_FIXED = 1),
                                three seeds each, three repetitions
  init_probe.py [LIB] --check   three seeds: span, tick kernel and the steady kernel's bails; for the
                                first seed the first 2,048 clusters' digests against the C oracle"""
import numpy as np

import probe


def first_launches(lib, clusters, seeds, report, **extra):
    """Fresh handles, one per seed; then each one's first step, reported, and the handle closed."""
    sims = [probe.open_sim(lib, **probe.workload("c2_init", clusters, seed=s, **extra))
            for s in seeds]
    for s in sims:
        s.step_async(probe.TICKS)
        s.sync()
        ms, nl = s.last_step_timing()
        report(s, s.last_span() * 1e3, ms * 1e3, nl)
        s.close()


def check(s, span, ms, nl):
    print(f"span {span:7.1f} us  kernel {ms:7.1f} us x{nl}  bails {s.diag_last_bails()}", flush=True)
    if s.config.seed == 42:
        import pairing
        cfg = probe.workload("c2_init", min(s.C, 2048))
        with pairing.closing(pairing.oracle(cfg, ticks=probe.TICKS)) as (r,):
            bad = np.nonzero(s.digest(0, r.C) != r.digest())[0]
            print(f"digest mismatches in [0, {r.C}):", len(bad), bad[:8])
            pairing.same(s, r, "c2_init", lo=0)         # raises with the first cluster's diff


def main(argv=None):
    p = probe.parser(__doc__)
    p.add_argument("lib", nargs="?", metavar="LIB", help="default: the product library")
    p.add_argument("--check", action="store_true")
    p.add_argument("--clusters", type=int)
    args = p.parse_args(argv)
    for rep in range(3):
        if args.check:
            first_launches(args.lib, args.clusters, [42 + rep], check)
            continue
        for sched in (0, 1):
            first_launches(args.lib, args.clusters, (42, 43, 44), lambda s, span, ms, nl: print(
                f"sched {sched} span {span:8.1f} us  tick kernel {ms:8.1f} us x{nl}", flush=True),
                schedule=sched)


if __name__ == "__main__":
    main()
