"""One configuration on the GPU against the C oracle (tests/pairing.py's comparison): clusters that
differ, whether the counters are equal, and on a mismatch the first differing cluster's diff and
its first divergent tick (bisected on the product library, or RAFTSIM_LIB).
  one_case.py [LIB] NAME [--ticks T] [--chunk N] [--set KEY=VALUE ...]
      NAME a parity case of tests/cases.py (CASES); LIB a build (default: the product library)
  one_case.py [LIB] --workload W --clusters C ...
      a bench.py workload at C clusters instead, e.g. --workload c3_spec --clusters 2048
      --ticks 8000 --chunk 1000 --set variant_flags=3"""
from pathlib import Path

import probe


def compare(cfg, make, ticks=20000, chunk=None, what="case"):
    """(clusters differing, counters equal, report) of make(**cfg) against the oracle after `ticks`
    ticks, compared every `chunk` ticks (default: at the end)."""
    import pairing
    with pairing.pair(cfg, make=make) as (g, r):
        try:        # digests, then same_counters, after every chunk
            pairing.run(g, r, pairing.chunks(ticks, chunk or ticks), what, counters=True,
                        bisect=cfg)
            report = ""
        except AssertionError as e:
            report = str(e)
        return int((g.digest() != r.digest()).sum()), g.counters() == r.counters(), report


def main(argv=None):
    p = probe.parser(__doc__)
    p.add_argument("names", nargs="*", metavar="[LIB] NAME")
    p.add_argument("--workload", choices=list(probe.bench.WORKLOADS))
    p.add_argument("--clusters", type=int)
    p.add_argument("--ticks", type=int, default=20000)
    p.add_argument("--chunk", type=int)
    p.add_argument("--set", action="append", default=[], metavar="KEY=VALUE")
    args = p.parse_args(argv)
    over = {k: int(v) for k, v in (kv.split("=") for kv in args.set)}
    if args.workload:
        name, cfg = args.workload, probe.workload(args.workload, args.clusters, **over)
    else:
        import cases
        if not args.names or args.names[-1] not in cases.CASES:
            p.error(f"expected [LIB] NAME, NAME one of {', '.join(cases.CASES)}")
        name = args.names.pop()
        cfg = dict(cases.CASES[name], **over)
    lib = args.names[0] if args.names else None
    bad, equal, report = compare(cfg, lambda **c: probe.open_sim(lib, **c), args.ticks,
                                 args.chunk, name)
    print(report + "\n" * bool(report) + (Path(lib).name if lib else "product"), name,
          "clusters differing:", bad, "counters equal:", equal, flush=True)
    return 1 if report else 0


if __name__ == "__main__":
    raise SystemExit(main())
