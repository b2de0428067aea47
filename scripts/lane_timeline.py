"""Per-wave timeline of the lane-per-cluster steady kernel from a -DRS_WAVELOG build (diagnostic
only): wave start/end, load / loop / write-back split, loop trips and events per lane.
Usage: lane_timeline.py LIB [clusters] [launches]"""
import numpy as np

import probe


def main(argv=None):
    p = probe.parser(__doc__)
    p.add_argument("lib", metavar="LIB")
    p.add_argument("clusters", nargs="?", type=int, default=65536)
    p.add_argument("launches", nargs="?", type=int, default=6)
    args = p.parse_args(argv)
    sim = probe.open_sim(args.lib, **probe.workload("c2", args.clusters))
    probe.launches(sim, args.launches)
    a, start, end = probe.wavelog(sim, 2 * args.clusters // 12 + 1000, width=32)
    t0 = start.min()
    st, en = (start - t0) / 100.0, (end - t0) / 100.0
    q = lambda x: probe.pct(x, 8)  # noqa: E731
    print(f"kernel_ms {sim.last_step_timing()[0]:.4f} waves {len(a)} span {en.max():.1f} us")
    print("start us    p0/10/50/90/99/100:", q(st))
    print("life us     p0/10/50/90/99/100:", q(en - st))
    print("load us     p0/10/50/90/99/100:", q(a[:, 8] / 100.0))
    print("loop us     p0/10/50/90/99/100:", q((a[:, 9] - a[:, 8]) / 100.0))
    print("wb us       p0/10/50/90/99/100:", q((end - start - a[:, 9]) / 100.0))
    print("trips       p0/10/50/90/99/100:", q(a[:, 4]))
    if (a[:, 20] | a[:, 21] | a[:, 22]).any():   # fixed-point path stamps (round-5 builds)
        x1, x2, x3 = a[:, 20], a[:, 21], a[:, 22]
        print("  load..extracted  us:", q((x1 - a[:, 8]) / 100.0))
        print("  ..fp decided     us:", q((x2 - x1) / 100.0))
        print("  ..fp rounds done us:", q((x3 - x2) / 100.0))
        print("  ..general loop   us:", q((a[:, 9] - x3) / 100.0))
        # the line-0 body flags a wave with some cluster in a round at the launch's start or its end
        # (rec[5]'s last word): wave life and the five phases for the waves without and with one
        cutw = a[:, 23] != 0
        for nm, m in (("no cluster in a cut round", ~cutw), ("some cluster in a cut round", cutw)):
            if not m.any():
                print(f"  waves with {nm}: none")
                continue
            print(f"  waves with {nm}: {int(m.sum())}")
            print("    life             us:", q((en - st)[m]))
            print("    line 0 loaded    us:", q(a[m, 8] / 100.0))
            print("    ..extracted      us:", q((x1 - a[:, 8])[m] / 100.0))
            print("    ..rounds done    us:", q((x3 - x2)[m] / 100.0))
            print("    ..image, rings   us:", q((a[:, 9] - x3)[m] / 100.0))
            print("    ..lines stored   us:", q((end - start - a[:, 9])[m] / 100.0))
            if a[:, 19].any():   # the stamp before the line-store block's first image read
                q2 = lambda x: " ".join(  # noqa: E731  (the clock's own resolution, 0.01 us)
                    f"{v:8.2f}" for v in np.percentile(x, [0, 10, 50, 90, 99, 100]))
                print("      body end -> store block      us:", q2((a[:, 19] - a[:, 9])[m] / 100.0))
                print("      store block -> stores issued us:",
                      q2((end - start - a[:, 19])[m] / 100.0))
    print("lanes on    p0/10/50/90/99/100:", q(a[:, 7]))
    print("events/lane min p0/10/50/90/99/100:", q(a[:, 10]))
    print("events/lane max p0/10/50/90/99/100:", q(a[:, 11]))
    print("us per trip p0/10/50/90/99/100:", q((a[:, 9] - a[:, 8]) / 100.0 / np.maximum(a[:, 4], 1)))
    done = a[:, 17] | (a[:, 18] << 32)
    done = done[done != 0]
    if len(done):
        print(f"workgroup done (stores drained, counters added) us after the first start: "
              f"p50 {np.percentile((done - t0) / 100.0, 50):.1f} max {(done.max() - t0) / 100.0:.1f}")
    probe.simd_packing(a[:, 5], a[:, 6])
    ph = a[:, 12:17].astype(np.float64)
    trips = np.maximum(a[:, 4], 1)[:, None]
    names = ("head", "decide", "heartbeat", "-", "run (append-entries + responses)")
    print("shader cycles per trip (mean over waves): " + "  ".join(
        f"{nm} {v:7.0f}" for nm, v in zip(names, (ph / trips).mean(axis=0))))
    print("shader cycles per wave (mean): " + "  ".join(f"{nm} {v:8.0f}" for nm, v in zip(names, ph.mean(axis=0))))


if __name__ == "__main__":
    main()
