"""The configurations the tests run (test infrastructure): tables and the functions that build a
config, and nothing that runs one. CPU witnesses and GPU parity tests read the same entries."""

# ---- parity (test_gpu_parity.py)
FAULTS = dict(drop_ppm=100000, dup_ppm=10000, dmin=1, dmax=50, part_ppm=100000)
# SIM_SPEC D14/D15: bursts of client traffic with quiet gaps longer than the election timeout,
# and clients that follow redirect-client (server.clj:62-63) to the leader
BURSTS = dict(client_period=16384, client_burst=2048, client_redirects=4)
C4_BURSTS = dict(log_cap=4096, client_ppm=500000, client_period=8192, client_burst=2048,
                 client_redirects=4)
# the burst-engine fault cases: short timers and delays with drops, partitions and duplicates
# (medium client rate), and config-4-rate bursts under fast timers
MID = dict(hb=100, el_base=150, el_span=150, dmin=1, dmax=8, drop_ppm=100000, part_ppm=100000,
           dup_ppm=10000)
FAST = dict(hb=300, el_base=500, el_span=500)
B4 = dict(log_cap=4096, client_ppm=500000, client_period=4096, client_burst=1024,
          client_redirects=4)

CASES = {
    # C2 shape (no faults, no client traffic), smaller cluster count
    "c2_small": dict(n_clusters=4096, nodes=5, seed=42),
    # C3 shape: faults, partitions, client-set
    "c3_faults": dict(n_clusters=2048, nodes=5, seed=1, client_ppm=1000, log_cap=256, **FAULTS),
    # C4 shape: 7 and 9 nodes, client-heavy, long logs
    "c4_n7": dict(n_clusters=1024, nodes=7, seed=3, client_ppm=3000, log_cap=512,
                  commit_stream_cap=256),
    "c4_n9": dict(n_clusters=512, nodes=9, seed=5, client_ppm=2000, log_cap=1024, dup_ppm=20000,
                  dmax=8),
    # C5: bug variant (vote granted without the log check)
    "c5_variant": dict(n_clusters=1024, nodes=5, seed=9, client_ppm=1000, log_cap=256,
                       variant_flags=1, commit_stream_cap=7, **FAULTS),
    # overflow and tiny inboxes, heavy duplication
    "overflow": dict(n_clusters=512, nodes=9, seed=11, inbox_cap=2, dup_ppm=300000, dmax=3,
                     client_ppm=5000, log_cap=64),
    # arena pressure: arena == 2L, short logs, frequent client-sets
    "arena_tight": dict(n_clusters=512, nodes=5, seed=13, client_ppm=20000, log_cap=16,
                        arena_cap=32, dup_ppm=100000, dmax=10),
    # arena sizes that are not a multiple of the 8-slot chunks of the arena loops (tick_wave.hpp):
    # runs wrap inside a chunk, and chunks read past an arena's end into the next one
    "arena_odd": dict(n_clusters=512, nodes=5, seed=14, client_ppm=20000, log_cap=16,
                      arena_cap=37, hb=40, el_base=60, el_span=60, dup_ppm=100000, dmax=10,
                      commit_stream_cap=5),
    "spec_arena_odd": dict(n_clusters=512, nodes=5, seed=15, client_ppm=30000, log_cap=24,
                           arena_cap=51, hb=40, el_base=60, el_span=60, variant_flags=2, **FAULTS),
    # launch boundaries that split ticks oddly
    "tiny_launches": dict(n_clusters=300, nodes=5, seed=17, client_ppm=1000, ticks_per_launch=7,
                          **FAULTS),
    "n2": dict(n_clusters=700, nodes=2, seed=19, client_ppm=500, **FAULTS),
    "n3": dict(n_clusters=700, nodes=3, seed=21, client_ppm=500, **FAULTS),
    "n4": dict(n_clusters=700, nodes=4, seed=23, client_ppm=500, **FAULTS),
    "n6": dict(n_clusters=700, nodes=6, seed=25, client_ppm=500, **FAULTS),
    "n8": dict(n_clusters=700, nodes=8, seed=27, client_ppm=500, **FAULTS),
    # F3 trace rings on (they enter the digest): wrap-around, entry-ring overwrite, evictions
    "traced": dict(n_clusters=1024, nodes=5, seed=31, client_ppm=2000, log_cap=128, trace_cap=48,
                   trace_entry_cap=300, commit_stream_cap=16, **FAULTS),
    "traced_tight": dict(n_clusters=256, nodes=9, seed=33, client_ppm=20000, log_cap=16,
                         arena_cap=32, dup_ppm=100000, dmax=10, trace_cap=16, trace_entry_cap=64),
    "fast_timers": dict(n_clusters=1000, nodes=5, seed=29, hb=30, el_base=50, el_span=50,
                        client_ppm=20000, log_cap=128, **FAULTS),
    # F4 Spec-Raft control (SIM_SPEC §8) and its bug-injected form
    "spec_c3": dict(n_clusters=2048, nodes=5, seed=41, client_ppm=2000, log_cap=256,
                    variant_flags=2, commit_stream_cap=64, **FAULTS),
    "spec_nolog": dict(n_clusters=1024, nodes=5, seed=43, client_ppm=5000, log_cap=512, hb=300,
                       el_base=500, el_span=500, variant_flags=3, **FAULTS),
    "spec_n9": dict(n_clusters=512, nodes=9, seed=45, client_ppm=3000, log_cap=1024,
                    variant_flags=2, commit_stream_cap=256, dup_ppm=20000, dmax=8),
    "spec_n4_traced": dict(n_clusters=512, nodes=4, seed=47, client_ppm=4000, log_cap=128,
                           variant_flags=2, trace_cap=32, trace_entry_cap=256, **FAULTS),
    "spec_tight": dict(n_clusters=512, nodes=3, seed=49, client_ppm=30000, log_cap=24,
                       arena_cap=48, hb=40, el_base=60, el_span=60, variant_flags=2,
                       inbox_cap=3, **FAULTS),
    # BASELINE config 4: 7 and 9 nodes, 4096-entry logs, bursts that build 1000+-entry batches
    "c4_n7_bursts": dict(n_clusters=512, nodes=7, seed=3, commit_stream_cap=256, **C4_BURSTS),
    "c4_n9_bursts": dict(n_clusters=256, nodes=9, seed=5, dup_ppm=20000, dmax=8, **C4_BURSTS),
    # the N >= 7 burst engine's edges (tick_wave.hpp BURST): no redirect hops (abandoned
    # client-sets) with one-slot inboxes; follower timers and heartbeats that fall inside bursts;
    # launches that split bursts at odd ticks
    "burst_edges_n7": dict(n_clusters=512, nodes=7, seed=91, client_ppm=500000, client_period=4096,
                           client_burst=1024, client_redirects=0, inbox_cap=1, log_cap=700, hb=300,
                           el_base=500, el_span=500),
    "burst_timers_n9": dict(n_clusters=512, nodes=9, seed=93, client_ppm=300000, client_period=2048,
                            client_burst=512, client_redirects=1, inbox_cap=2, log_cap=2000, hb=40,
                            el_base=60, el_span=40),
    "burst_launches_n8": dict(n_clusters=512, nodes=8, seed=95, client_ppm=500000,
                              client_period=1024, client_burst=256, client_redirects=4,
                              ticks_per_launch=37, log_cap=1500),
    # the burst engine under faults (tests/test_burst_witness.py shows on the oracle that these
    # reach its states). Medium client rate, short timers, drops, partitions, duplicates: heartbeats,
    # fault-caused elections and faulty messages fall between injections, so the engine is entered
    # after an election and left for a lost heartbeat, with halted nodes and with followers whose
    # logs are longer than the new leader's (the `pre = own[as]` compare path); n9 fills its logs
    # (OVERFLOW at log_cap), n8 is the vote-without-log-check variant
    "burst_faults_mid_n7": dict(n_clusters=256, nodes=7, seed=121, log_cap=1024, client_ppm=30000,
                                client_redirects=4, **MID),
    "burst_faults_mid_n9": dict(n_clusters=256, nodes=9, seed=123, log_cap=1024, client_ppm=60000,
                                client_redirects=2, **MID),
    "burst_variant_mid_n8": dict(n_clusters=256, nodes=8, seed=125, log_cap=1024, client_ppm=30000,
                                 client_redirects=4, variant_flags=1, **MID),
    # ... with an odd arena a little above 2L and no trace rings: the engine's arena wrap and its
    # read-ahead of the follower's next entry run across the arena's end
    "burst_arena_odd_n7": dict(n_clusters=256, nodes=7, seed=127, log_cap=48, arena_cap=101,
                               client_ppm=30000, client_redirects=4, **MID),
    # C4-rate bursts with faults: messages in flight when a burst starts and when it ends; with
    # two-slot inboxes on top
    "burst_faults_c4_n9": dict(n_clusters=256, nodes=9, seed=103, **B4, **FAST, **FAULTS),
    "burst_faults_n8_inbox2": dict(n_clusters=256, nodes=8, seed=111, inbox_cap=2, **B4, **FAST,
                                   **FAULTS),
    # config 3 / 5 shapes with the bursty, redirect-following client
    "c3_bursts": dict(n_clusters=2048, nodes=5, seed=1, client_ppm=80000, log_cap=256,
                      **BURSTS, **FAULTS),
    "spec_bursts": dict(n_clusters=1024, nodes=5, seed=61, client_ppm=80000, log_cap=1024,
                        variant_flags=2, commit_stream_cap=64, **BURSTS, **FAULTS),
    "spec_nolog_bursts": dict(n_clusters=1024, nodes=5, seed=63, client_ppm=80000, log_cap=1024,
                              variant_flags=3, **BURSTS, **FAULTS),
    # faithful crash storm under client traffic: most client-sets reach halted nodes (to-halted)
    "crash_storm_clients": dict(n_clusters=2048, nodes=5, seed=13, client_ppm=80000, log_cap=16,
                                hb=300, el_base=500, el_span=500, **BURSTS, **FAULTS),
    "redirect_storm": dict(n_clusters=512, nodes=6, seed=65, client_ppm=1000000,
                           client_period=300, client_burst=40, client_redirects=16, inbox_cap=4,
                           log_cap=128, hb=50, el_base=80, el_span=80, **FAULTS),
    # LITE launches (no faults, no client, fixed delay) at N <= 5 take the steady kernel and hand
    # every other event to the catch-up launch (steady_kernel.hip): its edges
    "lite_n2": dict(n_clusters=1000, nodes=2, seed=71, hb=40, el_base=60, el_span=40),
    "lite_n3": dict(n_clusters=1000, nodes=3, seed=73, hb=300, el_base=500, el_span=500),
    "lite_n4": dict(n_clusters=1000, nodes=4, seed=75, hb=300, el_base=500, el_span=500, dmin=4,
                    dmax=4),
    # heartbeats slower than the election timer: elections keep interrupting the rounds
    "lite_elections": dict(n_clusters=1200, nodes=5, seed=77, hb=700, el_base=500, el_span=400,
                           dmin=3, dmax=3),
    # two-slot inboxes: a leader's four responses overflow its RES ring (the slow delivery path)
    "lite_tiny_inbox": dict(n_clusters=1200, nodes=5, seed=79, inbox_cap=2, hb=200, el_base=500,
                            el_span=300),
    # odd launch splits: queued messages cross launch boundaries into the pair cells
    "lite_odd_launches": dict(n_clusters=600, nodes=5, seed=81, ticks_per_launch=13, hb=60,
                              el_base=100, el_span=100, dmin=7, dmax=7),
    # timers too short for the lane kernel's one-trip heartbeat round (hb < 2d + N - 1, el_base <
    # d + N - 1): every round runs tick by tick, elections keep interrupting them
    "lite_short_round": dict(n_clusters=1000, nodes=5, seed=85, hb=9, el_base=6, el_span=30,
                             dmin=3, dmax=3),
    # LITE launches at N >= 6 have no steady kernel: every launch of a fault-free, client-free
    # handle runs the general body's LITE instance, tick_kernel<N, 0, 0, LITE> (one copy per
    # message, the fault-free delivery pack, no PROV / RC / REGS / BURST): a fixed delay above 1;
    # heartbeats slower than the election timer (NPE halts, messages to halted nodes); four-slot
    # and one-slot inboxes (a leader's RES ring overflows; with one slot every vote is lost and no
    # leader is ever elected); 7-tick delays across 13-tick launches; timers shorter than a round
    "lite_n6": dict(n_clusters=700, nodes=6, seed=171, hb=300, el_base=500, el_span=500),
    "lite_n7_d4": dict(n_clusters=700, nodes=7, seed=173, hb=300, el_base=500, el_span=500,
                       dmin=4, dmax=4),
    "lite_n8_elections": dict(n_clusters=600, nodes=8, seed=175, hb=700, el_base=500, el_span=400,
                              dmin=3, dmax=3),
    "lite_n9_inbox4": dict(n_clusters=512, nodes=9, seed=177, inbox_cap=4, hb=200, el_base=500,
                           el_span=300),
    "lite_n6_inbox1": dict(n_clusters=512, nodes=6, seed=183, inbox_cap=1, hb=40, el_base=60,
                           el_span=40, dmin=2, dmax=2),
    "lite_n9_odd_launches": dict(n_clusters=400, nodes=9, seed=179, ticks_per_launch=13, hb=60,
                                 el_base=100, el_span=100, dmin=7, dmax=7),
    "lite_n7_short_round": dict(n_clusters=512, nodes=7, seed=181, hb=9, el_base=6, el_span=30,
                                dmin=3, dmax=3),
    # fault-free Spec-Raft handles: DevSim::lite is set (rebuild period 8, first launch unpacked,
    # no storm split) but the kernel is tick_kernel<N, 0, SPEC, 0>; at N = 6 the one N = 6 instance
    # with REGS and one wave per SIMD
    "spec_lite_n5": dict(n_clusters=700, nodes=5, seed=185, hb=300, el_base=500, el_span=500,
                         variant_flags=2),
    "spec_lite_n6_elections": dict(n_clusters=512, nodes=6, seed=191, hb=700, el_base=500,
                                   el_span=400, dmin=3, dmax=3, variant_flags=2),
    "spec_lite_n9_inbox4": dict(n_clusters=512, nodes=9, seed=193, inbox_cap=4, hb=200,
                                el_base=500, el_span=300, variant_flags=2),
    # a fault-free traced faithful handle, tick_kernel<6, TRACE, 0, 0> with DevSim::lite set: the
    # 16-event trace ring wraps
    "traced_lite_n6": dict(n_clusters=256, nodes=6, seed=189, hb=40, el_base=60, el_span=40,
                           dmin=2, dmax=2, trace_cap=16, trace_entry_cap=8),
}

# ---- cluster packs (test_gather_abi.py)
# The cases tests/test_gpu_gather.py runs for parity: (config, ticks). Chosen on the oracle, so
# that the witnesses of tests/test_gather_abi.py hold.
GPU_CASES = {
    "arena_odd": (dict(CASES["arena_odd"], n_clusters=96), 6000),
    "burst_arena_odd_n7": (dict(CASES["burst_arena_odd_n7"], n_clusters=64), 6000),
    "n2": (dict(CASES["n2"], n_clusters=96), 20000),
    "c4_n9": (dict(CASES["c4_n9"], n_clusters=64), 20000),
    "spec_c3": (dict(CASES["spec_c3"], n_clusters=96, commit_stream_cap=8), 20000),
}
ROUNDTRIP = dict(n_clusters=64, nodes=5, seed=3, client_ppm=3000, log_cap=64, **FAULTS)

# ---- census and audit (test_gpu_census.py)
# case, clusters, checkpoints: the runs of test_census_abi.POPULATIONS, one per N = 2..9; where
# that table lists one tick, half of it first. 333 and 96 are no multiples of floor(64/N) except
# 96 at N = 8, so "n8" at 333 clusters (333 = 41 * 8 + 5) runs beside the table's N = 8 case.
PARITY = [("n2", 333, (10000, 20000)), ("n3", 333, (10000, 20000)), ("n4", 333, (10000, 20000)),
          ("fast_timers", 333, (1000, 2000)), ("n6", 333, (10000, 20000)),
          ("burst_faults_mid_n7", 96, (2500, 5000)), ("burst_variant_mid_n8", 96, (1250, 2500)),
          ("n8", 333, (10000, 20000)), ("burst_faults_mid_n9", 96, (2500, 5000))]


def cfg_of(name, n, **extra):
    return dict(CASES[name], n_clusters=n, **extra)


# ---- steady line-0 path (test_gpu_steady_line0.py)
C_CUT = 199          # three full waves and a partial one: the shard ends inside a wave


def cut_cfg(nodes, d, clusters=C_CUT):
    """Small timers on which the certified path's conditions hold (hb >= 2d + F, el_base >= P)
    and a launch end can land in every phase of a round."""
    F = nodes - 1
    hb = 2 * d + F + 2
    P = 2 * d + F - 1 + hb
    return dict(n_clusters=clusters, nodes=nodes, seed=100 + 10 * nodes + d, hb=hb, el_base=2 * P,
                el_span=4 * P, dmin=d, dmax=d), P


# ---- high clocks (test_gpu_high_clock.py)
# Shapes: 256 clusters (512 where stated), short timers (hb 40, election 60 + 60), delays up to 10,
# 6,000 ticks in launches of 1,500 unless stated.
HC_C = 256
HC_TICKS, HC_LAUNCH = 6000, 1500
HC_CHUNKS = [HC_LAUNCH] * (HC_TICKS // HC_LAUNCH)
HC_SHORT = dict(hb=40, el_base=60, el_span=60)
HC_NET = dict(drop_ppm=100000, dup_ppm=10000, dmin=1, dmax=10, part_ppm=100000)
HC_CLIENTS = dict(client_ppm=20000, client_period=4096, client_burst=1024, client_redirects=4,
                  log_cap=256)


def hc_case(**kw):
    return dict(dict(n_clusters=HC_C, ticks_per_launch=HC_LAUNCH, **HC_SHORT), **kw)


FAULTS_N5 = hc_case(nodes=5, seed=301, part_epoch=7, **HC_NET)
CLIENTS_N5 = hc_case(nodes=5, seed=303, part_epoch=7, **HC_CLIENTS, **HC_NET)

# name -> config; the comment names the kernel family the case reaches
GENERAL = {
    # tick_kernel<5, 0, 0, 0>: the faithful N = 5 body with drops, duplicates, partitions
    "faults_n5": FAULTS_N5,
    "clients_n5": CLIENTS_N5,
    # tick_kernel<N, 0, 0, 0> for the other node counts (the n2..n8 shapes)
    "n2": hc_case(nodes=2, seed=19, client_ppm=500, **HC_NET),
    "n3": hc_case(nodes=3, seed=21, client_ppm=500, **HC_NET),
    "n4": hc_case(nodes=4, seed=23, client_ppm=500, **HC_NET),
    "n6": hc_case(nodes=6, seed=25, client_ppm=500, **HC_NET),
    "n8": hc_case(nodes=8, seed=27, client_ppm=500, **HC_NET),
    # N >= 7 at config-4 burst rates: above tick 2^28 the burst engine is gated off and the tick
    # loop carries the bursts (at LOW the engine itself runs them)
    "burst_n7": hc_case(nodes=7, seed=103, **B4, **FAST, **HC_NET),
    "burst_n9": hc_case(nodes=9, seed=105, **B4, **FAST, **HC_NET),
    "burst_n8_inbox2": hc_case(nodes=8, seed=111, inbox_cap=2, **B4, **FAST, **HC_NET),
    # ... and with the short timers: after the overdue-fresh start the long ones leave few leaders
    # in 6,000 ticks, these have one in a quarter of the clusters when the bursts come
    "burst_n7_short": hc_case(nodes=7, seed=103, **B4, **HC_NET),
    "burst_n9_short": hc_case(nodes=9, seed=105, **B4, **HC_NET),
    # Spec-Raft bodies, tick_kernel<N, 0, SPEC, 0>, and the two bug variants (they violate)
    "spec_n5": hc_case(nodes=5, seed=41, client_ppm=2000, log_cap=256, variant_flags=2,
                       commit_stream_cap=64, **HC_NET),
    "spec_n8": hc_case(nodes=8, seed=45, client_ppm=2000, log_cap=256, variant_flags=2, **HC_NET),
    "variant1_n5": hc_case(nodes=5, seed=9, client_ppm=20000, log_cap=128, variant_flags=1,
                           **HC_NET),
    "spec_nolog_n5": hc_case(nodes=5, seed=43, client_ppm=20000, log_cap=256, variant_flags=3,
                             **HC_NET),
    # overflowing two-slot inboxes under heavy duplication; an arena that is no multiple of the
    # 8-slot chunks
    "overflow": hc_case(nodes=9, seed=11, inbox_cap=2, dup_ppm=300000, dmax=3, client_ppm=5000,
                        log_cap=64),
    "arena_odd": hc_case(nodes=5, seed=14, client_ppm=20000, log_cap=16, arena_cap=37,
                         dup_ppm=100000, dmax=10, commit_stream_cap=5),
    # launches of 7 ticks; both schedules (the wave packing's sched_bucket(ev, t0))
    "tiny_launches": dict(CLIENTS_N5, seed=17, ticks_per_launch=7),
    "sched_aligned": dict(CLIENTS_N5, schedule=0),
    "sched_fixed": dict(CLIENTS_N5, schedule=1),
    # the partition epoch's divisor
    "epoch_1": dict(FAULTS_N5, part_epoch=1),
    "epoch_3": dict(FAULTS_N5, part_epoch=3),
    "epoch_1000": dict(FAULTS_N5, part_epoch=1000),
    "epoch_65537": dict(FAULTS_N5, part_epoch=65537),
    "epoch_2p31": dict(FAULTS_N5, part_epoch=2 ** 31 + 3),
    # the client schedule's divisors: a short period, and one above 2^31 (at TOP its next window
    # starts past the clock: the cursor saturates at "never" and nothing is injected)
    "period_37": dict(CLIENTS_N5, client_period=37, client_burst=11),
    "period_2p31": dict(CLIENTS_N5, client_period=2 ** 31 + 5, client_burst=2 ** 30 + 1),
    # fault-free, client-free handles at N >= 6: tick_kernel<N, 0, *, LITE> (and the Spec-Raft
    # N = 6 instance with heartbeats slower than the election timer)
    "lite_n6": hc_case(nodes=6, seed=171),
    "lite_n7_d4": hc_case(nodes=7, seed=173, dmin=4, dmax=4),
    # (nine timers firing together overflow four-slot inboxes for good: lite_n9_inbox4 elects
    # almost nobody and runs elections and overflow throughout; lite_n9 settles)
    "lite_n9_inbox4": hc_case(nodes=9, seed=177, inbox_cap=4),
    "lite_n9": hc_case(nodes=9, seed=179),
    "spec_lite_n6_elections": hc_case(nodes=6, seed=191, hb=70, el_base=50, el_span=40, dmin=3,
                                      dmax=3, variant_flags=2),
}
# trace rings on (they enter the digest): tick_kernel<N, TRACE, 0, 0>
TRACED = {
    "traced_n5": hc_case(nodes=5, seed=31, client_ppm=2000, log_cap=128, trace_cap=48,
                         trace_entry_cap=300, commit_stream_cap=16, **HC_NET),
    "traced_n6": hc_case(nodes=6, seed=189, dmin=2, dmax=2, trace_cap=16, trace_entry_cap=8),
}
# the violating cases the queries run on
QUERIES = {
    "variant1_n5": GENERAL["variant1_n5"],
    "spec_nolog_n5_512": dict(GENERAL["spec_nolog_n5"], n_clusters=512),
}
LITE = [(n, d) for n in (2, 3, 4, 5) for d in (1, 3)]


def lite_cfg(nodes, d):
    """cut_cfg at 256 clusters, one launch per step, and the launch plan: 300 P ticks in launches
    of 3 P (the elections settle), 40 P + 1, then one launch of 1000 P + 3 ticks."""
    cfg, P = cut_cfg(nodes, d, HC_C)
    cfg["ticks_per_launch"] = 65536
    return cfg, P, [3 * P] * 100 + [40 * P + 1, 1000 * P + 3]


# ---- the burst engine's gate (test_burst_witness.py)
# The 2^28 gate (test_gpu_burst_engine.py::test_gpu_burst_gate_2_28): the engine packs arrivals in
# 28 bits and runs only in launches that end at or before tick 2^28 - 1.
GATE_T0 = 2 ** 28 - 15000
GATE_TICKS = 24000
GATE_CFG = dict(n_clusters=256, nodes=7, seed=131, ticks_per_launch=2500, drop_ppm=20000, dmin=1,
                dmax=8, **B4, **FAST)


def gate_setup(be):
    """After set_tick no client-set is ever injected unless the cursors are written too."""
    be.write_clusters(0, [dict(hwm=(0, 0, 0), client_next=GATE_T0 + 1500 + 3 * i, client_count=0)
                          for i in range(be.C)])
