"""csrc/launch_plan.hpp on the CPU: what a tick launch is -- the kernel, the schedule kernels before
it, the packing, the keys, the event pair, the bail counters' parity -- and what each host call
invalidates for the next launch.

A stand-alone C++ program (its own main, the header and include/raftsim.h alone) is compiled with
g++ -- under ASan and UBSan where the machine has their runtimes -- and run once.

Reference: the decisions as they stood before the header, spread over raftsim.hip (sh_create,
sh_step_async, the write sites, raft_sim_set_tick, the scatter's bookkeeping) and the launchers
(launch_tick / _n / _ns, launch_steady's refusal of a perm), transcribed as flat functions over a
plain struct of the old field names, with the constants as literals. For a random sequence of
events on every configuration -- N = 2..9, Spec-Raft on and off, trace rings, client traffic,
faults (none, drops, dmin != dmax), both schedules, ticks per launch 7 / 10000 / 65536, the three
steady modes, launch events, C in {15, 16, 17, 131071, 131072}, el_base in {5000, 2^28 - 1, 2^28},
client_redirects in {15, 16}; two shards -- planner and transcription agree on every field of every
launch's plan and on the state after every event. Events: steps of 1, 7, tpl - 1, tpl, tpl + 1 and
3 tpl ticks (several before a sync), syncs, every write accepted and refused at each of its refusal
points with and without what ends lite, set_tick (to 0, el_base, either side of 2^31, the horizon
and past it), a scatter on a subset of the shards, bail reports of 0, C/16, C/16 + 1 and C. The
handles that can take the steady kernel run 400 more events of steps, syncs, bail reports and
set_tick alone, so that they change path many times while still lite.

Properties over the same sequences: a planned path has a kernel (path_exists); a step's launches sum
to the step; no launch straddles storm_until; a steady plan has no perm, no keys and no schedule
kernel; the storm kernel is planned only where create's predicates give it a list; a rebuild that
computes no keys follows a launch that wrote them with no set_tick or scatter in between.

Hand-written expectations, independent of the transcription: a C2-shaped handle plans the steady
kernel for every launch and times the first of each sync window only; a bail report of C/16 + 1
(not C/16) seen before launch k sends launches k and k + 1 to the LITE kernel, timed, resets the
report once, and launch k + 2 is steady again; a fresh client handle with el_base 5000 steps 20000
ticks as [0, 5000) storm, [5000, 15000), [15000, 20000) (storm kernel from 131072 clusters, STORM
body below); a lite aligned handle in mode `never` runs launch 0 in id order, launches 1..7 in id
order too (no packing yet), and builds its first packing at the launch where resort_ctr reaches
RESORT_EVERY_LITE -- from the keys launch 7 wrote, which is what the code before the header did
(the comment there said "computes them from the state"; that holds only after a set_tick or a
scatter, which is the next expectation: after set_tick the next rebuild computes its keys); a
steady launch between the launch that wrote keys and the rebuild makes the rebuild compute them;
path_exists is N <= 5 without Spec-Raft for the steady kernel, no Spec-Raft for LITE, N = 2..9."""
import hostprog

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "launch_plan.hpp"

using namespace rs;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() {                      // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static long checks = 0, bad = 0;
static long cfg_id = 0;
static void expect(bool ok, const char* what, long a = 0, long b = 0) {
  ++checks;
  if (!ok && bad++ < 20) printf("MISMATCH %s (config %ld) at %ld, %ld\n", what, cfg_id, a, b);
}

// ---- the decisions as raftsim.hip and tick_kernel.hip made them before the header ---------------
// The kernels the old launchers could run, in TickPath's order; K_INVALID: hipErrorInvalidValue.
enum OldKernel { K_STEADY, K_STORM, K_STORM_BODY, K_TRACE, K_LITE, K_GENERAL, K_INVALID };

struct OldDevSim {                           // the DevSim fields the decisions read
  uint32_t N, TC, lite, client_ppm, variant;
  bool storm_list, perm, shist;              // pointers: null or not
};
struct Old {                                 // Shard
  raft_sim_config_t cfg;
  uint32_t N, C, tpl;
  uint64_t tick, ticks_run;
  bool launch_events, pending;
  uint32_t pending_launches;
  OldDevSim d;
  bool keys_written;
  uint64_t resort_ctr;
  uint32_t resort_every;
  bool steady_ok, last_steady;
  uint32_t steady_parity;
  int steady_mode;                           // 0 auto, 1 always, 2 never
  bool has_bail_host;
  uint32_t bail_host, steady_cooldown, storm_until;
  bool storm_ran, audit_valid;
};
struct OldLaunch {
  uint32_t t0, nt;
  bool sched_key, sched_perm, D_perm, D_shist, timed, report_reset, steady;
  uint32_t nbail;                            // index into nbail2 of d.nbail
  OldKernel kernel;
};

static Old old_create(const raft_sim_config_t& cfg, int env_mode, bool env_events, uint32_t storm_min) {
  Old s;
  memset(&s, 0, sizeof s);
  s.cfg = cfg;
  s.N = cfg.nodes; s.C = cfg.n_clusters;
  s.tpl = cfg.ticks_per_launch ? std::min<uint32_t>(cfg.ticks_per_launch, 65536u) : 10000u;
  OldDevSim& d = s.d;
  d.N = s.N; d.TC = cfg.trace_cap; d.client_ppm = cfg.client_ppm; d.variant = cfg.variant_flags;
  d.lite = cfg.client_ppm == 0 && cfg.drop_ppm == 0 && cfg.dup_ppm == 0 && cfg.part_ppm == 0 &&
           cfg.dmin == cfg.dmax;
  s.steady_ok = d.lite && s.N <= 5 && !d.TC && !(cfg.variant_flags & RAFT_VARIANT_SPEC);
  s.storm_until = cfg.client_ppm && !d.TC ? cfg.el_base : 0u;
  s.resort_every = d.lite ? 8 : 2;
  s.launch_events = env_events;
  d.storm_list = s.storm_until && s.C >= storm_min && cfg.el_base < (1u << 28) &&
                 cfg.client_redirects < 16;
  if (s.steady_ok) {
    s.steady_mode = env_mode;
    s.steady_cooldown = 0;
    s.has_bail_host = true;
    s.bail_host = 0;
  }
  d.shist = cfg.schedule == RAFT_SCHED_ALIGNED;
  return s;
}

template <bool SPEC>
static OldKernel old_launch_tick_ns(uint32_t N, const OldDevSim& S, bool steady, bool storm) {
  if (N <= 5 && !SPEC) {
    if (steady) return S.perm ? K_INVALID : K_STEADY;      // launch_steady: id order only
  }
  if (storm && !S.TC && !S.lite && S.storm_list) return K_STORM;
  if (storm && !S.TC && !S.lite) return K_STORM_BODY;
  else if (S.TC) return K_TRACE;
  else if (!SPEC && S.lite) return K_LITE;
  else return K_GENERAL;
}
static OldKernel old_launch_tick_n(uint32_t N, const OldDevSim& S, bool steady, bool storm) {
  if (S.variant & RAFT_VARIANT_SPEC) return old_launch_tick_ns<true>(N, S, false, storm);
  return old_launch_tick_ns<false>(N, S, steady, storm);
}
static OldKernel old_launch_tick(const OldDevSim& S, bool steady, bool storm) {
  switch (S.N) {
    case 2: case 3: case 4: case 5: return old_launch_tick_n(S.N, S, steady, storm);
    case 6: case 7: case 8: case 9: return old_launch_tick_n(S.N, S, false, storm);
    default: return K_INVALID;
  }
}

static void old_step_async(Old* s, uint32_t n_ticks, std::vector<OldLaunch>& out) {
  s->audit_valid = false;
  uint32_t launches = s->pending_launches;
  if (!s->pending) {
    launches = 0;
    s->pending = true;
  }
  for (uint32_t done = 0; done < n_ticks;) {
    OldLaunch o;
    memset(&o, 0, sizeof o);
    uint32_t nt = std::min(s->tpl, n_ticks - done);
    const uint32_t t0 = (uint32_t)s->tick;
    const bool storm = t0 < s->storm_until;
    if (storm) nt = std::min(nt, s->storm_until - t0);
    bool steady = s->steady_ok && s->d.lite;
    if (steady && s->steady_mode == 2) steady = false;
    if (steady && s->steady_mode == 0) {
      if (s->steady_cooldown) {
        --s->steady_cooldown;
        steady = false;
      } else if (s->bail_host > s->C / 16) {
        s->bail_host = 0;
        o.report_reset = true;
        s->steady_cooldown = 2 - 1;
        steady = false;
      }
    }
    bool no_keys = false;
    bool no_perm = false;
    if (steady) {
      no_perm = no_keys = true;
      s->keys_written = false;
    } else if (s->cfg.schedule == RAFT_SCHED_ALIGNED && s->resort_ctr == 0 && !s->d.client_ppm) {
      no_perm = no_keys = true;
      s->keys_written = false;
      ++s->resort_ctr;
    } else if (s->cfg.schedule == RAFT_SCHED_ALIGNED) {
      if (s->resort_ctr % s->resort_every == 0) {
        if (!s->keys_written) o.sched_key = true;
        o.sched_perm = true;
        s->d.perm = true;
      }
      ++s->resort_ctr;
      s->keys_written = s->resort_ctr % s->resort_every == 0;
      no_keys = !s->keys_written;
    }
    o.timed = s->launch_events || launches == 0 || !steady;
    s->last_steady = steady;
    if (storm && !steady && s->d.storm_list && !s->d.TC && !s->d.lite) s->storm_ran = true;
    if (steady) {
      o.nbail = s->steady_parity;
      s->steady_parity ^= 1;
    }
    OldDevSim D = s->d;
    if (no_perm) D.perm = false;
    if (no_keys) D.shist = false;
    o.t0 = t0; o.nt = nt; o.steady = steady;
    o.D_perm = D.perm; o.D_shist = D.shist;
    o.kernel = old_launch_tick(D, steady, storm && !steady);
    out.push_back(o);
    done += nt;
    s->tick += nt;
    s->ticks_run += nt;
    ++launches;
    s->pending_launches = launches;
  }
}
static void old_sync(Old* s) {
  if (!s->pending) return;
  s->pending = false;
  s->pending_launches = 0;
}
// The write sites up to their last refusal point. `pass`: how many of the call's checks pass.
static void old_write_nodes(Old* s, int pass) {         // checks: range, null input, records
  if (pass < 1) return;
  s->storm_until = 0;
  s->audit_valid = false;
}
static void old_write_queue(Old* s, int pass, bool client_set) {   // checks: node, queue
  const int rc = pass < 1;
  if (!rc) s->storm_until = 0;
  if (rc) return;
  if (pass < 2) return;
  if (client_set) s->d.lite = 0;
}
static void old_write_arena(Old* s, int pass) {         // checks: node, count
  const int rc = pass < 1;
  if (!rc) s->storm_until = 0;
  if (rc) return;
  s->audit_valid = false;
}
static void old_write_commit_stream(Old* s, int pass) { // checks: node, count
  const int rc = pass < 1;
  if (!rc) s->storm_until = 0;
}
static void old_write_clusters(Old* s, int pass, bool cursor) {    // checks: range
  if (pass < 1) return;
  s->storm_until = 0;
  s->audit_valid = false;
  if (cursor) s->d.lite = 0;
}
static void old_set_tick(Old* s, uint64_t tick) {       // per shard, after the horizon check
  old_sync(s);
  s->tick = tick;
  s->storm_until = 0;
  s->keys_written = false;
}
static void old_scatter(Old* s, bool general) {         // per touched shard of an accepted call
  s->storm_until = 0;
  s->audit_valid = false;
  s->keys_written = false;
  if (general) s->d.lite = 0;
}

// ---- the same calls as raftsim.hip makes them now ---------------------------------------------
struct New {
  LaunchFixed f;
  LaunchState s;
  bool pending, has_report;
  uint32_t report;
};
static New new_create(const raft_sim_config_t& cfg, SteadyMode mode, bool events, uint32_t storm_min) {
  New n;
  memset(&n, 0, sizeof n);
  const LaunchEnv env = {mode, events, storm_min};
  n.f = launch_fixed(cfg, env);
  n.s = launch_state(cfg);
  n.has_report = n.f.steady_ok;
  return n;
}
static void new_step_async(New* n, uint32_t n_ticks, std::vector<LaunchPlan>& out) {
  invalidate(n->s, ON_STEP);
  n->pending = true;
  for (uint32_t done = 0; done < n_ticks;) {
    const LaunchPlan p = plan_launch(n->f, n->s, n_ticks - done, n->has_report ? n->report : 0u);
    if (p.reset_report) n->report = 0;
    out.push_back(p);
    launch_enqueued(n->s, p);
    done += p.nt;
  }
}
static void new_sync(New* n) {
  if (!n->pending) return;
  n->pending = false;
  synced(n->s);
}
static void new_write_nodes(New* n, int pass) {
  if (pass < 1) return;
  invalidate(n->s, ON_WRITE_NODES);
}
static void new_write_queue(New* n, int pass, bool client_set) {
  if (pass < 1) return;
  invalidate(n->s, ON_WRITE_QUEUE);
  if (pass < 2) return;
  if (client_set) invalidate(n->s, ON_QUEUED_CLIENT_SET);
}
static void new_write_arena(New* n, int pass) {
  if (pass < 1) return;
  invalidate(n->s, ON_WRITE_ARENA);
}
static void new_write_commit_stream(New* n, int pass) {
  if (pass < 1) return;
  invalidate(n->s, ON_WRITE_COMMIT_STREAM);
}
static void new_write_clusters(New* n, int pass, bool cursor) {
  if (pass < 1) return;
  invalidate(n->s, ON_WRITE_CLUSTERS);
  if (cursor) invalidate(n->s, ON_CLIENT_CURSOR);
}
static void new_set_tick(New* n, uint64_t tick) {
  new_sync(n);
  set_tick(n->s, tick);
}
static void new_scatter(New* n, bool general) {
  invalidate(n->s, ON_SCATTER);
  if (general) invalidate(n->s, ON_SCATTER_GENERAL);
}

// ---- agreement ----------------------------------------------------------------------------------
static void same_state(const Old& o, const New& n, long ev) {
  const LaunchState& s = n.s;
  expect(o.tick == s.tick && o.ticks_run == s.ticks_run, "state: tick, ticks_run", ev, (long)s.tick);
  expect((o.d.lite != 0) == s.lite, "state: lite", ev, s.lite);
  expect(o.storm_until == s.storm_until, "state: storm_until", ev, s.storm_until);
  expect(o.keys_written == s.keys_written, "state: keys_written", ev, s.keys_written);
  expect(o.d.perm == s.packed, "state: a packing exists", ev, s.packed);
  expect(o.resort_ctr == s.resort_ctr, "state: resort_ctr", ev, (long)s.resort_ctr);
  expect(o.steady_cooldown == s.steady_cooldown, "state: steady_cooldown", ev, s.steady_cooldown);
  expect(o.steady_parity == s.steady_parity, "state: steady_parity", ev, s.steady_parity);
  expect(o.pending == n.pending && o.pending_launches == s.window_launch, "state: window", ev,
         s.window_launch);
  expect((o.steady_ok && o.last_steady) == (s.last_path == PATH_STEADY), "state: last path", ev,
         s.last_path);
  expect(o.storm_ran == s.storm_kernel_ran, "state: storm kernel ran", ev, s.storm_kernel_ran);
  expect(o.audit_valid == s.audit_valid, "state: audit_valid", ev, s.audit_valid);
  expect(o.bail_host == n.report, "state: bail report", ev, n.report);
}
static void same_fixed(const Old& o, const New& n) {
  const LaunchFixed& f = n.f;
  expect(o.N == f.N && o.C == f.C && o.tpl == f.tpl && o.resort_every == f.resort_every,
         "fixed: N, C, tpl, resort_every", f.tpl, f.resort_every);
  expect(o.steady_ok == f.steady_ok && o.d.storm_list == f.storm_kernel &&
             o.launch_events == f.launch_events && o.has_bail_host == n.has_report,
         "fixed: steady_ok, storm_kernel, launch_events", f.steady_ok, f.storm_kernel);
  expect(!o.steady_ok || o.steady_mode == (int)f.steady_mode, "fixed: steady_mode", f.steady_mode);
}
static void same_launch(const OldLaunch& o, const LaunchPlan& p, long ev, long i) {
  expect(o.t0 == p.t0 && o.nt == p.nt, "plan: t0, nt", ev, i);
  expect((int)o.kernel == (int)p.path, "plan: path", ev, p.path);
  const SchedPrep want = o.sched_key ? SCHED_KEY_PERM : o.sched_perm ? SCHED_PERM : SCHED_NONE;
  expect(want == p.sched && (!o.sched_key || o.sched_perm), "plan: schedule kernels", ev, p.sched);
  expect(o.D_perm == p.use_perm, "plan: use_perm", ev, i);
  expect(o.D_shist == p.write_keys, "plan: write_keys", ev, i);
  expect(o.timed == p.timed, "plan: timed", ev, i);
  expect(o.report_reset == p.reset_report, "plan: reset_report", ev, i);
  expect(!o.steady || o.nbail == p.bail_parity, "plan: bail parity", ev, i);
}

// SIM_SPEC D1, as raft_sim_step_async and raft_sim_set_tick ask it before any shard is touched
static bool horizon_ok(const raft_sim_config_t& c, uint64_t tick, uint32_t n) {
  const uint64_t longest = std::max<uint64_t>({c.hb, (uint64_t)c.el_base + c.el_span, c.dmax});
  return tick + n + longest < 0xFFFFFFFFull;
}

constexpr int G = 2;                         // shards
// churn: steps, syncs, bail reports and a rare set_tick only, so that a steady handle stays lite
// through many changes of path
static void random_run(const raft_sim_config_t& cfg, int mode, bool events, int n_events,
                       bool churn = false) {
  Old o[G];
  New n[G];
  bool wrote_keys[G] = {};                   // the shard's last launch wrote keys, none spoilt since
  for (int d = 0; d < G; ++d) {
    o[d] = old_create(cfg, mode, events, 131072);
    n[d] = new_create(cfg, (SteadyMode)mode, events, STORM_MIN_CLUSTERS);
    same_fixed(o[d], n[d]);
    same_state(o[d], n[d], -1);
  }
  const bool list_by_create = cfg.client_ppm && !cfg.trace_cap && cfg.n_clusters >= 131072 &&
                              cfg.el_base < (1u << 28) && cfg.client_redirects < 16;
  const uint32_t tpl = n[0].f.tpl;
  const uint32_t longest = cfg.el_base + cfg.el_span;
  uint64_t handle_tick = 0;
  std::vector<OldLaunch> ol;
  std::vector<LaunchPlan> nl;
  for (int ev = 0; ev < n_events; ++ev) {
    const int d = (int)(rnd() % G);
    static const int churn_kinds[16] = {0, 0, 0, 0, 0, 0, 0, 0, 6, 6, 15, 15, 15, 15, 15, 13};
    const int kind = churn ? churn_kinds[rnd() % 16] : (int)(rnd() % 16);
    if (kind < 6) {                          // a step; no sync behind it: several make a window
      static const int mul[6] = {0, 0, -1, 0, 1, 0};
      const uint32_t pick = (uint32_t)(rnd() % 6);
      const uint32_t nticks = pick == 0 ? 1 : pick == 1 ? 7 : pick == 5 ? 3 * tpl : tpl + mul[pick];
      if (!horizon_ok(cfg, handle_tick, nticks)) continue;
      for (int k = 0; k < G; ++k) {
        ol.clear();
        nl.clear();
        const uint32_t storm_until = n[k].s.storm_until;
        old_step_async(&o[k], nticks, ol);
        new_step_async(&n[k], nticks, nl);
        expect(ol.size() == nl.size(), "launches of a step", ev, (long)nl.size());
        uint64_t sum = 0;
        for (size_t i = 0; i < nl.size(); ++i) {
          const LaunchPlan& p = nl[i];
          if (i < ol.size()) same_launch(ol[i], p, ev, (long)i);
          sum += p.nt;
          expect(path_exists(cfg.nodes, cfg.variant_flags & RAFT_VARIANT_SPEC, p.path),
                 "a planned path has a kernel", ev, p.path);
          expect(p.nt >= 1 && (p.t0 >= storm_until || p.nt <= storm_until - p.t0),
                 "no launch straddles storm_until", ev, p.t0);
          expect((p.t0 < storm_until) ==
                     (p.path == PATH_STORM_KERNEL || p.path == PATH_STORM_BODY),
                 "storm ticks, and they alone, take a storm path", ev, p.path);
          expect(p.path != PATH_STEADY || (!p.use_perm && !p.write_keys && p.sched == SCHED_NONE),
                 "a steady plan has no perm, no keys, no schedule kernel", ev, (long)i);
          expect(p.path != PATH_STORM_KERNEL || list_by_create, "the storm kernel needs its list",
                 ev, (long)i);
          expect(p.sched != SCHED_PERM || wrote_keys[k], "a rebuild without keys follows their launch",
                 ev, (long)i);
          expect(cfg.schedule == RAFT_SCHED_ALIGNED || (p.sched == SCHED_NONE && !p.use_perm &&
                                                        !p.write_keys),
                 "a fixed schedule packs nothing", ev, (long)i);
          wrote_keys[k] = p.write_keys;
        }
        expect(sum == nticks, "a step's launches sum to the step", ev, (long)sum);
      }
      handle_tick += nticks;
    } else if (kind < 8) {
      for (int k = 0; k < G; ++k) { old_sync(&o[k]); new_sync(&n[k]); }
    } else if (kind == 8) {
      const int pass = (int)(rnd() % 4);     // range / null / record refused, accepted
      old_write_nodes(&o[d], pass); new_write_nodes(&n[d], pass);
    } else if (kind == 9) {
      const int pass = (int)(rnd() % 3);
      const bool cs = rnd() & 1;
      old_write_queue(&o[d], pass, cs); new_write_queue(&n[d], pass, cs);
    } else if (kind == 10) {
      const int pass = (int)(rnd() % 3);
      old_write_arena(&o[d], pass); new_write_arena(&n[d], pass);
    } else if (kind == 11) {
      const int pass = (int)(rnd() % 3);
      old_write_commit_stream(&o[d], pass); new_write_commit_stream(&n[d], pass);
    } else if (kind == 12) {
      const int pass = (int)(rnd() % 2);
      const bool cursor = rnd() & 1;
      old_write_clusters(&o[d], pass, cursor); new_write_clusters(&n[d], pass, cursor);
    } else if (kind == 13) {
      const uint64_t H = 0xFFFFFFFFull - longest;           // the first tick past the horizon
      const uint64_t targets[] = {0, cfg.el_base - 1, cfg.el_base, (1ull << 31) - tpl - 1,
                                  (1ull << 31) - 1, 1ull << 31, H - 3ull * tpl - 1, H - 2, H - 1, H,
                                  (1ull << 32) + 5, rnd() % H};
      const uint64_t t = targets[rnd() % (sizeof targets / sizeof targets[0])];
      if (!horizon_ok(cfg, t, 0)) continue;
      for (int k = 0; k < G; ++k) {
        old_set_tick(&o[k], t); new_set_tick(&n[k], t);
        wrote_keys[k] = false;
      }
      handle_tick = t;
    } else if (kind == 14) {                 // a scatter: refused (nothing), or on a subset
      const uint32_t touched = (uint32_t)(rnd() % 4), general = (uint32_t)(rnd() % 4);
      if (rnd() % 4 == 0) continue;
      for (int k = 0; k < G; ++k)
        if ((touched >> k) & 1) {
          old_scatter(&o[k], (general >> k) & 1); new_scatter(&n[k], (general >> k) & 1);
          wrote_keys[k] = false;
        }
    } else {
      const uint32_t C = cfg.n_clusters;
      const uint32_t vals[] = {0, C / 16, C / 16 + 1, C};
      if (o[d].has_bail_host) o[d].bail_host = n[d].report = vals[rnd() % 4];
    }
    for (int k = 0; k < G; ++k) same_state(o[k], n[k], ev);
  }
}

static void every_configuration() {
  raft_sim_config_t base;
  memset(&base, 0, sizeof base);
  base.log_cap = 64; base.inbox_cap = 16; base.seed = 42; base.hb = 3000; base.el_span = 5000;
  base.dmin = base.dmax = 1; base.part_epoch = 1000; base.n_devices = 1;
  for (uint32_t N = 2; N <= 9; ++N)
  for (uint32_t spec = 0; spec < 2; ++spec)
  for (uint32_t trace = 0; trace < 2; ++trace)
  for (uint32_t client = 0; client < 2; ++client)
  for (uint32_t faults = 0; faults < 3; ++faults)
  for (uint32_t sched : {(uint32_t)RAFT_SCHED_ALIGNED, (uint32_t)RAFT_SCHED_FIXED})
  for (uint32_t tpl : {7u, 10000u, 65536u})
  for (int mode = 0; mode < 3; ++mode)
  for (int events = 0; events < 2; ++events)
  for (uint32_t C : {15u, 16u, 17u, 131071u, 131072u})
  for (uint32_t el_base : {5000u, (1u << 28) - 1, 1u << 28})
  for (uint32_t redirects : {15u, 16u}) {
    raft_sim_config_t c = base;
    c.nodes = N; c.n_clusters = C; c.el_base = el_base; c.client_redirects = redirects;
    c.variant_flags = spec ? RAFT_VARIANT_SPEC : 0;
    c.trace_cap = trace ? 8 : 0;
    c.client_ppm = client ? 20000 : 0;
    if (faults == 1) c.drop_ppm = 50000;
    if (faults == 2) c.dmax = 20;
    c.schedule = sched;
    c.ticks_per_launch = tpl;
    ++cfg_id;
    random_run(c, mode, events != 0, 24);
  }
  // the handles that can take the steady kernel, through many bail reports
  for (uint32_t N = 2; N <= 5; ++N)
  for (uint32_t sched : {(uint32_t)RAFT_SCHED_ALIGNED, (uint32_t)RAFT_SCHED_FIXED})
  for (uint32_t tpl : {7u, 10000u, 65536u})
  for (int mode = 0; mode < 3; ++mode)
  for (uint32_t C : {15u, 16u, 17u}) {
    raft_sim_config_t c = base;
    c.nodes = N; c.n_clusters = C; c.el_base = 5000; c.schedule = sched; c.ticks_per_launch = tpl;
    ++cfg_id;
    random_run(c, mode, false, 400, true);
  }
  // ticks_per_launch 0 is the default, and values above 65536 are clipped
  for (uint32_t tpl : {0u, 65537u, 0xFFFFFFFFu}) {
    raft_sim_config_t c = base;
    c.nodes = 5; c.n_clusters = 64; c.el_base = 5000; c.ticks_per_launch = tpl;
    ++cfg_id;
    random_run(c, 0, false, 200);
  }
}

// ---- hand-written expectations: the policy in words ---------------------------------------------
static raft_sim_config_t c2_shape() {
  raft_sim_config_t c;
  memset(&c, 0, sizeof c);
  c.n_clusters = 65536; c.nodes = 5; c.log_cap = 64; c.inbox_cap = 16; c.hb = 3000;
  c.el_base = 5000; c.el_span = 5000; c.dmin = c.dmax = 1; c.part_epoch = 1000;
  return c;
}
static const LaunchEnv env_auto = {STEADY_AUTO, false, STORM_MIN_CLUSTERS};
static const LaunchEnv env_never = {STEADY_NEVER, false, STORM_MIN_CLUSTERS};

static LaunchPlan one_launch(const LaunchFixed& f, LaunchState& s, uint32_t left, uint32_t report = 0) {
  const LaunchPlan p = plan_launch(f, s, left, report);
  launch_enqueued(s, p);
  return p;
}

static void expectations() {
  cfg_id = -1;
  // a fresh C2-shaped handle: steady for every launch, timed only the first of each sync window
  {
    const raft_sim_config_t c = c2_shape();
    const LaunchFixed f = launch_fixed(c, env_auto);
    LaunchState s = launch_state(c);
    expect(f.steady_ok && f.tpl == 10000 && s.lite && s.storm_until == 0, "C2: create");
    for (int window = 0; window < 3; ++window) {
      for (int i = 0; i < 25; ++i) {
        if (i == 0 || i == 20) invalidate(s, ON_STEP);       // two steps before the sync
        const LaunchPlan p = one_launch(f, s, 10000 * (uint32_t)(25 - i));
        expect(p.path == PATH_STEADY && p.nt == 10000 && p.sched == SCHED_NONE && !p.use_perm &&
                   !p.write_keys && !p.reset_report, "C2: every launch steady, unpacked", window, i);
        expect(p.timed == (i == 0), "C2: only a window's first launch is timed", window, i);
        expect(p.bail_parity == (uint32_t)((window * 25 + i) & 1), "C2: bail counters alternate", i);
      }
      synced(s);
    }
    expect(s.tick == 750000 && s.ticks_run == 750000, "C2: the clock", (long)s.tick);
  }
  // a report of C/16 + 1 before launch k: k and k + 1 LITE (timed), steady from k + 2, one reset
  for (uint32_t over : {0u, 1u}) {
    const raft_sim_config_t c = c2_shape();
    const LaunchFixed f = launch_fixed(c, env_auto);
    LaunchState s = launch_state(c);
    const uint32_t k = 3;
    uint32_t report = 0, resets = 0;
    for (uint32_t i = 0; i < 8; ++i) {
      if (i == k) report = c.n_clusters / 16 + over;
      const LaunchPlan p = one_launch(f, s, 80000 - 10000 * i, report);
      if (p.reset_report) { report = 0; ++resets; }
      const bool general = over && (i == k || i == k + 1);
      expect(p.path == (general ? PATH_LITE : PATH_STEADY), "bails: the path", over, i);
      expect(p.timed == (general || i == 0), "bails: general launches are timed", over, i);
      expect(p.reset_report == (over && i == k), "bails: the report is reset at launch k", over, i);
    }
    expect(resets == over, "bails: one reset", over, resets);
  }
  // a fresh client handle, el_base 5000, 10000 ticks per launch, a step of 20000
  for (uint32_t C : {131071u, 131072u}) {
    raft_sim_config_t c = c2_shape();
    c.n_clusters = C; c.client_ppm = 20000; c.client_redirects = 4;
    const LaunchFixed f = launch_fixed(c, env_auto);
    LaunchState s = launch_state(c);
    const uint32_t want_t0[3] = {0, 5000, 15000}, want_nt[3] = {5000, 10000, 5000};
    uint32_t left = 20000;
    for (int i = 0; i < 3; ++i) {
      const LaunchPlan p = one_launch(f, s, left);
      left -= p.nt;
      expect(p.t0 == want_t0[i] && p.nt == want_nt[i], "client: the launches", i, p.nt);
      const TickPath want = i ? PATH_GENERAL : C >= 131072 ? PATH_STORM_KERNEL : PATH_STORM_BODY;
      expect(p.path == want && p.timed, "client: storm first, then the general kernel", i, p.path);
    }
    expect(left == 0 && s.storm_kernel_ran == (C >= 131072), "client: the step is done", left);
  }
  // a lite aligned handle in mode never: id order, then the first packing when resort_ctr reaches
  // RESORT_EVERY_LITE, from the keys the launch before wrote
  {
    const raft_sim_config_t c = c2_shape();
    const LaunchFixed f = launch_fixed(c, env_never);
    LaunchState s = launch_state(c);
    for (uint32_t i = 0; i <= 2 * RESORT_EVERY_LITE; ++i) {
      expect(s.resort_ctr == i, "never: every launch counts", i, (long)s.resort_ctr);
      const LaunchPlan p = one_launch(f, s, 10000);
      expect(p.path == PATH_LITE && p.timed, "never: the LITE kernel, timed", i, p.path);
      const bool rebuild = i == RESORT_EVERY_LITE || i == 2 * RESORT_EVERY_LITE;
      expect(p.sched == (rebuild ? SCHED_PERM : SCHED_NONE), "never: rebuilt every 8th launch", i,
             p.sched);
      expect(p.use_perm == (i >= RESORT_EVERY_LITE), "never: id order until the first packing", i);
      expect(p.write_keys == (i % RESORT_EVERY_LITE == RESORT_EVERY_LITE - 1),
             "never: the launch before a rebuild writes the keys", i);
    }
  }
  // after set_tick the next rebuild computes its keys
  {
    const raft_sim_config_t c = c2_shape();
    const LaunchFixed f = launch_fixed(c, env_never);
    LaunchState s = launch_state(c);
    for (uint32_t i = 0; i < RESORT_EVERY_LITE; ++i) one_launch(f, s, 10000);
    expect(s.keys_written, "set_tick: launch 7 wrote keys");
    set_tick(s, 1000000);
    const LaunchPlan p = one_launch(f, s, 10000);
    expect(p.sched == SCHED_KEY_PERM && p.t0 == 1000000 && p.use_perm, "set_tick: keys from the state",
           p.sched);
  }
  // a steady launch writes no keys: the rebuild after it computes them, whatever the launch
  // before the steady one wrote
  {
    const raft_sim_config_t c = c2_shape();
    const LaunchFixed f = launch_fixed(c, env_auto);
    LaunchState s = launch_state(c);
    const uint32_t over = c.n_clusters / 16 + 1;
    for (uint32_t i = 0; i < RESORT_EVERY_LITE; ++i) {       // four reports, two LITE launches each
      const LaunchPlan p = one_launch(f, s, 10000, over);
      expect(p.path == PATH_LITE && p.write_keys == (i == RESORT_EVERY_LITE - 1),
             "steady between: the eighth general launch writes keys", i);
    }
    expect(one_launch(f, s, 10000, 0).path == PATH_STEADY, "steady between: a steady launch");
    const LaunchPlan p = one_launch(f, s, 10000, over);
    expect(p.path == PATH_LITE && p.sched == SCHED_KEY_PERM, "steady between: keys from the state",
           p.sched);
  }
  // which (N, SPEC, path) have a kernel
  for (uint32_t N = 0; N <= 11; ++N)
    for (int spec = 0; spec < 2; ++spec)
      for (int path = PATH_STEADY; path <= PATH_NONE; ++path) {
        const bool in = N >= 2 && N <= 9;
        const bool want = path == PATH_STEADY ? in && N <= 5 && !spec
                          : path == PATH_LITE ? in && !spec
                          : path == PATH_NONE ? false : in;
        expect(path_exists(N, spec, (TickPath)path) == want, "path_exists", N, path);
      }
}

int main() {
  every_configuration();
  expectations();
  printf("checks %ld bad %ld\n", checks, bad);
  return bad ? 1 : 0;
}
"""


def test_the_planner_is_the_old_policy_and_the_policy_is_what_the_words_say(tmp_path):
    out = hostprog.run_cpp(tmp_path, "launch_plan_check", PROGRAM,
                           sanitizers=("undefined", "address"), timeout=300)
    assert hostprog.checks(out) > 10000000
