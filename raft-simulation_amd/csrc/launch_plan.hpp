// launch_plan.hpp — what a tick launch is, decided once on the host: which kernel runs, whether
// the launch is packed, whether it writes packing keys, whether it carries an event pair, and
// which host calls change those answers for the next launch. raftsim.hip holds the HIP objects
// and does what a plan says; the launchers (tick_kernel.hip) dispatch on the plan's path. Every
// choice here is speed only: any path and any packing give the same state, so no GPU test sees
// it. Includes nothing from HIP: compiles under hipcc with raftsim.hip and under plain g++ with
// include/raftsim.h alone (tests/test_launch_plan_host.py runs it on the CPU).
#pragma once
#include <assert.h>
#include <stdint.h>

#include "../../include/raftsim.h"

namespace rs {

// The kernel a tick launch runs.
enum TickPath : uint8_t {
  PATH_STEADY,         // steady_kernel.hip: one lane per cluster, bails through tick_wave
  PATH_STORM_KERNEL,   // storm_kernel.hip: one lane per cluster, the STORM body over its leftovers
  PATH_STORM_BODY,     // tick_kernel<N, false, SPEC, false, STORM>
  PATH_TRACE,          // tick_kernel<N, true, SPEC, false>
  PATH_LITE,           // tick_kernel<N, false, false, true>
  PATH_GENERAL,        // tick_kernel<N, false, SPEC, false>
  PATH_NONE            // no launch yet (LaunchState::last_path)
};

// Which (N, SPEC, path) have a kernel. The launchers refuse the others (hipErrorInvalidValue) by
// asking this, and the planner chooses STEADY and LITE by asking it too: there is no second list.
constexpr bool path_exists(uint32_t N, bool spec, TickPath path) {
  if (N < 2 || N > RAFT_MAX_NODES) return false;
  switch (path) {
    case PATH_STEADY: return N <= 5 && !spec;
    case PATH_LITE: return !spec;
    case PATH_STORM_KERNEL:
    case PATH_STORM_BODY:
    case PATH_TRACE:
    case PATH_GENERAL: return true;
    case PATH_NONE: break;
  }
  return false;
}

// After a catch-up launch that took more than 1/16 of the clusters, this many launches take the
// general path (LaunchFixed::steady_mode).
constexpr uint32_t STEADY_COOLDOWN = 2;
// The wave packing is rebuilt every RESORT_EVERY-th tick launch and reused in between: with
// key-pure waves a steady-state cluster keeps its wave mates' phase, so a packing stays good for
// more than one 10k-tick launch, and skipping the schedule kernel (C2: 14.6 us) every other
// launch measured C2 step wall 0.127 -> 0.119 ms with the tick kernel unchanged (every 4th: no
// further gain). Results never depend on the packing.
constexpr uint32_t RESORT_EVERY = 2;
// LITE handles: a steady-state packing is a rotation of itself one launch later (every cluster's
// next event moves by the same launch length), so it is rebuilt every 8th launch
constexpr uint32_t RESORT_EVERY_LITE = 8;
// Clusters per handle from which storm ticks run the storm kernel. One lane per cluster needs
// clusters enough to fill the chip (two 64-cluster waves per SIMD at least: at C4's 16,384
// clusters its 256 waves ran 36 ms against the lane-per-node body's 14): below that the storm
// ticks run the general STORM body.
constexpr uint32_t STORM_MIN_CLUSTERS = 131072;

enum SteadyMode : uint8_t { STEADY_AUTO, STEADY_ALWAYS, STEADY_NEVER };

// What raft_sim_create reads from the environment (raftsim.hip keeps the getenv calls).
struct LaunchEnv {
  SteadyMode steady_mode;        // RAFTSIM_STEADY: auto (default), always, never
  bool launch_events;            // RAFTSIM_LAUNCH_EVENTS=1
  uint32_t storm_min_clusters;   // STORM_MIN_CLUSTERS; diagnostic builds may override it
};

// What is fixed at create.
struct LaunchFixed {
  uint32_t N, C;
  uint32_t tpl;            // ticks per launch at most
  uint32_t resort_every;   // rebuild period of the packing
  bool spec, trace, client, aligned;   // Spec-Raft, trace rings, client traffic, the schedule
  // steady kernel (steady_kernel.hip): LITE launches at N <= 5 without TRACE
  bool steady_ok;
  // Path choice per launch. auto: the steady kernel unless the last catch-up launch the host has
  // seen (the bail report, written by the GPU; a few launches stale at most) took more than 1/16
  // of the clusters, then the general kernel for the next STEADY_COOLDOWN launches. The first
  // launch of a handle is steady too: the steady kernel runs init-node's election in closed form
  // (steady_kernel.hip). always / never force a path.
  SteadyMode steady_mode;
  bool storm_kernel;       // the storm kernel's leftover list exists: storm ticks run that kernel
  // Start/stop events in a launch's dispatch packet time the kernel alone, but measured 8.2 against
  // 2.5 us per back-to-back launch of an empty kernel on MI355X (scripts/launch_probe.hip): a
  // steady-path launch (~0.025 ms at C2) carries them only when it is the first after a sync
  // (the kernel time reported is that launch's); general-kernel launches (milliseconds, and their
  // cost changes over a run as logs grow and nodes halt) are all timed. launch_events times every
  // launch (diagnostic).
  bool launch_events;
};

// What changes between launches.
struct LaunchState {
  uint64_t tick;        // the shard's next tick
  uint64_t ticks_run;   // ticks simulated by this handle (node_ticks counts these)
  // No client traffic (and no finite client cursor, no queued client-set), no faults, fixed delay:
  // the LITE and steady kernels can run. Host writes clear it; nothing sets it again.
  bool lite;
  // Ticks before this one are storm ticks (tick_wave.hpp, STORM): the handle is fresh from
  // init-node with client traffic, so no timer fires before el_base and the only events are
  // client-sets at followers. Any host write of state or of the clock ends it (0).
  uint32_t storm_until;
  // RAFT_SCHED_ALIGNED. keys_written: the last tick launch wrote every cluster's key and the
  // matching histogram; otherwise a rebuild zeroes the histogram and computes both from the state
  // (sched_key). Stale keys (after host writes or set_tick) change the packing (speed), never the
  // results; a histogram always counts each cluster once, so a packing always places each cluster
  // once. packed: a packing has been built (until then a launch runs in id order).
  bool keys_written, packed;
  uint64_t resort_ctr;         // RAFT_SCHED_ALIGNED: non-steady tick launches since create
  uint32_t steady_cooldown;    // launches left on the general path (STEADY_AUTO)
  uint32_t steady_parity;      // the two bail counters alternate between steady launches
  uint32_t window_launch;      // launches enqueued since the last sync
  TickPath last_path;          // the last tick launch's (raftsim_diag_last_bails)
  bool storm_kernel_ran;       // a storm-kernel launch has run (raftsim_diag_storm_bails)
  // The audit's records and folded summary are those of the state as it stands; every call that
  // can change a log or a commit index clears it, so queries in between walk the arenas once.
  bool audit_valid;
};

constexpr bool cfg_lite(const raft_sim_config_t& c) {
  return c.client_ppm == 0 && c.drop_ppm == 0 && c.dup_ppm == 0 && c.part_ppm == 0 &&
         c.dmin == c.dmax;
}
// init-node's deadlines are el_base or more ahead and every re-arm is too (SIM_SPEC D4; the
// Spec-Raft control re-arms on fewer events): until el_base, client-sets are the only events.
// Not with trace rings: the STORM body has no TRACE instantiation.
constexpr uint32_t cfg_storm_until(const raft_sim_config_t& c) {
  return c.client_ppm && !c.trace_cap ? c.el_base : 0u;
}

// cfg: a shard's own (its cluster count).
inline LaunchFixed launch_fixed(const raft_sim_config_t& cfg, const LaunchEnv& env) {
  LaunchFixed f = {};
  f.N = cfg.nodes;
  f.C = cfg.n_clusters;
  f.tpl = cfg.ticks_per_launch ? (cfg.ticks_per_launch < 65536u ? cfg.ticks_per_launch : 65536u)
                               : 10000u;
  f.resort_every = cfg_lite(cfg) ? RESORT_EVERY_LITE : RESORT_EVERY;
  f.spec = cfg.variant_flags & RAFT_VARIANT_SPEC;
  f.trace = cfg.trace_cap != 0;
  f.client = cfg.client_ppm != 0;
  f.aligned = cfg.schedule == RAFT_SCHED_ALIGNED;
  f.steady_ok = cfg_lite(cfg) && !f.trace && path_exists(f.N, f.spec, PATH_STEADY);
  f.steady_mode = env.steady_mode;
  // the storm kernel's registers hold arrivals below 2^28 and hop counts below 16
  f.storm_kernel = cfg_storm_until(cfg) && f.C >= env.storm_min_clusters &&
                   cfg.el_base < (1u << 28) && cfg.client_redirects < 16;
  f.launch_events = env.launch_events;
  return f;
}

inline LaunchState launch_state(const raft_sim_config_t& cfg) {
  LaunchState s = {};
  s.lite = cfg_lite(cfg);
  s.storm_until = cfg_storm_until(cfg);
  s.last_path = PATH_NONE;
  return s;
}

// The schedule kernels a launch runs first.
enum SchedPrep : uint8_t { SCHED_NONE, SCHED_PERM, SCHED_KEY_PERM };

struct LaunchPlan {
  uint32_t t0, nt;       // t0: the 32-bit clock of the launch's first tick
  TickPath path;
  SchedPrep sched;       // rebuild the packing first: from the written keys, or compute them at t0
  bool use_perm;         // run under the packing (else clusters in id order: DevSim::perm null)
  bool write_keys;       // the launch writes keys and histogram (else DevSim::shist null)
  bool timed;            // carries an event pair
  bool reset_report;     // zero the bail report word before the launch
  uint32_t bail_parity;  // PATH_STEADY: counts into bail counter [parity], zeroes [parity ^ 1]
};

// Plan the next launch of a step with ticks_left > 0 to go and advance what the choice depends on;
// launch_enqueued advances the clock once the launch stands in the stream. bail_report: the word
// the GPU reports the last catch-up launch's clusters in (0 where there is none).
//
// Implied, so not asked: a storm launch is never steady, LITE or traced. storm_until is nonzero
// only for a handle created with client traffic and without trace rings, cfg_lite needs no client
// traffic, and nothing sets lite or storm_until after create: t0 < storm_until implies !lite and
// !trace, and lite implies storm_until == 0.
inline LaunchPlan plan_launch(const LaunchFixed& f, LaunchState& s, uint32_t ticks_left,
                              uint32_t bail_report) {
  LaunchPlan p = {};
  p.t0 = (uint32_t)s.tick;
  p.nt = f.tpl < ticks_left ? f.tpl : ticks_left;
  // storm ticks run alone in a launch of their own
  const bool storm = p.t0 < s.storm_until;
  if (storm && p.nt > s.storm_until - p.t0) p.nt = s.storm_until - p.t0;
  assert(!storm || (!s.lite && !f.trace));

  bool steady = f.steady_ok && s.lite && f.steady_mode != STEADY_NEVER;
  if (steady && f.steady_mode == STEADY_AUTO) {
    if (s.steady_cooldown) {
      --s.steady_cooldown;
      steady = false;
    } else if (bail_report > f.C / 16) {
      p.reset_report = true;
      s.steady_cooldown = STEADY_COOLDOWN - 1;
      steady = false;
    }
  }
  if (steady) p.path = PATH_STEADY;
  else if (storm) p.path = f.storm_kernel ? PATH_STORM_KERNEL : PATH_STORM_BODY;
  else if (f.trace) p.path = PATH_TRACE;
  else if (s.lite && path_exists(f.N, f.spec, PATH_LITE)) p.path = PATH_LITE;
  else p.path = PATH_GENERAL;

  if (steady) {
    // the steady kernel runs the clusters in id order: no packing, no keys. (Packed by next
    // event, 64 to a wave, the same launch took 0.0329 against 0.0318 ms: a lane runs its own
    // cluster's clock, and the packing's perm load sat in front of every state load.)
    s.keys_written = false;
    p.bail_parity = s.steady_parity;
    s.steady_parity ^= 1;
  } else if (f.aligned && s.resort_ctr == 0 && !f.client) {
    // The handle's first general launch without client traffic (every cluster from init-node or as
    // the host wrote it): clusters in id order. Per-cluster clocks make a wave's trips its busiest
    // cluster's event ticks whatever its mates are, and the packing's key and sort kernels
    // measured +35-40 us on the 100-us first launch of 65,536 clusters (scripts/init_probe.py).
    // Keys are not written: the launch before the first rebuild writes them.
    s.keys_written = false;
    ++s.resort_ctr;
  } else if (f.aligned) {
    // pack clusters with the same next event onto the same waves for this launch: keys and
    // histogram come from the previous tick launch, or are computed from the state. The packing
    // is rebuilt every resort_every-th launch and reused in between (any packing gives the same
    // results); only the launch before a rebuild writes keys.
    if (s.resort_ctr % f.resort_every == 0) {
      p.sched = s.keys_written ? SCHED_PERM : SCHED_KEY_PERM;
      s.packed = true;
    }
    ++s.resort_ctr;
    s.keys_written = s.resort_ctr % f.resort_every == 0;   // the next launch rebuilds
    p.use_perm = s.packed;
    p.write_keys = s.keys_written;
  }
  p.timed = f.launch_events || s.window_launch == 0 || !steady;
  s.last_path = p.path;
  if (p.path == PATH_STORM_KERNEL) s.storm_kernel_ran = true;
  return p;
}

// The planned launch stands in the stream: the clock advances launch by launch, so after a failed
// enqueue it still names the tick the state has reached.
inline void launch_enqueued(LaunchState& s, const LaunchPlan& p) {
  s.tick += p.nt;
  s.ticks_run += p.nt;
  ++s.window_launch;
}
inline void synced(LaunchState& s) { s.window_launch = 0; }

// ---- The host calls that change the state: what each invalidates, and at which of its checks.
// A call refused before the named check leaves the state alone; one refused after it has marked.
enum Invalidates : uint32_t {
  INV_STORM = 1,   // storm_until = 0: the state is no longer init-node's
  INV_AUDIT = 2,   // audit_valid = false: a log or a commit index may have changed
  INV_KEYS = 4,    // keys_written = false: the next rebuild computes its keys from the state
  INV_LITE = 8     // lite = false: a client-set is queued or due, the general kernel is needed
};
// a step, before anything is enqueued (a step of 0 ticks too)
constexpr uint32_t ON_STEP = INV_AUDIT;
// raft_sim_write_nodes, per shard: after the range check and before the null and record checks, so
// a write refused for a bad record has already ended the storm ticks
constexpr uint32_t ON_WRITE_NODES = INV_STORM | INV_AUDIT;
// raft_sim_write_queue: after the node check, before the queue is validated ...
constexpr uint32_t ON_WRITE_QUEUE = INV_STORM;
// ... and once the queue has passed, when it holds a client-set
constexpr uint32_t ON_QUEUED_CLIENT_SET = INV_LITE;
// raft_sim_write_arena: after the node check, before the count is checked
constexpr uint32_t ON_WRITE_ARENA = INV_STORM | INV_AUDIT;
// raft_sim_write_commit_stream: after the node check, before the count is checked (like the queue
// write it changes neither a log nor a commit index: audit_valid stays)
constexpr uint32_t ON_WRITE_COMMIT_STREAM = INV_STORM;
// raft_sim_write_clusters, per shard: after the range check (its only one) ...
constexpr uint32_t ON_WRITE_CLUSTERS = INV_STORM | INV_AUDIT;
// ... and for a record whose client cursor is finite (a client-set is due: P0 is needed)
constexpr uint32_t ON_CLIENT_CURSOR = INV_LITE;
// raft_sim_set_tick, per shard once it is synced (with the tick itself, set_tick below): the
// packing keys are relative to the next launch's first tick
constexpr uint32_t ON_SET_TICK = INV_STORM | INV_KEYS;
// raft_scatter_write, per touched shard: every check has passed by then (a refused scatter has
// touched nothing) ...
constexpr uint32_t ON_SCATTER = INV_STORM | INV_AUDIT | INV_KEYS;
// ... and when one of the shard's records needs the general kernel (scatter_host.hpp)
constexpr uint32_t ON_SCATTER_GENERAL = INV_LITE;
// raft_clone_write, per touched target shard: what a scatter of the same clusters marks, and like
// it after every check (a refused clone has touched nothing; the source shards are only read and
// keep their state) ...
constexpr uint32_t ON_CLONE = ON_SCATTER;
// ... and when a shard it reads from is no longer LITE: a cloned cluster may then carry a finite
// client cursor or a queued client-set (no record is looked at on the host)
constexpr uint32_t ON_CLONE_GENERAL = ON_SCATTER_GENERAL;
// raft_restart_write, per touched shard, and raft_restart_where, every shard: what a scatter of the
// same clusters marks, after every check (a refused restart has touched nothing). A restart only
// removes queued client-sets and leaves the client cursor, so it never needs INV_LITE
constexpr uint32_t ON_RESTART = ON_SCATTER;

inline void invalidate(LaunchState& s, uint32_t what) {
  if (what & INV_STORM) s.storm_until = 0;
  if (what & INV_AUDIT) s.audit_valid = false;
  if (what & INV_KEYS) s.keys_written = false;
  if (what & INV_LITE) s.lite = false;
}
inline void set_tick(LaunchState& s, uint64_t tick) {
  s.tick = tick;
  invalidate(s, ON_SET_TICK);
}

}  // namespace rs
