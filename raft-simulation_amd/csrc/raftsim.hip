// raftsim.hip — C ABI of libraftsim.so (include/raftsim.h) over the gfx950 tick kernel.
#include <errno.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "clone_host.hpp"
#include "launch_plan.hpp"
#include "node_codec.hpp"
#include "restart_host.hpp"
#include "scatter_host.hpp"
#include "summary_host.hpp"

namespace rs {
hipError_t launch_tick(const DevSim& S, TickPath path, uint32_t t0, uint32_t nt, hipStream_t st,
                       hipEvent_t ev0, hipEvent_t ev1);
hipError_t launch_sched_key(const DevSim& S, uint32_t t0, hipStream_t st);
hipError_t launch_sched_perm(const DevSim& S, uint32_t* zero, uint32_t* perm, uint32_t* nslots,
                             hipStream_t st);
hipError_t launch_init(const DevSim& S, hipStream_t st);
hipError_t launch_digest(const DevSim& S, uint32_t c0, uint32_t nc, unsigned long long* out,
                         hipStream_t st);
hipError_t configure_kernels();
// violations_kernel.hip
hipError_t launch_viol_clear(const DevSim& S, hipStream_t st);
size_t viol_scratch_words(uint32_t C);
const uint32_t* viol_total_ptr(const uint32_t* scratch, uint32_t C);
hipError_t launch_viol_query(const DevSim& S, uint32_t kinds, uint64_t t_lo, uint64_t t_hi,
                             uint32_t* scratch, void* out, uint32_t cap, hipStream_t st);
// census_kernel.hip (its scratch: summary_host.hpp, census_layout)
hipError_t launch_census(const DevSim& S, unsigned long long* scratch, hipStream_t st);
hipError_t launch_census_select(const DevSim& S, uint32_t any, uint32_t all, uint32_t none,
                                unsigned long long* scratch, void* out, uint32_t cap,
                                hipStream_t st);
// audit_kernel.hip (its scratch: audit_layout)
hipError_t launch_audit(const DevSim& S, uint32_t width, void* rec, unsigned long long* scratch,
                        hipStream_t st);
hipError_t launch_audit_select(uint32_t C, uint32_t any, uint32_t all, uint32_t none,
                               const void* rec, unsigned long long* scratch, void* out,
                               uint32_t cap, hipStream_t st);
// gather_kernel.hip
hipError_t launch_gather(const DevSim& S, const void* pairs, uint32_t n,
                         const raft_gather_layout_t& Y, void* out, hipStream_t st);
// scatter_kernel.hip
hipError_t launch_scatter(const DevSim& S, const void* pairs, uint32_t n,
                          const raft_gather_layout_t& Y, const void* in, hipStream_t st);
hipError_t launch_clone(const DevSim& T, const DevSim& Src, const void* pairs, uint32_t n,
                        uint64_t stride, hipStream_t st);
hipError_t launch_restart(const DevSim& S, const void* pairs, uint32_t n, uint32_t mode, uint32_t T,
                          hipStream_t st);
hipError_t launch_restart_where(const DevSim& S, uint32_t fault_mask, uint32_t mode, uint32_t T,
                                uint32_t* count, hipStream_t st);
}  // namespace rs

using rs::DevSim;

static thread_local char g_err[512];

static int fail(int code, const char* fmt, const char* detail = "") {
  snprintf(g_err, sizeof g_err, fmt, detail);
  return code;
}

static int unusable() {
  return fail(-EIO, "a previous step failed part-way; the handle is unusable");
}

#define HIP_OK(expr)                                                               \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return fail(-EIO, "HIP error: %s (" #expr ")",           \
                                      hipGetErrorString(e_));                      \
  } while (0)

struct Shard {
  raft_sim_config_t cfg;
  uint32_t N, Q, L, A, C, NN;
  // What a tick launch is (launch_plan.hpp): fixed at create, and what changes between launches
  rs::LaunchFixed lf;
  rs::LaunchState ls;
  hipStream_t stream;
  hipEvent_t ev_start, ev_stop;
  std::vector<uint8_t> ktimed;   // per launch since the last sync: carries an event pair
  std::vector<hipEvent_t> kev;   // per tick-kernel launch of a step: start, stop
  DevSim d;
  std::vector<void*> allocs;
  double last_ms, last_step_ms;
  uint32_t last_timed;           // launches of the last sync window that carried an event pair
  bool pending;                  // a step has been enqueued since the last sync
  uint32_t last_launches;
  unsigned long long* client_pw;
  // RAFT_SCHED_ALIGNED: the spare histogram (the schedule kernel zeroes it while reading d.shist;
  // the two swap every rebuild) and the wave-slot -> cluster map of the next launch
  uint32_t *soff, *sperm, *snslots;   // + the slot count of the packing
  uint32_t* nbail2;                    // the steady kernel's two bail counters (lf.steady_ok)
  uint32_t* bail_host;                 // the bail report: a host-mapped word (hipHostMalloc)
  // The device-side queries. qev0 / qev1: the events around a query's kernels. raft_viol_read: the
  // compaction's scratch (violations_kernel.hip) and the device time of the last query
  // (raftsim_diag_viol_ms). raft_census_read / raft_census_select (census_kernel.hip): their
  // scratch, made by the first query, and the last query's device time (raftsim_diag_census_ms).
  hipEvent_t qev0, qev1;
  uint32_t* vscratch;
  double viol_ms;
  unsigned long long* cscratch;
  double census_ms;
  // raft_audit_read / raft_audit_select (audit_kernel.hip): the per-cluster records and the
  // scratch (partial and folded summaries, the compaction's counts), made by the first query, and
  // the last query's device time (raftsim_diag_audit_ms). The records and the folded summary are
  // valid while ls.audit_valid (launch_plan.hpp has the calls that clear it).
  raft_audit_record_t* arec;
  unsigned long long* ascratch;
  double audit_ms;
  // raft_gather_read (gather_kernel.hip): the device scratch its records are packed into and the
  // (cluster, slot) list behind them in the same allocation, made and grown by the queries up to
  // GATHER_SCRATCH_BYTES; an event pair per chunk of a query; the device time of the last query's
  // kernels (raftsim_diag_gather_ms).
  uint8_t* gscratch;
  size_t gscratch_bytes;
  std::vector<hipEvent_t> gev;
  double gather_ms;
  // raft_scatter_write (scatter_kernel.hip) uploads its records and lists into the same scratch and
  // times its chunks' kernels with the same events (raftsim_diag_scatter_ms); pack_scratch,
  // pack_events and pack_wait below serve both calls.
  double scatter_ms;
  // raft_clone_write (clone_kernel, scatter_kernel.hip) uploads its lists of pairs into the same
  // scratch and times its chunks' kernels with the same events (raftsim_diag_clone_ms). cev: as a
  // source shard, the event the target shard's stream waits for before it reads this shard.
  hipEvent_t cev;
  double clone_ms;
  // raft_restart_write / raft_restart_where (restart_kernel, restart_where_kernel,
  // scatter_kernel.hip) upload their list, or keep their counter, in the same scratch and time
  // their kernels with the same events (raftsim_diag_restart_ms).
  double restart_ms;
};

// Exported functions take their C linkage from the declarations in include/raftsim.h.

const char* raft_sim_last_error(void) { return g_err; }
int raft_sim_abi_version(void) { return RAFT_SIM_ABI_VERSION; }

void raft_sim_default_config(raft_sim_config_t* c) {
  memset(c, 0, sizeof *c);
  c->n_clusters = 1; c->nodes = 5; c->log_cap = 64; c->inbox_cap = 16; c->seed = 42;
  c->hb = 3000; c->el_base = 5000; c->el_span = 5000; c->dmin = 1; c->dmax = 1;
  c->part_epoch = 1000; c->n_devices = 1;
}

static int validate_cfg(const raft_sim_config_t* c) {
  if (c->nodes < 2 || c->nodes > RAFT_MAX_NODES) return fail(-EINVAL, "nodes must be 2..9");
  if (c->n_clusters == 0) return fail(-EINVAL, "n_clusters must be > 0");
  if ((uint64_t)c->n_clusters * c->nodes > 0x7FFFFFFFull) return fail(-EINVAL, "too many nodes");
  if (c->inbox_cap < 1 || c->inbox_cap > RAFT_MAX_INBOX) return fail(-EINVAL, "inbox_cap 1..16");
  if (c->log_cap < 1 || c->log_cap > 65535) return fail(-EINVAL, "log_cap 1..65535");
  uint64_t A = c->arena_cap ? c->arena_cap : 4ull * c->log_cap;
  if (A < 2ull * c->log_cap || A > (1u << 24))
    return fail(-EINVAL, "arena_cap must be >= 2*log_cap");
  if (c->hb < 1 || c->el_base < 1) return fail(-EINVAL, "hb and el_base must be >= 1");
  if (c->dmin < 1 || c->dmax < c->dmin || c->dmax > 255)
    return fail(-EINVAL, "1 <= dmin <= dmax <= 255");
  if (c->part_epoch < 1) return fail(-EINVAL, "part_epoch must be >= 1");
  if (c->drop_ppm > 1000000 || c->dup_ppm > 1000000 || c->part_ppm > 1000000 ||
      c->client_ppm > 1000000)
    return fail(-EINVAL, "ppm values must be <= 1e6");
  if (c->variant_flags & ~3u) return fail(-EINVAL, "variant_flags: only bits 0-1 are defined");
  if (c->schedule > RAFT_SCHED_FIXED) return fail(-EINVAL, "schedule: 0 (aligned) or 1 (fixed)");
  if (c->trace_cap > (1u << 20) || c->trace_entry_cap > (1u << 24))
    return fail(-EINVAL, "trace_cap <= 2^20, trace_entry_cap <= 2^24");
  if ((uint64_t)c->cluster_offset + c->n_clusters > (1ull << 32))
    return fail(-EINVAL, "cluster_offset + n_clusters must be <= 2^32");
  if ((uint64_t)c->nodes * c->nodes * c->n_clusters >= (1ull << 31))
    return fail(-EINVAL, "nodes^2 * n_clusters must be < 2^31");
  if (c->client_period && (c->client_burst < 1 || c->client_burst > c->client_period))
    return fail(-EINVAL, "client_burst must be 1..client_period");
  if (c->client_redirects > 16) return fail(-EINVAL, "client_redirects <= 16");
  if (c->n_devices < 0 || c->n_devices > 64) return fail(-EINVAL, "n_devices 0..64");
  return 0;
}

// Zero every copy of the counter block, with "no violation" (UINT64_MAX) in the first-violation
// slots (rs::CTR_COPIES copies of rs::CTR_STRIDE words, reduced by sh_read_counters).
static hipError_t init_counters(Shard* s) {
  std::vector<unsigned long long> c((size_t)rs::CTR_COPIES * rs::CTR_STRIDE, 0ull);
  for (int k = 0; k < rs::CTR_COPIES; ++k) c[(size_t)k * rs::CTR_STRIDE + RAFT_CTR_COUNT] = ~0ull;
  return hipMemcpy(s->d.ctr, c.data(), c.size() * 8, hipMemcpyHostToDevice);   // blocking: c dies
}

template <typename T>
static int dalloc(Shard* s, T** p, size_t count) {
  void* v = nullptr;
  hipError_t e = hipMalloc(&v, std::max<size_t>(count, 1) * sizeof(T));
  if (e != hipSuccess) return fail(-ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
  s->allocs.push_back(v);
  *p = static_cast<T*>(v);
  return 0;
}

static void sh_destroy(Shard* s) {
  if (!s) return;
  (void)hipSetDevice(s->cfg.device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (void* p : s->allocs) (void)hipFree(p);
  if (s->bail_host) (void)hipHostFree(s->bail_host);
  if (s->ev_start) (void)hipEventDestroy(s->ev_start);
  if (s->ev_stop) (void)hipEventDestroy(s->ev_stop);
  if (s->qev0) (void)hipEventDestroy(s->qev0);
  if (s->qev1) (void)hipEventDestroy(s->qev1);
  if (s->cev) (void)hipEventDestroy(s->cev);
  for (hipEvent_t e : s->kev) (void)hipEventDestroy(e);
  for (hipEvent_t e : s->gev) (void)hipEventDestroy(e);
  if (s->gscratch) (void)hipFree(s->gscratch);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

// What raft_sim_create reads from the environment for the launch plan.
static rs::LaunchEnv launch_env() {
  rs::LaunchEnv env = {rs::STEADY_AUTO, false, rs::STORM_MIN_CLUSTERS};
  const char* m = getenv("RAFTSIM_STEADY");
  if (m && !strcmp(m, "always")) env.steady_mode = rs::STEADY_ALWAYS;
  if (m && !strcmp(m, "never")) env.steady_mode = rs::STEADY_NEVER;
  const char* le = getenv("RAFTSIM_LAUNCH_EVENTS");
  env.launch_events = le && !strcmp(le, "1");
#ifdef RS_DIAG_BUILD   // scripts/storm_probe.py forces either path; the product takes no override
  if (const char* sm = getenv("RAFTSIM_STORM_MIN_CLUSTERS"))
    env.storm_min_clusters = (uint32_t)strtoul(sm, nullptr, 10);
#endif
  return env;
}

// Everything of sh_create that can fail once the shard exists: the caller destroys it on failure.
static int sh_init(Shard* s, const raft_sim_config_t* cfg) {
  int rc = 0;
  s->cfg = *cfg;
  s->N = cfg->nodes; s->Q = cfg->inbox_cap; s->L = cfg->log_cap; s->C = cfg->n_clusters;
  s->A = cfg->arena_cap ? cfg->arena_cap : 4 * cfg->log_cap;
  s->NN = s->C * s->N;
  s->lf = rs::launch_fixed(*cfg, launch_env());
  s->ls = rs::launch_state(*cfg);
  DevSim& d = s->d;
  d.C = s->C; d.N = s->N; d.Q = s->Q; d.L = s->L; d.A = s->A; d.NN = s->NN;
  d.goff = cfg->cluster_offset;
  d.key0 = (uint32_t)cfg->seed; d.key1 = (uint32_t)(cfg->seed >> 32);
  d.hb = cfg->hb; d.el_base = cfg->el_base; d.el_span = cfg->el_span;
  d.drop_ppm = cfg->drop_ppm; d.dup_ppm = cfg->dup_ppm; d.dmin = cfg->dmin; d.dmax = cfg->dmax;
  d.part_ppm = cfg->part_ppm; d.part_epoch = cfg->part_epoch; d.client_ppm = cfg->client_ppm;
  d.variant = cfg->variant_flags;
  d.client_period = cfg->client_period; d.client_burst = cfg->client_burst;
  d.client_redirects = cfg->client_redirects;
  d.div_period = rs::make_div(cfg->client_period ? cfg->client_period : 1);
  d.div_burst = rs::make_div(cfg->client_burst ? cfg->client_burst : 1);
  d.div_epoch = rs::make_div(cfg->part_epoch);
  d.SC = cfg->commit_stream_cap;
  d.TC = cfg->trace_cap;
  d.TE = cfg->trace_entry_cap;
  uint64_t pw[32];
  rs::client_powers(cfg->client_ppm, pw);
  d.client_pw = nullptr;
  d.lite = s->ls.lite;   // no kernel reads it and the host reads ls.lite: it keeps this value
  d.client_top = -1;
  for (int i = 0; i < 32; ++i)
    if (pw[i]) d.client_top = i;
  if (pw[0] >> 32) d.client_top = 32;   // client_ppm == 0: every power is 2^32 (rs::client_gap)
  const size_t NN = s->NN;
  d.HB = rs::hot_block_words(s->N);
  if ((rc = dalloc(s, &d.hot, (size_t)s->C * d.HB)) ||
      (rc = dalloc(s, &d.qbuf, NN * 2 * s->Q * 8)) ||
      (rc = dalloc(s, &d.arena, (NN * (size_t)s->A + rs::ARENA_PAD_SLOTS) * 2)) ||
      (rc = dalloc(s, &d.ctr, (size_t)rs::CTR_COPIES * rs::CTR_STRIDE)) || (rc = dalloc(s, &s->client_pw, 32)) ||
      (rc = dalloc(s, &d.ccount, NN)) ||
      (rc = dalloc(s, &d.stream, NN * std::max<uint32_t>(cfg->commit_stream_cap, 1))) ||
      (rc = dalloc(s, &d.tr, NN * std::max<uint32_t>(d.TC, 1) * 32)) ||
      (rc = dalloc(s, &d.tcount, NN)) ||
      (rc = dalloc(s, &d.tent, NN * std::max<uint32_t>(d.TE, 1))) ||
      (rc = dalloc(s, &d.tecount, NN)) ||
      (rc = dalloc(s, &d.viol, (size_t)s->C * 4)) ||
      (rc = dalloc(s, &s->vscratch, rs::viol_scratch_words(s->C))))
    return rc;
  d.client_pw = s->client_pw;
  d.wavelog = nullptr;
#ifdef RS_WAVELOG
  if ((rc = dalloc(s, &d.wavelog, (size_t)rs::sched_slots_bound(s->C, s->N) * 12))) return rc;
#endif
  if (s->lf.steady_ok && (rc = dalloc(s, &s->nbail2, 2))) return rc;
  // the storm kernel's leftover list (storm_kernel.hip)
  if (s->lf.storm_kernel &&
      ((rc = dalloc(s, &d.storm_list, s->C)) || (rc = dalloc(s, &d.storm_count, 1))))
    return rc;
  if (s->lf.steady_ok) {
    void* hp = nullptr;
    if (hipHostMalloc(&hp, sizeof(uint32_t), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&d.bail_report), hp, 0) != hipSuccess) {
      if (hp) (void)hipHostFree(hp);
      return fail(-ENOMEM, "hipHostMalloc (bail report) failed");
    }
    s->bail_host = static_cast<uint32_t*>(hp);
    *s->bail_host = 0;
  }
  if (s->lf.aligned &&
      ((rc = dalloc(s, &d.skey, s->C)) || (rc = dalloc(s, &d.shist, rs::SCHED_BUCKETS)) ||
       (rc = dalloc(s, &s->soff, rs::SCHED_BUCKETS)) ||
       (rc = dalloc(s, &s->sperm, rs::sched_slots_bound(s->C, s->N))) ||
       (rc = dalloc(s, &s->snslots, 1))))
    return rc;
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&s->ev_start)) != hipSuccess ||
      (e = hipEventCreate(&s->ev_stop)) != hipSuccess ||
      (e = hipEventCreate(&s->qev0)) != hipSuccess ||
      (e = hipEventCreate(&s->qev1)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&s->cev, hipEventDisableTiming)) != hipSuccess ||
      (e = hipMemsetAsync(d.hot, 0, (size_t)s->C * d.HB * 4, s->stream)) != hipSuccess ||
      (e = hipMemsetAsync(d.qbuf, 0, NN * 2 * s->Q * 32, s->stream)) != hipSuccess ||
      (e = hipMemsetAsync(d.arena, 0, (NN * (size_t)s->A + rs::ARENA_PAD_SLOTS) * 8, s->stream)) != hipSuccess ||
      (e = hipMemsetAsync(d.stream, 0, NN * std::max<uint32_t>(cfg->commit_stream_cap, 1) * 4,
                          s->stream)) != hipSuccess ||
      (e = hipMemsetAsync(d.tr, 0, NN * std::max<uint32_t>(d.TC, 1) * 128, s->stream)) != hipSuccess ||
      (e = hipMemsetAsync(d.tcount, 0, NN * 4, s->stream)) != hipSuccess ||
      (e = hipMemsetAsync(d.tent, 0, NN * std::max<uint32_t>(d.TE, 1) * 8, s->stream)) != hipSuccess ||
      (e = hipMemsetAsync(d.tecount, 0, NN * 4, s->stream)) != hipSuccess ||
      (d.shist && (e = hipMemsetAsync(d.shist, 0, rs::SCHED_BUCKETS * 4, s->stream)) != hipSuccess) ||
      (s->nbail2 && (e = hipMemsetAsync(s->nbail2, 0, 8, s->stream)) != hipSuccess) ||
      (e = init_counters(s)) != hipSuccess ||
      (e = hipMemcpyAsync(s->client_pw, pw, sizeof pw, hipMemcpyHostToDevice, s->stream)) !=
          hipSuccess ||
      (e = rs::launch_init(d, s->stream)) != hipSuccess ||
      (e = rs::launch_viol_clear(d, s->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(s->stream)) != hipSuccess)
    return fail(-EIO, "HIP error during create: %s", hipGetErrorString(e));
  return 0;
}

// One shard: cfg holds its own cluster count, global offset and device (validated by the caller).
static int sh_create(const raft_sim_config_t* cfg, Shard** out) {
  HIP_OK(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, cfg->device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(-EIO, "device is %s; libraftsim.so is built for gfx950", prop.gcnArchName);
  HIP_OK(rs::configure_kernels());
  Shard* s = new Shard();
  const int rc = sh_init(s, cfg);
  if (rc) {
    sh_destroy(s);
    return rc;
  }
  *out = s;
  return 0;
}

// Enqueue n_ticks on the shard's stream, launch by launch as rs::plan_launch says. ls.tick
// advances with every enqueued launch, so after a failure it still names the tick the state has
// reached (the handle is then poisoned anyway).
static int sh_step_async(Shard* s, uint32_t n_ticks) {
  rs::invalidate(s->ls, rs::ON_STEP);
  HIP_OK(hipSetDevice(s->cfg.device));
  if (!s->pending) {
    HIP_OK(hipEventRecord(s->ev_start, s->stream));
    s->pending = true;
  }
  for (uint32_t done = 0; done < n_ticks;) {
    const uint32_t launch = s->ls.window_launch;
    const rs::LaunchPlan p = rs::plan_launch(
        s->lf, s->ls, n_ticks - done,
        s->bail_host ? __atomic_load_n(s->bail_host, __ATOMIC_RELAXED) : 0u);
    if (p.reset_report) __atomic_store_n(s->bail_host, 0u, __ATOMIC_RELAXED);
    if (p.sched != rs::SCHED_NONE) {
      if (p.sched == rs::SCHED_KEY_PERM) {
        HIP_OK(hipMemsetAsync(s->d.shist, 0, rs::SCHED_BUCKETS * 4, s->stream));
        HIP_OK(rs::launch_sched_key(s->d, p.t0, s->stream));
      }
      HIP_OK(rs::launch_sched_perm(s->d, s->soff, s->sperm, s->snslots, s->stream));
      // the schedule kernel read d.shist and zeroed soff: the next key-writing launch fills it
      std::swap(s->d.shist, s->soff);
      s->d.perm = s->sperm;
      s->d.nslots = s->snslots;
    }
    if (s->ktimed.size() < launch + 1) s->ktimed.resize(launch + 1);
    s->ktimed[launch] = p.timed;
    while (p.timed && s->kev.size() < 2 * (size_t)(launch + 1)) {
      hipEvent_t e;   // timing only: no system-scope fence (cache writeback) per launch
      HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
      s->kev.push_back(e);
    }
#ifdef RS_WAVELOG
    HIP_OK(hipMemsetAsync(s->d.wavelog, 0,
                          (size_t)rs::sched_slots_bound(s->C, s->N) * 192 / (64 / s->N), s->stream));
#endif
    if (p.path == rs::PATH_STEADY) {
      s->d.nbail = s->nbail2 + p.bail_parity;
      s->d.nbail_zero = s->nbail2 + (p.bail_parity ^ 1);
    }
    DevSim D = s->d;
    if (!p.use_perm) D.perm = nullptr;
    if (!p.write_keys) D.shist = nullptr;
    HIP_OK(rs::launch_tick(D, p.path, p.t0, p.nt, s->stream,
                           p.timed ? s->kev[2 * launch] : nullptr,
                           p.timed ? s->kev[2 * launch + 1] : nullptr));
    rs::launch_enqueued(s->ls, p);
    done += p.nt;
  }
  return 0;
}

static int sh_sync(Shard* s) {
  if (!s) return fail(-EINVAL, "null sim");
  HIP_OK(hipSetDevice(s->cfg.device));
  if (!s->pending) {
    HIP_OK(hipStreamSynchronize(s->stream));
    return 0;
  }
  const uint32_t launches = s->ls.window_launch;
  s->pending = false;
  rs::synced(s->ls);
  HIP_OK(hipEventRecord(s->ev_stop, s->stream));
  HIP_OK(hipEventSynchronize(s->ev_stop));
  float ms = 0, kms = 0;
  HIP_OK(hipEventElapsedTime(&ms, s->ev_start, s->ev_stop));
  uint32_t timed = 0;
  for (uint32_t i = 0; i < launches; ++i) {
    if (!s->ktimed[i]) continue;
    float one = 0;
    HIP_OK(hipEventElapsedTime(&one, s->kev[2 * i], s->kev[2 * i + 1]));
    kms += one;
    ++timed;
  }
  s->last_ms = timed ? kms / timed : 0.0;         // per timed tick-kernel launch
  s->last_timed = timed;
  s->last_step_ms = ms;                           // + the schedule's key and sort kernels
  s->last_launches = launches;
  return 0;
}


static int check_range(Shard* s, uint32_t c0, uint32_t nc) {
  if (!s) return fail(-EINVAL, "null sim");
  if ((uint64_t)c0 + nc > s->C) return fail(-EINVAL, "cluster range out of bounds");
  return 0;
}

// Slot 0 of node gi's queue `which` and the ring's slot pitch in bytes (rs::qslots: REQ rings
// slot-major, RES rings node-major).
static uint32_t* qring(Shard* s, uint32_t gi, uint32_t which) {
  return s->d.qbuf + (which ? (size_t)s->Q * s->NN + (size_t)gi * s->Q : (size_t)gi) * 8;
}
static size_t qpitch(Shard* s, uint32_t which) {
  return (which ? 1 : (size_t)s->NN) * sizeof(raft_msg_t);
}

// Field `f` of node `id` in cluster `cluster`'s hot block (rs::HotField).
static uint32_t* hot_word(Shard* s, uint32_t cluster, uint32_t id, uint32_t f) {
  return s->d.hot + (size_t)cluster * s->d.HB + rs::HOT_CW + (size_t)f * s->N + (id - 1);
}
static uint32_t* cl_words(Shard* s, uint32_t cluster) {
  return s->d.hot + (size_t)cluster * s->d.HB;
}

static int check_node(Shard* s, uint32_t cluster, uint32_t id) {
  if (!s) return fail(-EINVAL, "null sim");
  if (cluster >= s->C || id < 1 || id > s->N) return fail(-EINVAL, "cluster/node out of bounds");
  return 0;
}

template <typename T>
static hipError_t d2h(Shard* s, T* host, const T* dev, size_t count) {
  return hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, s->stream);
}
template <typename T>
static hipError_t h2d(Shard* s, T* dev, const T* host, size_t count) {
  return hipMemcpyAsync(dev, host, count * sizeof(T), hipMemcpyHostToDevice, s->stream);
}

static int sh_read_nodes(Shard* s, uint32_t c0, uint32_t nc, raft_node_t* out) {
  int rc = check_range(s, c0, nc);
  if (rc) return rc;
  if (!out) return fail(-EINVAL, "null output");
  HIP_OK(hipSetDevice(s->cfg.device));
  const size_t n0 = (size_t)c0 * s->N, cnt = (size_t)nc * s->N, N = s->N, HB = s->d.HB;
  std::vector<uint32_t> blk(nc * HB), cc(cnt);
  HIP_OK(d2h(s, blk.data(), s->d.hot + (size_t)c0 * HB, nc * HB));
  HIP_OK(d2h(s, cc.data(), s->d.ccount + n0, cnt));
  HIP_OK(hipStreamSynchronize(s->stream));
  const rs::DrawKeys dk = {s->cfg.el_base, s->cfg.el_span, s->d.key0, s->d.key1};
  for (size_t i = 0; i < cnt; ++i) {
    const uint32_t k = (uint32_t)(i % N), g = (uint32_t)(s->cfg.cluster_offset + c0 + i / N);
    uint32_t nw[rs::NODE_WORDS];
    for (uint32_t w = 0; w < rs::NODE_WORDS; ++w)
      nw[w] = rs::node_word(&blk[(i / N) * HB + rs::HOT_CW + k], (uint32_t)N, w, cc[i], g, k, dk);
    memcpy(&out[i], nw, sizeof nw);
  }
  return 0;
}

static int sh_write_nodes(Shard* s, uint32_t c0, uint32_t nc, const raft_node_t* in) {
  int rc = check_range(s, c0, nc);
  if (rc) return rc;
  rs::invalidate(s->ls, rs::ON_WRITE_NODES);
  if (!in) return fail(-EINVAL, "null input");
  HIP_OK(hipSetDevice(s->cfg.device));
  const uint32_t N = s->N;
  const size_t n0 = (size_t)c0 * N, cnt = (size_t)nc * N;
  for (size_t i = 0; i < cnt; ++i)
    if (!rs::node_record_ok(in[i], (uint32_t)(i % N) + 1, N, s->L))
      return fail(-EINVAL, "invalid node record");
  // the queue words of the blocks (qmeta, head/tail arrivals) and the cluster words are kept
  const size_t HB = s->d.HB;
  std::vector<uint32_t> blk(nc * HB), ccv(cnt);
  HIP_OK(d2h(s, blk.data(), s->d.hot + (size_t)c0 * HB, nc * HB));
  HIP_OK(hipStreamSynchronize(s->stream));
  for (size_t i = 0; i < cnt; ++i) {
    uint32_t nw[rs::NODE_WORDS];
    memcpy(nw, &in[i], sizeof nw);
    uint32_t* h = &blk[(i / N) * HB + rs::HOT_CW + i % N];           // field f at h[f * N]
    for (uint32_t f = 0; f < rs::hot_fields(N); ++f)
      if (!rs::hf_is_queue(f)) h[f * N] = rs::hot_field(nw, N, f);
    ccv[i] = in[i].commit_count;
  }
  for (size_t c = 0; c < nc; ++c) blk[c * HB + rs::CL_CERT] = 0;   // the steady certificate
  HIP_OK(h2d(s, s->d.hot + (size_t)c0 * HB, blk.data(), nc * HB));
  HIP_OK(h2d(s, s->d.ccount + n0, ccv.data(), cnt));
  HIP_OK(hipStreamSynchronize(s->stream));
  return 0;
}

static int sh_read_queue(Shard* s, uint32_t cluster, uint32_t id, uint32_t which,
                        raft_msg_t* out, uint32_t cap) {
  int rc = check_node(s, cluster, id);
  if (rc) return rc;
  if (which > 1) return fail(-EINVAL, "which must be 0 (req) or 1 (res)");
  HIP_OK(hipSetDevice(s->cfg.device));
  const uint32_t gi = cluster * s->N + id - 1;
  uint32_t qm = 0;
  std::vector<raft_msg_t> slots(s->Q);
  HIP_OK(d2h(s, &qm, hot_word(s, cluster, id, rs::HF_QMETA), 1));
  HIP_OK(hipMemcpy2DAsync(slots.data(), sizeof(raft_msg_t), qring(s, gi, which),
                          qpitch(s, which), sizeof(raft_msg_t), s->Q,
                          hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  const uint32_t head = which ? rs::qm_res_head(qm) : rs::qm_req_head(qm);
  const uint32_t cnt = which ? rs::qm_res_cnt(qm) : rs::qm_req_cnt(qm);
  for (uint32_t i = 0; i < cnt && i < cap && out; ++i) out[i] = slots[(head + i) % s->Q];
  return (int)cnt;
}

static int sh_write_queue(Shard* s, uint32_t cluster, uint32_t id, uint32_t which,
                         const raft_msg_t* in, uint32_t count) {
  int rc = check_node(s, cluster, id);
  if (rc) return rc;
  rs::invalidate(s->ls, rs::ON_WRITE_QUEUE);
  switch (rs::queue_fault(in, count, which, id, s->N, s->Q)) {
    case rs::QUEUE_OK: break;
    case rs::QUEUE_COUNT: return fail(-EINVAL, "bad queue or count");
    default: return fail(-EINVAL, "invalid message or order");
  }
  if (rs::queue_has_client_set(in, count)) rs::invalidate(s->ls, rs::ON_QUEUED_CLIENT_SET);
  HIP_OK(hipSetDevice(s->cfg.device));
  const uint32_t gi = cluster * s->N + id - 1;
  std::vector<raft_msg_t> slots(s->Q);
  memset(slots.data(), 0, s->Q * sizeof(raft_msg_t));
  for (uint32_t i = 0; i < count; ++i) slots[i] = in[i];
  uint32_t qm = 0;
  HIP_OK(d2h(s, &qm, hot_word(s, cluster, id, rs::HF_QMETA), 1));
  HIP_OK(hipStreamSynchronize(s->stream));
  const rs::RingWords ring = rs::ring_words(which, count, reinterpret_cast<const uint32_t*>(in));
  qm = rs::with_ring(qm, ring);                                   // the other ring's half stays
  HIP_OK(hipMemcpy2DAsync(qring(s, gi, which), qpitch(s, which), slots.data(),
                          sizeof(raft_msg_t), sizeof(raft_msg_t), s->Q, hipMemcpyHostToDevice,
                          s->stream));
  HIP_OK(h2d(s, hot_word(s, cluster, id, rs::HF_QMETA), &qm, 1));
  const uint32_t farr = which ? rs::HF_RES_ARR : rs::HF_REQ_ARR;
  const uint32_t ftail = which ? rs::HF_RES_TAIL : rs::HF_REQ_TAIL;
  HIP_OK(h2d(s, hot_word(s, cluster, id, farr), &ring.arr, 1));
  HIP_OK(h2d(s, hot_word(s, cluster, id, ftail), &ring.tail, 1));
  const uint32_t zero = 0;                                        // the steady certificate
  HIP_OK(h2d(s, cl_words(s, cluster) + rs::CL_CERT, &zero, 1));
  HIP_OK(hipStreamSynchronize(s->stream));
  return 0;
}

static int sh_read_arena(Shard* s, uint32_t cluster, uint32_t id, raft_entry_t* out,
                        uint32_t cap) {
  int rc = check_node(s, cluster, id);
  if (rc) return rc;
  if (out && cap) {
    HIP_OK(hipSetDevice(s->cfg.device));
    const size_t gi = (size_t)cluster * s->N + id - 1;
    HIP_OK(hipMemcpyAsync(out, s->d.arena + gi * s->A * 2,
                          std::min(cap, s->A) * sizeof(raft_entry_t), hipMemcpyDeviceToHost,
                          s->stream));
    HIP_OK(hipStreamSynchronize(s->stream));
  }
  return (int)s->A;
}

static int sh_write_arena(Shard* s, uint32_t cluster, uint32_t id, const raft_entry_t* in,
                         uint32_t count) {
  int rc = check_node(s, cluster, id);
  if (rc) return rc;
  rs::invalidate(s->ls, rs::ON_WRITE_ARENA);
  if (count > s->A || (count && !in)) return fail(-EINVAL, "count > arena_cap");
  HIP_OK(hipSetDevice(s->cfg.device));
  std::vector<raft_entry_t> buf(s->A);
  memset(buf.data(), 0, s->A * sizeof(raft_entry_t));
  if (count) memcpy(buf.data(), in, count * sizeof(raft_entry_t));
  const size_t gi = (size_t)cluster * s->N + id - 1;
  HIP_OK(hipMemcpyAsync(s->d.arena + gi * s->A * 2, buf.data(), s->A * sizeof(raft_entry_t),
                        hipMemcpyHostToDevice, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  return 0;
}

static int sh_read_commit_stream(Shard* s, uint32_t cluster, uint32_t id, uint32_t* out,
                                uint32_t cap) {
  int rc = check_node(s, cluster, id);
  if (rc) return rc;
  HIP_OK(hipSetDevice(s->cfg.device));
  const uint32_t SC = s->cfg.commit_stream_cap;
  const size_t gi = (size_t)cluster * s->N + id - 1;
  uint32_t cc = 0;
  std::vector<uint32_t> ring(std::max<uint32_t>(SC, 1));
  HIP_OK(d2h(s, &cc, s->d.ccount + gi, 1));
  if (SC) HIP_OK(d2h(s, ring.data(), s->d.stream + gi * SC, SC));
  HIP_OK(hipStreamSynchronize(s->stream));
  uint32_t kept = std::min(std::min(cc, SC), cap);
  for (uint32_t i = 0; i < kept && out; ++i) out[i] = ring[(cc - kept + i) % SC];
  return (int)kept;
}

static int sh_write_commit_stream(Shard* s, uint32_t cluster, uint32_t id, const uint32_t* in,
                                 uint32_t count) {
  int rc = check_node(s, cluster, id);
  if (rc) return rc;
  rs::invalidate(s->ls, rs::ON_WRITE_COMMIT_STREAM);
  HIP_OK(hipSetDevice(s->cfg.device));
  const uint32_t SC = s->cfg.commit_stream_cap;
  const size_t gi = (size_t)cluster * s->N + id - 1;
  uint32_t cc = 0;
  HIP_OK(d2h(s, &cc, s->d.ccount + gi, 1));
  HIP_OK(hipStreamSynchronize(s->stream));
  if (count > SC || count > cc || (count && !in))
    return fail(-EINVAL, "count exceeds ring or commit_count");
  if (!count) return 0;
  std::vector<uint32_t> ring(SC);
  HIP_OK(d2h(s, ring.data(), s->d.stream + gi * SC, SC));
  HIP_OK(hipStreamSynchronize(s->stream));
  for (uint32_t i = 0; i < count; ++i) ring[(cc - count + i) % SC] = in[i];
  HIP_OK(h2d(s, s->d.stream + gi * SC, ring.data(), SC));
  HIP_OK(hipStreamSynchronize(s->stream));
  return 0;
}

// F3 rings: copy the retained items with index >= first (oldest first), at most cap of them;
// `strict` rejects a `first` that has been overwritten instead of starting at the oldest kept.
template <typename T>
static int read_ring(Shard* s, const uint32_t* dcount, const T* dring, uint32_t R, uint32_t gi,
                     uint32_t first, T* out, uint32_t cap, bool strict) {
  uint32_t cnt = 0;
  HIP_OK(d2h(s, &cnt, dcount + gi, 1));
  HIP_OK(hipStreamSynchronize(s->stream));
  uint32_t lo = cnt > R ? cnt - R : 0;
  if (strict && first < lo) return fail(-ERANGE, "trace entries overwritten (ring holds the newest)");
  if (first > lo) lo = first;
  const uint32_t n = lo < cnt ? std::min(cnt - lo, cap) : 0;
  if (n && !out) return fail(-EINVAL, "null output");
  // at most two contiguous pieces of the ring
  for (uint32_t done = 0; done < n;) {
    const uint32_t slot = (lo + done) % R, run = std::min(n - done, R - slot);
    HIP_OK(d2h(s, out + done, dring + (size_t)gi * R + slot, run));
    done += run;
  }
  HIP_OK(hipStreamSynchronize(s->stream));
  return (int)n;
}

static int sh_read_trace(Shard* s, uint32_t cluster, uint32_t id, uint32_t first,
                        raft_trace_event_t* out, uint32_t cap) {
  static_assert(sizeof(raft_trace_event_t) == 128, "trace record is 32 words");
  int rc = check_node(s, cluster, id);
  if (rc) return rc;
  HIP_OK(hipSetDevice(s->cfg.device));
  if (!s->d.TC) return 0;
  return read_ring(s, s->d.tcount, reinterpret_cast<const raft_trace_event_t*>(s->d.tr),
                   s->d.TC, cluster * s->N + id - 1, first, out, cap, false);
}

static int sh_read_trace_entries(Shard* s, uint32_t cluster, uint32_t id, uint32_t first,
                                raft_entry_t* out, uint32_t cap) {
  int rc = check_node(s, cluster, id);
  if (rc) return rc;
  HIP_OK(hipSetDevice(s->cfg.device));
  if (!s->d.TE) return fail(-ERANGE, "trace_entry_cap is 0");
  return read_ring(s, s->d.tecount, reinterpret_cast<const raft_entry_t*>(s->d.tent), s->d.TE,
                   cluster * s->N + id - 1, first, out, cap, true);
}

static int sh_read_clusters(Shard* s, uint32_t c0, uint32_t nc, raft_cluster_t* out) {
  int rc = check_range(s, c0, nc);
  if (rc) return rc;
  HIP_OK(hipSetDevice(s->cfg.device));
  static_assert(sizeof(raft_cluster_t) == 32, "cluster record is 8 words");
  if (nc)    // the cluster words sit at a fixed offset of each block
    HIP_OK(hipMemcpy2DAsync(out, sizeof(raft_cluster_t), cl_words(s, c0), (size_t)s->d.HB * 4,
                            sizeof(raft_cluster_t), nc, hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  // the reserved words are the kernels' (the steady certificate, rs::CL_CERT): not state
  for (uint32_t i = 0; i < nc; ++i) out[i].reserved[0] = out[i].reserved[1] = out[i].reserved[2] = 0;
  return 0;
}

static int sh_write_clusters(Shard* s, uint32_t c0, uint32_t nc, const raft_cluster_t* in) {
  int rc = check_range(s, c0, nc);
  if (rc) return rc;
  rs::invalidate(s->ls, rs::ON_WRITE_CLUSTERS);
  HIP_OK(hipSetDevice(s->cfg.device));
  std::vector<raft_cluster_t> buf(in, in + nc);
  for (auto& h : buf) {
    h.reserved[0] = h.reserved[1] = h.reserved[2] = 0;
    if (h.client_next != 0xFFFFFFFFu) rs::invalidate(s->ls, rs::ON_CLIENT_CURSOR);
  }
  if (nc)
    HIP_OK(hipMemcpy2DAsync(cl_words(s, c0), (size_t)s->d.HB * 4, buf.data(),
                            sizeof(raft_cluster_t), sizeof(raft_cluster_t), nc,
                            hipMemcpyHostToDevice, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  return 0;
}

static int sh_read_counters(Shard* s, raft_counters_t* out) {
  if (!s || !out) return fail(-EINVAL, "null argument");
  HIP_OK(hipSetDevice(s->cfg.device));
  std::vector<unsigned long long> buf((size_t)rs::CTR_COPIES * rs::CTR_STRIDE);
  HIP_OK(hipMemcpyAsync(buf.data(), s->d.ctr, buf.size() * 8, hipMemcpyDeviceToHost, s->stream));
  HIP_OK(hipStreamSynchronize(s->stream));
  memset(out->c, 0, sizeof out->c);
  out->first_violation_tick = ~0ull;
  out->payload_max = 0;
  for (int k = 0; k < rs::CTR_COPIES; ++k) {        // the copies the waves flushed into
    const unsigned long long* b = &buf[(size_t)k * rs::CTR_STRIDE];
    for (int i = 0; i < RAFT_CTR_COUNT; ++i) out->c[i] += b[i];
    out->first_violation_tick = std::min<uint64_t>(out->first_violation_tick, b[RAFT_CTR_COUNT]);
    out->payload_max = std::max<uint64_t>(out->payload_max, b[RAFT_CTR_COUNT + 1]);
  }
  out->node_ticks = (uint64_t)s->NN * s->ls.ticks_run;
  return 0;
}

static int sh_digest(Shard* s, uint32_t c0, uint32_t nc, uint64_t* out) {
  int rc = check_range(s, c0, nc);
  if (rc) return rc;
  if (!out) return fail(-EINVAL, "null output");
  HIP_OK(hipSetDevice(s->cfg.device));
  unsigned long long* dout = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&dout), std::max<size_t>(nc, 1) * 8));
  hipError_t e = rs::launch_digest(s->d, c0, nc, dout, s->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(out, dout, (size_t)nc * 8, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  (void)hipFree(dout);
  if (e != hipSuccess) return fail(-EIO, "HIP error in digest: %s", hipGetErrorString(e));
  return 0;
}


// ---------------------------------------------------------------------------------------------
// The handle: n_devices shards, each a contiguous cluster range [C*d/G, C*(d+1)/G) on device
// (device + d) mod the visible devices, with its own stream. The global cluster id keys Philox
// (SIM_SPEC D13), so every G gives bit-identical clusters; calls addressed to clusters are routed
// to their shard and counters are reduced on the host (SUM; MIN first violation; MAX payload).
// Across processes (torchrun, one rank per GPU) bench.py reduces the same vector over RCCL.
struct raft_sim {
  raft_sim_config_t cfg;
  std::vector<Shard*> sh;
  std::vector<uint32_t> lo;   // shard d owns clusters [lo[d], lo[d+1])
  uint64_t tick;
  bool poisoned;              // a step failed part-way: the state no longer matches `tick`
};

void raft_sim_destroy(raft_sim_t* r) {
  if (!r) return;
  for (Shard* s : r->sh) sh_destroy(s);
  delete r;
}

int raft_sim_create(const raft_sim_config_t* cfg, raft_sim_t** out) {
  if (!cfg || !out) return fail(-EINVAL, "null argument");
  int rc = validate_cfg(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(-EIO, "no HIP device visible: libraftsim.so requires an MI355X (gfx950)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(-EINVAL, "device ordinal out of range");
  const uint32_t G = std::min<uint32_t>(cfg->n_devices > 1 ? cfg->n_devices : 1, cfg->n_clusters);
  for (uint32_t d = 0; d < G; ++d) {
    const int dev = (cfg->device + (int)d) % ndev;
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return fail(-EIO, "device is %s; libraftsim.so is built for gfx950", prop.gcnArchName);
    HIP_OK(hipSetDevice(dev));
    HIP_OK(rs::configure_kernels());
  }
  raft_sim* r = new raft_sim();
  r->cfg = *cfg;
  for (uint32_t d = 0; d <= G; ++d) r->lo.push_back((uint32_t)((uint64_t)cfg->n_clusters * d / G));
  for (uint32_t d = 0; d < G; ++d) {
    raft_sim_config_t c = *cfg;
    c.n_clusters = r->lo[d + 1] - r->lo[d];
    c.cluster_offset = cfg->cluster_offset + r->lo[d];
    c.device = (cfg->device + (int)d) % ndev;
    c.n_devices = 1;
    Shard* s = nullptr;
    if ((rc = sh_create(&c, &s))) {
      raft_sim_destroy(r);
      return rc;
    }
    r->sh.push_back(s);
  }
  *out = r;
  return 0;
}

// SIM_SPEC D1: no deadline or arrival may reach 2^32 - 1, the "never" marker.
static bool horizon_ok(const raft_sim_config_t& c, uint64_t tick, uint32_t n) {
  const uint64_t longest = std::max<uint64_t>({c.hb, (uint64_t)c.el_base + c.el_span, c.dmax});
  return tick + n + longest < 0xFFFFFFFFull;
}

int raft_sim_step_async(raft_sim_t* r, uint32_t n_ticks) {
  if (!r) return fail(-EINVAL, "null sim");
  if (r->poisoned) return unusable();
  if (!horizon_ok(r->cfg, r->tick, n_ticks))
    return fail(-ERANGE, "tick + n_ticks + the longest timer would reach 2^32-1");
  for (Shard* s : r->sh) {
    const int rc = sh_step_async(s, n_ticks);
    if (rc) {
      r->poisoned = true;
      return rc;
    }
  }
  r->tick += n_ticks;
  return 0;
}

int raft_sim_sync(raft_sim_t* r) {
  if (!r) return fail(-EINVAL, "null sim");
  for (Shard* s : r->sh) {
    const int rc = sh_sync(s);
    if (rc) {
      r->poisoned = true;
      return rc;
    }
  }
  return 0;
}

int raft_sim_step(raft_sim_t* r, uint32_t n_ticks) {
  const int rc = raft_sim_step_async(r, n_ticks);
  return rc ? rc : raft_sim_sync(r);
}

uint64_t raft_sim_tick(const raft_sim_t* r) { return r ? r->tick : 0; }

int raft_sim_set_tick(raft_sim_t* r, uint64_t tick) {
  if (!r) return fail(-EINVAL, "null sim");
  if (!horizon_ok(r->cfg, tick, 0)) return fail(-ERANGE, "tick beyond the 32-bit horizon");
  for (Shard* s : r->sh) {
    const int rc = sh_sync(s);
    if (rc) return rc;
    rs::set_tick(s->ls, tick);
  }
  r->tick = tick;
  return 0;
}

int raft_sim_last_step_timing(raft_sim_t* r, double* avg_kernel_ms, uint32_t* launches) {
  if (!r || !avg_kernel_ms || !launches) return fail(-EINVAL, "null argument");
  double sum = 0;
  uint32_t n = 0;
  for (Shard* s : r->sh) {
    sum += s->last_ms * s->last_launches;
    n += s->last_launches;
  }
  *avg_kernel_ms = n ? sum / n : 0.0;
  *launches = r->sh.empty() ? 0 : r->sh[0]->last_launches;
  return 0;
}

int raft_sim_last_span(raft_sim_t* r, double* span_ms) {
  if (!r || !span_ms) return fail(-EINVAL, "null argument");
  double m = 0;
  for (Shard* s : r->sh) m = std::max(m, s->last_step_ms);
  *span_ms = m;
  return 0;
}

// The index of the shard owning cluster c; the shard, and c's index inside it.
static size_t owner_index(const raft_sim* r, uint32_t c) {
  return std::upper_bound(r->lo.begin() + 1, r->lo.end() - 1, c) - (r->lo.begin() + 1);
}
static Shard* owner(raft_sim* r, uint32_t c, uint32_t* lc) {
  const size_t d = owner_index(r, c);
  *lc = c - r->lo[d];
  return r->sh[d];
}

// Run `fn(shard, local c0, count, offset into the caller's range)` over the per-shard pieces.
template <typename F>
static int pieces(raft_sim* r, uint32_t c0, uint32_t nc, F fn) {
  if (!r) return fail(-EINVAL, "null sim");
  if ((uint64_t)c0 + nc > r->cfg.n_clusters) return fail(-EINVAL, "cluster range out of bounds");
  for (uint32_t done = 0; done < nc;) {
    uint32_t lc;
    Shard* s = owner(r, c0 + done, &lc);
    const uint32_t n = std::min(s->C - lc, nc - done);
    const int rc = fn(s, lc, n, (size_t)done);
    if (rc) return rc;
    done += n;
  }
  return 0;
}

int raft_sim_read_nodes(raft_sim_t* r, uint32_t c0, uint32_t nc, raft_node_t* out) {
  if (!out) return fail(-EINVAL, "null output");
  return pieces(r, c0, nc, [&](Shard* s, uint32_t lc, uint32_t n, size_t off) {
    return sh_read_nodes(s, lc, n, out + off * r->cfg.nodes);
  });
}
int raft_sim_write_nodes(raft_sim_t* r, uint32_t c0, uint32_t nc, const raft_node_t* in) {
  if (!in) return fail(-EINVAL, "null input");
  return pieces(r, c0, nc, [&](Shard* s, uint32_t lc, uint32_t n, size_t off) {
    return sh_write_nodes(s, lc, n, in + off * r->cfg.nodes);
  });
}
int raft_sim_read_clusters(raft_sim_t* r, uint32_t c0, uint32_t nc, raft_cluster_t* out) {
  if (!out) return fail(-EINVAL, "null output");
  return pieces(r, c0, nc, [&](Shard* s, uint32_t lc, uint32_t n, size_t off) {
    return sh_read_clusters(s, lc, n, out + off);
  });
}
int raft_sim_write_clusters(raft_sim_t* r, uint32_t c0, uint32_t nc, const raft_cluster_t* in) {
  if (!in) return fail(-EINVAL, "null input");
  return pieces(r, c0, nc, [&](Shard* s, uint32_t lc, uint32_t n, size_t off) {
    return sh_write_clusters(s, lc, n, in + off);
  });
}
int raft_sim_digest(raft_sim_t* r, uint32_t c0, uint32_t nc, uint64_t* out) {
  if (!out) return fail(-EINVAL, "null output");
  return pieces(r, c0, nc, [&](Shard* s, uint32_t lc, uint32_t n, size_t off) {
    return sh_digest(s, lc, n, out + off);
  });
}

#define ROUTE_NODE(call)                                                                  \
  if (!r || cluster >= r->cfg.n_clusters) return fail(-EINVAL, "cluster/node out of bounds"); \
  uint32_t lc;                                                                            \
  Shard* s = owner(r, cluster, &lc);                                                      \
  return call;

int raft_sim_read_queue(raft_sim_t* r, uint32_t cluster, uint32_t id, uint32_t which,
                        raft_msg_t* out, uint32_t cap) {
  ROUTE_NODE(sh_read_queue(s, lc, id, which, out, cap))
}
int raft_sim_write_queue(raft_sim_t* r, uint32_t cluster, uint32_t id, uint32_t which,
                         const raft_msg_t* in, uint32_t count) {
  ROUTE_NODE(sh_write_queue(s, lc, id, which, in, count))
}
int raft_sim_read_arena(raft_sim_t* r, uint32_t cluster, uint32_t id, raft_entry_t* out,
                        uint32_t cap) {
  ROUTE_NODE(sh_read_arena(s, lc, id, out, cap))
}
int raft_sim_write_arena(raft_sim_t* r, uint32_t cluster, uint32_t id, const raft_entry_t* in,
                         uint32_t count) {
  ROUTE_NODE(sh_write_arena(s, lc, id, in, count))
}
int raft_sim_read_commit_stream(raft_sim_t* r, uint32_t cluster, uint32_t id, uint32_t* out,
                                uint32_t cap) {
  ROUTE_NODE(sh_read_commit_stream(s, lc, id, out, cap))
}
int raft_sim_write_commit_stream(raft_sim_t* r, uint32_t cluster, uint32_t id, const uint32_t* in,
                                 uint32_t count) {
  ROUTE_NODE(sh_write_commit_stream(s, lc, id, in, count))
}
int raft_sim_read_trace(raft_sim_t* r, uint32_t cluster, uint32_t id, uint32_t first,
                        raft_trace_event_t* out, uint32_t cap) {
  ROUTE_NODE(sh_read_trace(s, lc, id, first, out, cap))
}
int raft_sim_read_trace_entries(raft_sim_t* r, uint32_t cluster, uint32_t id, uint32_t first,
                                raft_entry_t* out, uint32_t cap) {
  ROUTE_NODE(sh_read_trace_entries(s, lc, id, first, out, cap))
}

int raft_sim_read_counters(raft_sim_t* r, raft_counters_t* out) {
  if (!r || !out) return fail(-EINVAL, "null argument");
  memset(out, 0, sizeof *out);
  out->first_violation_tick = UINT64_MAX;
  for (Shard* s : r->sh) {
    raft_counters_t c;
    const int rc = sh_read_counters(s, &c);
    if (rc) return rc;
    out->node_ticks += c.node_ticks;
    for (int i = 0; i < RAFT_CTR_COUNT; ++i) out->c[i] += c.c[i];
    out->first_violation_tick = std::min(out->first_violation_tick, c.first_violation_tick);
    out->payload_max = std::max(out->payload_max, c.payload_max);
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// The sharded query path of raft_viol_read and raft_census_select: a compaction (compact.hpp) runs
// on every shard's stream at once, behind whatever the shard has enqueued; shards are contiguous
// cluster ranges, so their results concatenated in shard order are sorted, and a record's cluster
// is rebased from the shard to the handle. Returns the handle's total, with the first `cap`
// records in out.
//   name      the calling function, for error messages
//   prepare   (Shard*) -> int: what the shard needs before its first query; may fail
//   enqueue   (Shard*, Rec* dout, uint32_t dcap, const uint32_t** dtotal) -> hipError_t: launch the
//             query into the device buffer dout of dcap records; *dtotal: where its total will stand
//   ms        the shard's field for the device time of the query's kernels
template <class Rec, class Prepare, class Enqueue>
static int64_t sharded_query(raft_sim_t* r, uint32_t cap, Rec* out, const char* name,
                             Prepare prepare, Enqueue enqueue, double Shard::*ms) {
  const size_t G = r->sh.size();
  // shard d can contribute min(cap, its clusters) records at most; freed on every path below
  std::vector<Rec*> dout(G, nullptr);
  std::vector<uint32_t> dcap(G, 0), total(G, 0);
  char herr[64], merr[64];
  snprintf(herr, sizeof herr, "HIP error in %s: %%s", name);
  snprintf(merr, sizeof merr, "hipMalloc failed in %s: %%s", name);
  int rc = 0;
  auto step = [&](hipError_t e, const char* what) {
    if (!rc && e != hipSuccess) rc = fail(-EIO, what, hipGetErrorString(e));
    return !rc;
  };
  for (size_t d = 0; d < G && !rc; ++d) {
    Shard* s = r->sh[d];
    dcap[d] = std::min(cap, s->C);
    if (!step(hipSetDevice(s->cfg.device), herr) || (rc = prepare(s))) break;
    if (dcap[d] && !step(hipMalloc(reinterpret_cast<void**>(&dout[d]), (size_t)dcap[d] * sizeof(Rec)),
                         merr))
      break;
    const uint32_t* dtotal = nullptr;
    if (step(hipEventRecord(s->qev0, s->stream), herr) &&
        step(enqueue(s, dout[d], dcap[d], &dtotal), herr) &&
        step(hipEventRecord(s->qev1, s->stream), herr))
      step(d2h(s, &total[d], dtotal, 1), herr);
  }
  int64_t sum = 0;
  for (size_t d = 0; d < G && !rc; ++d) {
    Shard* s = r->sh[d];
    if (!step(hipSetDevice(s->cfg.device), herr) || !step(hipStreamSynchronize(s->stream), herr))
      break;
    float t = 0;
    if (!step(hipEventElapsedTime(&t, s->qev0, s->qev1), herr)) break;
    s->*ms = t;
    // the handle's first `cap` matches: what is left of cap after the shards before this one
    const uint32_t left = (uint64_t)sum < cap ? cap - (uint32_t)sum : 0u;
    const uint32_t n = std::min(std::min(total[d], dcap[d]), left);
    if (n) {
      Rec* dst = out + sum;
      if (!step(hipMemcpy(dst, dout[d], (size_t)n * sizeof(Rec), hipMemcpyDeviceToHost), herr))
        break;
      for (uint32_t i = 0; i < n; ++i) dst[i].cluster += r->lo[d];
    }
    sum += total[d];
  }
  for (size_t d = 0; d < G; ++d) {
    if (!rc && !dout[d]) continue;
    (void)hipSetDevice(r->sh[d]->cfg.device);
    // after an error a shard's kernels may still write dout[d] and its copy total[d]
    if (rc) (void)hipStreamSynchronize(r->sh[d]->stream);
    if (dout[d]) (void)hipFree(dout[d]);
  }
  return rc ? rc : sum;
}

// The sharded summary path of raft_census_read and raft_audit_read: every shard leaves its folded
// T (summary.hpp) in its scratch, the host folds them in shard order. Every started shard is
// waited for, also after an error (its copy writes part[d]); the first error wins; a shard's time
// is recorded only on success.
//   name, prepare, ms   as sharded_query's
//   enqueue   (Shard*) -> hipError_t: launch the query on the shard's stream
//   result    (Shard*) -> const unsigned long long*: where the shard's folded T will stand
//   failed    (Shard*): called after the wait for a shard when the call has failed by then
template <class T, class Prepare, class Enqueue, class Result, class Failed>
static int sharded_summary(raft_sim_t* r, T* out, const char* name, Prepare prepare,
                           Enqueue enqueue, Result result, double Shard::*ms, Failed failed) {
  const size_t G = r->sh.size();
  std::vector<T> part(G);
  char herr[64];
  snprintf(herr, sizeof herr, "HIP error in %s: %%s", name);
  int rc = 0;
  auto step = [&](hipError_t e) {
    if (!rc && e != hipSuccess) rc = fail(-EIO, herr, hipGetErrorString(e));
    return !rc;
  };
  size_t started = 0;
  for (size_t d = 0; d < G && !rc; ++d) {
    Shard* s = r->sh[d];
    if (!step(hipSetDevice(s->cfg.device)) || (rc = prepare(s))) break;
    ++started;
    step(hipEventRecord(s->qev0, s->stream)) && step(enqueue(s)) &&
        step(hipEventRecord(s->qev1, s->stream)) &&
        step(d2h(s, reinterpret_cast<unsigned long long*>(&part[d]), result(s), sizeof(T) / 8));
  }
  rs::summary_init(out);
  for (size_t d = 0; d < started; ++d) {
    Shard* s = r->sh[d];
    float t = 0;
    step(hipSetDevice(s->cfg.device));
    step(hipStreamSynchronize(s->stream));
    if (rc) failed(s);
    if (rc || !step(hipEventElapsedTime(&t, s->qev0, s->qev1))) continue;
    s->*ms = t;
    rs::summary_combine(out, &part[d]);
  }
  return rc;
}

// The body of the raftsim_diag_*_ms exports: the maximum over shards of a query's device time.
static int diag_ms(raft_sim_t* r, double* ms, double Shard::*field) {
  if (!r || !ms) return fail(-EINVAL, "null argument");
  double m = 0;
  for (Shard* s : r->sh) m = std::max(m, s->*field);
  *ms = m;
  return 0;
}

// Violation records (include/raftsim.h, "no reference counterpart").
int64_t raft_viol_read(raft_sim_t* r, uint32_t kinds_mask, uint64_t t_lo, uint64_t t_hi,
                       raft_violation_t* out, uint32_t cap) {
  if (!r) return fail(-EINVAL, "null sim");
  if (r->poisoned) return unusable();
  if (kinds_mask == 0 || kinds_mask > 7) return fail(-EINVAL, "kinds_mask must be 1..7");
  if (t_lo > t_hi) return fail(-EINVAL, "t_lo must be <= t_hi");
  if (cap && !out) return fail(-EINVAL, "null output");
  return sharded_query(
      r, cap, out, "raft_viol_read", [](Shard*) { return 0; },
      [&](Shard* s, raft_violation_t* dout, uint32_t dcap, const uint32_t** dtotal) {
        *dtotal = rs::viol_total_ptr(s->vscratch, s->C);
        return rs::launch_viol_query(s->d, kinds_mask, t_lo, t_hi, s->vscratch, dout, dcap,
                                     s->stream);
      },
      &Shard::viol_ms);
}

int raft_viol_clear(raft_sim_t* r) {
  if (!r) return fail(-EINVAL, "null sim");
  if (r->poisoned) return unusable();
  for (Shard* s : r->sh) {
    HIP_OK(hipSetDevice(s->cfg.device));
    HIP_OK(rs::launch_viol_clear(s->d, s->stream));
  }
  for (Shard* s : r->sh) {
    HIP_OK(hipSetDevice(s->cfg.device));
    HIP_OK(hipStreamSynchronize(s->stream));
  }
  return 0;
}

// Diagnostic (not part of include/raftsim.h): device time of the last raft_viol_read's kernels
// (HIP events around them on each shard's stream), the maximum over shards, in ms.
extern "C" int raftsim_diag_viol_ms(raft_sim_t* r, double* ms) {
  return diag_ms(r, ms, &Shard::viol_ms);
}

// ---------------------------------------------------------------------------------------------
// State census (include/raftsim.h, "no reference counterpart, none in the oracle"): read-only
// kernels over the hot blocks on every shard's stream at once, behind whatever the shard has
// enqueued. They touch neither the state nor the host's bookkeeping of it (storm_until,
// keys_written, the steady path choice), so a certificate stays and the next step runs as it would
// have. The census goes through sharded_summary, selections through sharded_query.
static int census_prepare(Shard* s) {
  if (s->cscratch) return 0;
  return dalloc(s, &s->cscratch, rs::census_layout(s->C, s->N).words());   // freed by sh_destroy
}

int raft_census_read(raft_sim_t* r, raft_census_t* out) {
  if (!r || !out) return fail(-EINVAL, "null argument");
  if (r->poisoned) return unusable();
  return sharded_summary(
      r, out, "raft_census_read", census_prepare,
      [](Shard* s) { return rs::launch_census(s->d, s->cscratch, s->stream); },
      [](Shard* s) { return s->cscratch + rs::census_layout(s->C, s->N).result(); },
      &Shard::census_ms, [](Shard*) {});
}

int64_t raft_census_select(raft_sim_t* r, uint32_t any_mask, uint32_t all_mask, uint32_t none_mask,
                           raft_cluster_state_t* out, uint32_t cap) {
  if (!r) return fail(-EINVAL, "null sim");
  if (any_mask > RAFT_CLS_ALL || all_mask > RAFT_CLS_ALL || none_mask > RAFT_CLS_ALL)
    return fail(-EINVAL, "class masks must be <= RAFT_CLS_ALL (511)");
  if (all_mask & none_mask) return fail(-EINVAL, "all_mask and none_mask share a class");
  if (cap && !out) return fail(-EINVAL, "null output");
  if (r->poisoned) return unusable();
  return sharded_query(
      r, cap, out, "raft_census_select", census_prepare,
      [&](Shard* s, raft_cluster_state_t* dout, uint32_t dcap, const uint32_t** dtotal) {
        *dtotal = rs::census_layout(s->C, s->N).total_ptr(s->cscratch);
        return rs::launch_census_select(s->d, any_mask, all_mask, none_mask, s->cscratch, dout,
                                        dcap, s->stream);
      },
      &Shard::census_ms);
}

// Diagnostic (not part of include/raftsim.h): device time of the last raft_census_read's or
// raft_census_select's kernels (HIP events around them on each shard's stream), the maximum over
// shards, in ms.
extern "C" int raftsim_diag_census_ms(raft_sim_t* r, double* ms) {
  return diag_ms(r, ms, &Shard::census_ms);
}

// ---------------------------------------------------------------------------------------------
// Log audit (include/raftsim.h, "no reference counterpart, none in the oracle"): a read-only pass
// over the hot blocks and the arenas on every shard's stream at once, behind whatever the shard
// has enqueued. It leaves one record per cluster and the shard's summary on the device, valid
// until the next call that can change a log or a commit index (LaunchState::audit_valid): the
// summary is copied from there and folded over the shards on the host, selections compact the records
// through sharded_query. Like the census it touches neither the state nor the host's bookkeeping
// of it.
static int audit_prepare(Shard* s) {
  if (s->ascratch) return 0;
  int rc = dalloc(s, &s->arec, s->C);
  if (!rc) rc = dalloc(s, &s->ascratch, rs::audit_layout(s->C).words());   // freed by sh_destroy
  return rc;
}
// Enqueue the pass unless the shard's records are those of the state as it stands.
static hipError_t audit_refresh(Shard* s) {
  if (s->ls.audit_valid) return hipSuccess;
  // the pass's lanes per cluster (audit_kernel.hip; DESIGN.md has both widths' figures): 64 unless
  // RAFTSIM_AUDIT_WIDTH=16 is in the environment. Same records and summary either way.
  const char* aw = getenv("RAFTSIM_AUDIT_WIDTH");
  const uint32_t width = aw && !strcmp(aw, "16") ? 16u : 64u;
  const hipError_t e = rs::launch_audit(s->d, width, s->arec, s->ascratch, s->stream);
  s->ls.audit_valid = e == hipSuccess;
  return e;
}

int raft_audit_read(raft_sim_t* r, raft_audit_t* out) {
  if (!r || !out) return fail(-EINVAL, "null argument");
  if (r->poisoned) return unusable();
  return sharded_summary(
      r, out, "raft_audit_read", audit_prepare, audit_refresh,
      [](Shard* s) { return s->ascratch + rs::audit_layout(s->C).result(); },
      &Shard::audit_ms, [](Shard* s) { s->ls.audit_valid = false; });
}

int64_t raft_audit_select(raft_sim_t* r, uint32_t any_mask, uint32_t all_mask, uint32_t none_mask,
                          raft_audit_record_t* out, uint32_t cap) {
  if (!r) return fail(-EINVAL, "null sim");
  if (any_mask > RAFT_AUD_ALL || all_mask > RAFT_AUD_ALL || none_mask > RAFT_AUD_ALL)
    return fail(-EINVAL, "class masks must be <= RAFT_AUD_ALL (31)");
  if (all_mask & none_mask) return fail(-EINVAL, "all_mask and none_mask share a class");
  if (cap && !out) return fail(-EINVAL, "null output");
  if (r->poisoned) return unusable();
  const int64_t n = sharded_query(
      r, cap, out, "raft_audit_select", audit_prepare,
      [&](Shard* s, raft_audit_record_t* dout, uint32_t dcap, const uint32_t** dtotal) {
        *dtotal = rs::audit_layout(s->C).total_ptr(s->ascratch);
        const hipError_t e = audit_refresh(s);
        return e != hipSuccess ? e
                               : rs::launch_audit_select(s->C, any_mask, all_mask, none_mask,
                                                         s->arec, s->ascratch, dout, dcap,
                                                         s->stream);
      },
      &Shard::audit_ms);
  if (n < 0)
    for (Shard* s : r->sh) s->ls.audit_valid = false;
  return n;
}

// Diagnostic (not part of include/raftsim.h): device time of the last raft_audit_read's or
// raft_audit_select's kernels (HIP events around them on each shard's stream), the maximum over
// shards, in ms. A query that found the records valid ran no pass: its time is the copy's or the
// compaction's alone.
extern "C" int raftsim_diag_audit_ms(raft_sim_t* r, double* ms) {
  return diag_ms(r, ms, &Shard::audit_ms);
}

// ---------------------------------------------------------------------------------------------
// Cluster packs (include/raftsim.h, "no reference counterpart, none in the oracle"): a read-only
// kernel over the state of a list of clusters on every shard's stream at once, behind whatever the
// shard has enqueued. The caller's list is split by owner shard; a shard packs its clusters into
// its scratch, GATHER_SCRATCH_BYTES at a time, and every chunk is one device-to-host copy: straight
// into the caller's buffer where the shard's clusters stand at consecutive positions of the list
// (always, on one device), else into a host buffer whose records are moved to their positions once
// the shard is done. Like the census it touches neither the state nor the host's bookkeeping of it
// (storm_until, keys_written, lite, audit_valid, the steady path choice). The check of the list,
// the scratch, the events and the wait for a started shard are the pack calls' shared helpers.
constexpr uint64_t GATHER_SCRATCH_BYTES = 64ull << 20;

static void gather_layout_of(const Shard* s, uint32_t parts, raft_gather_layout_t* y) {
  const uint64_t N = s->N;
  const uint64_t size[6] = {sizeof(raft_cluster_t),
                            N * sizeof(raft_node_t),
                            N * 2 * s->Q * sizeof(raft_msg_t),
                            N * s->L * sizeof(raft_entry_t),
                            N * s->A * sizeof(raft_entry_t),
                            N * s->cfg.commit_stream_cap * sizeof(uint32_t)};
  uint64_t off = 0;
  for (int b = 0; b < 6; ++b) {
    const bool on = (parts >> b) & 1;
    y->off[b] = on ? off : UINT64_MAX;
    y->size[b] = on ? size[b] : 0;
    if (on) off += (size[b] + 15) & ~15ull;
  }
  y->stride = off;
}

static int gather_parts_ok(uint32_t parts) {
  if (parts == 0 || parts > RAFT_GATHER_ALL)
    return fail(-EINVAL, "parts must be 1..RAFT_GATHER_ALL (63)");
  return 0;
}

int raft_gather_layout(raft_sim_t* r, uint32_t parts, raft_gather_layout_t* out) {
  if (!r || !out) return fail(-EINVAL, "null argument");
  const int rc = gather_parts_ok(parts);
  if (rc) return rc;
  gather_layout_of(r->sh[0], parts, out);
  return 0;
}

// What raft_gather_read and raft_scatter_write (the pack calls) share on the host.

// Position i of a pack call's cluster list lies in the handle.
static int pack_cluster_ok(const raft_sim* r, const uint32_t* clusters, uint32_t i) {
  if (clusters[i] < r->cfg.n_clusters) return 0;
  char what[96];
  snprintf(what, sizeof what, "clusters[%u] = %u is outside the handle's %u clusters", i,
           clusters[i], r->cfg.n_clusters);
  return fail(-EINVAL, "%s", what);
}

// The HIP calls of a pack call `who`: the first failure becomes the call's return code, with
// who's name in the text, and every later step is skipped.
struct PackCall {
  const char* who;
  int rc = 0;
  void failed(int code, const char* what, hipError_t e) {
    char text[sizeof g_err];
    snprintf(text, sizeof text, "%s in %s: %s", what, who, hipGetErrorString(e));
    rc = fail(code, "%s", text);
  }
  bool step(hipError_t e) {
    if (!rc && e != hipSuccess) failed(-EIO, "HIP error", e);
    return !rc;
  }
};

// The shard's scratch holds `need` bytes (a larger one is made once the stream is done with the
// smaller), and the shard has an event pair for each of `chunks` kernels.
static bool pack_scratch(PackCall& p, Shard* s, size_t need) {
  if (s->gscratch_bytes >= need) return true;
  if (!p.step(hipStreamSynchronize(s->stream))) return false;
  if (s->gscratch) (void)hipFree(s->gscratch);
  s->gscratch = nullptr;
  s->gscratch_bytes = 0;
  void* v = nullptr;
  const hipError_t e = hipMalloc(&v, need);
  if (e != hipSuccess) {
    p.failed(-ENOMEM, "hipMalloc failed", e);
    return false;
  }
  s->gscratch = static_cast<uint8_t*>(v);
  s->gscratch_bytes = need;
  return true;
}
static bool pack_events(PackCall& p, Shard* s, size_t chunks) {
  while (!p.rc && s->gev.size() < 2 * chunks) {
    hipEvent_t e;
    if (p.step(hipEventCreate(&e))) s->gev.push_back(e);
  }
  return !p.rc;
}

// Wait for a started shard -- also after an error, of this shard or of an earlier one: its copies
// read or write the caller's buffers and the stages -- and, when all went well, make the summed
// kernel times of its `chunks` event pairs its *ms.
static bool pack_wait(PackCall& p, Shard* s, size_t chunks, double Shard::*ms) {
  p.step(hipSetDevice(s->cfg.device));
  p.step(hipStreamSynchronize(s->stream));
  double sum = 0;
  for (size_t ch = 0; ch < chunks && !p.rc; ++ch) {
    float t = 0;
    if (p.step(hipEventElapsedTime(&t, s->gev[2 * ch], s->gev[2 * ch + 1]))) sum += t;
  }
  if (!p.rc) s->*ms = sum;
  return !p.rc;
}

// One shard's share of a raft_gather_read.
struct GatherJob {
  std::vector<uint2> pairs;     // (shard-local cluster, slot in its chunk's scratch)
  std::vector<uint32_t> pos;    // the record's position in the caller's list
  std::vector<uint8_t> stage;   // the shard's records in list order, unless they go straight to out
  uint8_t* host = nullptr;      // where chunk 0's first record goes
  uint32_t per_chunk = 0, chunks = 0;
};

int64_t raft_gather_read(raft_sim_t* r, const uint32_t* clusters, uint32_t n, uint32_t parts,
                         void* out, uint64_t cap_bytes) {
  if (!r) return fail(-EINVAL, "null sim");
  int rc = gather_parts_ok(parts);
  if (rc) return rc;
  if (n && !clusters) return fail(-EINVAL, "null cluster list");
  if (n && !out) return fail(-EINVAL, "null output");
  for (uint32_t i = 0; i < n; ++i)
    if ((rc = pack_cluster_ok(r, clusters, i))) return rc;
  raft_gather_layout_t Y;
  gather_layout_of(r->sh[0], parts, &Y);
  const uint64_t stride = Y.stride, bytes = (uint64_t)n * stride;   // stride < 2^31: no overflow
  if (cap_bytes < bytes) return fail(-ERANGE, "cap_bytes is below n * stride");
  if (r->poisoned) return unusable();
  if (!bytes) return 0;          // no cluster, or the commit streams alone of a handle without them

  const size_t G = r->sh.size();
  std::vector<GatherJob> job(G);
  for (uint32_t i = 0; i < n; ++i) {
    const size_t d = owner_index(r, clusters[i]);
    job[d].pairs.push_back(make_uint2(clusters[i] - r->lo[d], 0));
    job[d].pos.push_back(i);
  }
  // records and their list entries share the scratch: stride + 8 bytes each, one record at least
  const uint32_t per_chunk =
      (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(GATHER_SCRATCH_BYTES / (stride + 8), n));
  uint8_t* const dst = static_cast<uint8_t*>(out);
  PackCall hip = {"raft_gather_read"};
  size_t started = 0;
  for (size_t d = 0; d < G && !hip.rc; ++d) {
    Shard* s = r->sh[d];
    GatherJob& j = job[d];
    const size_t m = j.pairs.size();
    ++started;
    if (!m) continue;
    bool direct = true;
    for (size_t i = 1; i < m && direct; ++i) direct = j.pos[i] == j.pos[0] + i;
    if (direct) j.host = dst + (size_t)j.pos[0] * stride;
    else {
      j.stage.resize(m * stride);
      j.host = j.stage.data();
    }
    j.per_chunk = (uint32_t)std::min<size_t>(per_chunk, m);
    j.chunks = (uint32_t)((m + j.per_chunk - 1) / j.per_chunk);
    for (size_t i = 0; i < m; ++i) j.pairs[i].y = (uint32_t)(i % j.per_chunk);
    if (!hip.step(hipSetDevice(s->cfg.device)) ||
        !pack_scratch(hip, s, (size_t)j.per_chunk * (stride + 8)) || !pack_events(hip, s, j.chunks))
      break;
    // the list stands behind the records (stride is a multiple of 16)
    uint2* const dpairs = reinterpret_cast<uint2*>(s->gscratch + (size_t)j.per_chunk * stride);
    for (uint32_t ch = 0; ch < j.chunks && !hip.rc; ++ch) {
      const size_t i0 = (size_t)ch * j.per_chunk;
      const uint32_t k = (uint32_t)std::min<size_t>(j.per_chunk, m - i0);
      hip.step(h2d(s, dpairs, j.pairs.data() + i0, k)) &&
          hip.step(hipEventRecord(s->gev[2 * ch], s->stream)) &&
          hip.step(rs::launch_gather(s->d, dpairs, k, Y, s->gscratch, s->stream)) &&
          hip.step(hipEventRecord(s->gev[2 * ch + 1], s->stream)) &&
          hip.step(hipMemcpyAsync(j.host + i0 * stride, s->gscratch, (size_t)k * stride,
                                  hipMemcpyDeviceToHost, s->stream));
    }
  }
  // every started shard is waited for, also after an error: its copies write out and the stages
  for (size_t d = 0; d < started; ++d) {
    Shard* s = r->sh[d];
    GatherJob& j = job[d];
    if (j.pairs.empty()) {
      if (!hip.rc) s->gather_ms = 0;
      continue;
    }
    if (pack_wait(hip, s, j.chunks, &Shard::gather_ms) && !j.stage.empty())
      for (size_t i = 0; i < j.pos.size(); ++i)
        memcpy(dst + (size_t)j.pos[i] * stride, j.stage.data() + i * stride, stride);
  }
  return hip.rc ? hip.rc : (int64_t)bytes;
}

// Diagnostic (not part of include/raftsim.h): device time of the last raft_gather_read's kernels
// (HIP events around each chunk's kernel on each shard's stream, summed), the maximum over shards,
// in ms.
extern "C" int raftsim_diag_gather_ms(raft_sim_t* r, double* ms) {
  return diag_ms(r, ms, &Shard::gather_ms);
}

// ---------------------------------------------------------------------------------------------
// Cluster packs written back: the gather turned round. Everything that can refuse the call is
// checked on the host first (scatter_host.hpp: the ranges, a target named twice, every referenced
// record against the predicates of raft_sim_write_nodes and raft_sim_write_queue), so a refused
// call has touched no device. The (record, target) pairs are sorted by owner shard and record and
// cut into chunks of the shard's scratch (the gather's, GATHER_SCRATCH_BYTES): a chunk's distinct
// records are uploaded once each, its (local cluster, slot) list behind them, and one kernel
// writes its targets; the chunks of a shard follow each other on its stream, all shards run at
// once, and every started shard is waited for (pack_wait). The host's bookkeeping of a touched
// shard is what the per-node writes leave, taken together.
static const char* const NODE_FAULT_TEXT[] = {
    "", "role > 3", "voted_for > nodes", "leader_id > nodes", "fault > 4",
    "votes outside ids 1..nodes", "ls_keys outside the peers", "entries_is_seq > 1", "ls_present > 1", "log_len > log_cap",
    "arena_frontier - arena_base < log_len", "arena_frontier - arena_base > log_cap",
    "a leader without its leader-state keys", "ls_keys without ls_present"};
static const char* const QUEUE_FAULT_TEXT[] = {
    "", "count > inbox_cap", "type outside 1..5", "a message of the other queue", "src > nodes",
    "src is the node itself", "client-set and src 0 do not go together", "arrivals decrease"};

int64_t raft_scatter_write(raft_sim_t* r, const uint32_t* clusters, const uint32_t* records,
                           uint32_t n, uint32_t parts, const void* in, uint32_t n_records) {
  if (!r) return fail(-EINVAL, "null sim");
  int rc = gather_parts_ok(parts);
  if (rc) return rc;
  static const char* const part_name[] = {"CLUSTER", "NODES",  "QUEUES",
                                          "LOGS",    "ARENAS", "STREAMS"};
  for (int b : {0, 1, 2, 4})
    if (!((parts >> b) & 1))
      return fail(-EINVAL, "raft_scatter_write needs the part RAFT_GATHER_%s", part_name[b]);
  if (n && !clusters) return fail(-EINVAL, "null cluster list");
  if (n && !in) return fail(-EINVAL, "null input");
  if (r->cfg.commit_stream_cap && !(parts & RAFT_GATHER_STREAMS))
    return fail(-EINVAL, "raft_scatter_write needs the part RAFT_GATHER_%s", part_name[5]);
  char what[160];
  for (uint32_t i = 0; i < n; ++i) {
    if ((rc = pack_cluster_ok(r, clusters, i))) return rc;
    const uint32_t rec = records ? records[i] : i;
    if (rec >= n_records) {
      snprintf(what, sizeof what, "records[%u] = %u is outside the buffer's %u records", i, rec,
               n_records);
      return fail(-EINVAL, "%s", what);
    }
  }
  const uint32_t dup = rs::first_duplicate(clusters, n);
  if (dup < n) {
    snprintf(what, sizeof what, "clusters[%u] = %u is a target twice", dup, clusters[dup]);
    return fail(-EINVAL, "%s", what);
  }
  if (r->poisoned) return unusable();
  if (!n) return 0;

  raft_gather_layout_t Y;
  gather_layout_of(r->sh[0], parts, &Y);
  const uint64_t stride = Y.stride;
  const size_t G = r->sh.size();
  const rs::ScatterPlan plan = rs::scatter_plan(clusters, records, n, r->lo.data(), (uint32_t)G,
                                                stride, GATHER_SCRATCH_BYTES);
  const uint8_t* const src = static_cast<const uint8_t*>(in);
  // every referenced record, once per chunk that uploads it; the first offending position is named
  const rs::RecordShape shape = {r->cfg.nodes, r->cfg.inbox_cap, r->cfg.log_cap, Y.off[0], Y.off[1],
                                 Y.off[2]};
  std::vector<uint8_t> general(G, 0);
  uint32_t bad_pos = UINT32_MAX;
  rs::RecordVerdict bad = {};
  for (const rs::ScatterChunk& ch : plan.chunks) {
    size_t pi = ch.pair0;
    for (size_t k = 0; k < ch.records; ++k) {
      const rs::RecordVerdict v =
          rs::record_verdict(src + (size_t)plan.records[ch.rec0 + k] * stride, shape);
      general[ch.shard] |= v.general;
      uint32_t pos = UINT32_MAX;                 // the record's first position in this chunk
      for (; pi < ch.pair0 + ch.pairs && plan.pairs[pi].slot == k; ++pi)
        pos = std::min(pos, plan.pos[pi]);
      if (!v.ok() && pos < bad_pos) {
        bad_pos = pos;
        bad = v;
      }
    }
  }
  if (bad_pos != UINT32_MAX) {
    const uint32_t rec = records ? records[bad_pos] : bad_pos;
    if (bad.node_fault)
      snprintf(what, sizeof what, "records[%u] = %u: invalid node record (node %u: %s)", bad_pos,
               rec, bad.id, NODE_FAULT_TEXT[bad.node_fault]);
    else
      snprintf(what, sizeof what, "records[%u] = %u: invalid message or order (node %u, %s message "
               "%u: %s)", bad_pos, rec, bad.id, bad.which ? "res" : "req", bad.msg,
               QUEUE_FAULT_TEXT[bad.queue_fault]);
    return fail(-EINVAL, "%s", what);
  }

  PackCall hip = {"raft_scatter_write"};
  // Per shard: its chunks [first, first + count) of the plan and the scratch the largest needs. A
  // chunk's records are staged in slot order (one host copy), unless they stand in the caller's
  // buffer as a run in that order (a pack used whole: uploaded straight from the buffer).
  std::vector<size_t> first(G, 0), count(G, 0);
  for (size_t i = 0; i < plan.chunks.size(); ++i) {
    const uint32_t d = plan.chunks[i].shard;
    if (!count[d]) first[d] = i;
    ++count[d];
  }
  // the staging buffers live until every shard has been waited for
  std::vector<std::vector<uint8_t>> stages(plan.chunks.size());
  std::vector<size_t> started;
  for (size_t d = 0; d < G && !hip.rc; ++d) {
    if (!count[d]) continue;
    Shard* s = r->sh[d];
    started.push_back(d);
    if (!hip.step(hipSetDevice(s->cfg.device))) break;
    rs::invalidate(s->ls, rs::ON_SCATTER);
    if (general[d]) rs::invalidate(s->ls, rs::ON_SCATTER_GENERAL);
    size_t need = 0;
    for (size_t i = first[d]; i < first[d] + count[d]; ++i)
      need = std::max<size_t>(need, plan.chunks[i].bytes(stride));
    if (!pack_scratch(hip, s, need) || !pack_events(hip, s, count[d])) break;
    for (size_t i = 0; i < count[d] && !hip.rc; ++i) {
      const rs::ScatterChunk& ch = plan.chunks[first[d] + i];
      const uint32_t* const recs = plan.records.data() + ch.rec0;
      bool run = true;                           // the records stand in the buffer as in the chunk
      for (size_t k = 1; k < ch.records && run; ++k) run = recs[k] == recs[0] + k;
      const uint8_t* up = src + (size_t)recs[0] * stride;
      if (!run) {
        std::vector<uint8_t>& st = stages[first[d] + i];
        st.resize(ch.records * stride);
        for (size_t k = 0; k < ch.records; ++k)
          memcpy(st.data() + k * stride, src + (size_t)recs[k] * stride, stride);
        up = st.data();
      }
      // the list stands behind the records (stride is a multiple of 16)
      uint8_t* const dpairs = s->gscratch + ch.records * stride;
      hip.step(hipMemcpyAsync(s->gscratch, up, ch.records * stride, hipMemcpyHostToDevice,
                              s->stream)) &&
          hip.step(hipMemcpyAsync(dpairs, plan.pairs.data() + ch.pair0,
                                  ch.pairs * sizeof(rs::ScatterPair), hipMemcpyHostToDevice,
                                  s->stream)) &&
          hip.step(hipEventRecord(s->gev[2 * i], s->stream)) &&
          hip.step(rs::launch_scatter(s->d, dpairs, (uint32_t)ch.pairs, Y, s->gscratch,
                                      s->stream)) &&
          hip.step(hipEventRecord(s->gev[2 * i + 1], s->stream));
    }
  }
  // every started shard is waited for, also after an error: its uploads read the stages
  for (size_t d : started) pack_wait(hip, r->sh[d], count[d], &Shard::scatter_ms);
  if (!hip.rc)
    for (size_t d = 0; d < G; ++d)
      if (!count[d]) r->sh[d]->scatter_ms = 0;
  return hip.rc ? hip.rc : (int64_t)n;
}

// Diagnostic (not part of include/raftsim.h): device time of the last raft_scatter_write's kernels
// (HIP events around each chunk's kernel on each shard's stream, summed), the maximum over shards,
// in ms.
extern "C" int raftsim_diag_scatter_ms(raft_sim_t* r, double* ms) {
  return diag_ms(r, ms, &Shard::scatter_ms);
}

// ---------------------------------------------------------------------------------------------
// Cluster clones: the scatter of a gather without the pack (include/raftsim.h, "Cluster clones").
// Everything that can refuse the call is checked on the host first (clone_host.hpp: the ranges, a
// target named twice, a cluster both read and written; here the handles' shapes and devices), so a
// refused call has touched no device. The (target, source) pairs are grouped by the shards they
// join and cut into chunks of the target shard's scratch (the gather's, GATHER_SCRATCH_BYTES at 8
// bytes a pair): a chunk's list is uploaded and one kernel writes its targets from the source
// shard's state. A target shard's stream first waits for an event on the stream of every other
// shard it reads, so the call is ordered after everything enqueued on both handles; the chunks of a
// shard follow each other on its stream, all target shards run at once, and every started shard is
// waited for (pack_wait). The host's bookkeeping of a touched target shard is a scatter's; a
// source shard is only read.
int64_t raft_clone_write(raft_sim_t* dst, const uint32_t* targets, raft_sim_t* src,
                         const uint32_t* sources, uint32_t n) {
  if (!dst || !src) return fail(-EINVAL, "null sim");
  if (n && !targets) return fail(-EINVAL, "null target list");
  if (n && !sources) return fail(-EINVAL, "null source list");
  char what[200];
  {
    const Shard *t = dst->sh[0], *s = src->sh[0];
    const struct {
      const char* name;
      uint32_t dst, src;
    } shape[] = {{"nodes", t->N, s->N},
                 {"inbox_cap", t->Q, s->Q},
                 {"log_cap", t->L, s->L},
                 {"arena_cap", t->A, s->A},
                 {"commit_stream_cap", t->cfg.commit_stream_cap, s->cfg.commit_stream_cap}};
    for (const auto& f : shape)
      if (f.dst != f.src) {
        snprintf(what, sizeof what, "the handles differ in %s: the target's is %u, the source's %u",
                 f.name, f.dst, f.src);
        return fail(-EINVAL, "%s", what);
      }
  }
  for (uint32_t i = 0; i < n; ++i) {
    const bool t_out = targets[i] >= dst->cfg.n_clusters;
    if (!t_out && sources[i] < src->cfg.n_clusters) continue;
    snprintf(what, sizeof what, "%s[%u] = %u is outside the handle's %u clusters",
             t_out ? "targets" : "sources", i, t_out ? targets[i] : sources[i],
             t_out ? dst->cfg.n_clusters : src->cfg.n_clusters);
    return fail(-EINVAL, "%s", what);
  }
  const uint32_t dup = rs::first_duplicate(targets, n);
  if (dup < n) {
    snprintf(what, sizeof what, "targets[%u] = %u is a target twice", dup, targets[dup]);
    return fail(-EINVAL, "%s", what);
  }
  if (src == dst) {
    bool target_is_source = false;
    const uint32_t at = rs::first_source_target(targets, sources, n, &target_is_source);
    if (at < n) {
      snprintf(what, sizeof what, "%s[%u] = %u is both a source and a target of the handle",
               target_is_source ? "targets" : "sources", at,
               target_is_source ? targets[at] : sources[at]);
      return fail(-EINVAL, "%s", what);
    }
  }
  const size_t TG = dst->sh.size(), SG = src->sh.size();
  const rs::ClonePlan plan =
      rs::clone_plan(targets, dst->lo.data(), (uint32_t)TG, sources, src->lo.data(), (uint32_t)SG, n,
                     GATHER_SCRATCH_BYTES / sizeof(rs::ClonePair));
  uint32_t far = UINT32_MAX;                     // the first position that joins two devices
  for (const rs::CloneChunk& ch : plan.chunks)
    if (dst->sh[ch.dst_shard]->cfg.device != src->sh[ch.src_shard]->cfg.device)
      far = std::min(far, *std::min_element(plan.pos.begin() + ch.pair0,
                                            plan.pos.begin() + ch.pair0 + ch.pairs));
  if (far != UINT32_MAX) {
    snprintf(what, sizeof what, "sources[%u] = %u and targets[%u] = %u live on different devices: "
             "clone across devices through raft_gather_read and raft_scatter_write", far,
             sources[far], far, targets[far]);
    return fail(-EXDEV, "%s", what);
  }
  if (dst->poisoned || src->poisoned) return unusable();
  if (!n) return 0;

  raft_gather_layout_t Y;
  gather_layout_of(dst->sh[0],
                   RAFT_GATHER_CLUSTER | RAFT_GATHER_NODES | RAFT_GATHER_QUEUES | RAFT_GATHER_ARENAS |
                       (dst->cfg.commit_stream_cap ? RAFT_GATHER_STREAMS : 0),
                   &Y);
  // Per target shard: its chunks [first, first + count) of the plan, and whether it reads a shard
  // that is no longer LITE (asked before any shard is marked: src may be dst).
  std::vector<size_t> first(TG, 0), count(TG, 0);
  std::vector<uint8_t> general(TG, 0), read(SG, 0);
  for (size_t i = 0; i < plan.chunks.size(); ++i) {
    const rs::CloneChunk& ch = plan.chunks[i];
    if (!count[ch.dst_shard]) first[ch.dst_shard] = i;
    ++count[ch.dst_shard];
    general[ch.dst_shard] |= !src->sh[ch.src_shard]->ls.lite;
    read[ch.src_shard] = 1;
  }
  PackCall hip = {"raft_clone_write"};
  for (size_t e = 0; e < SG && !hip.rc; ++e)
    if (read[e])
      hip.step(hipSetDevice(src->sh[e]->cfg.device)) &&
          hip.step(hipEventRecord(src->sh[e]->cev, src->sh[e]->stream));
  std::vector<size_t> started;
  for (size_t d = 0; d < TG && !hip.rc; ++d) {
    if (!count[d]) continue;
    Shard* s = dst->sh[d];
    started.push_back(d);
    if (!hip.step(hipSetDevice(s->cfg.device))) break;
    rs::invalidate(s->ls, rs::ON_CLONE);
    if (general[d]) rs::invalidate(s->ls, rs::ON_CLONE_GENERAL);
    size_t need = 0;
    for (size_t i = first[d]; i < first[d] + count[d]; ++i)
      need = std::max(need, plan.chunks[i].pairs * sizeof(rs::ClonePair));
    if (!pack_scratch(hip, s, need) || !pack_events(hip, s, count[d])) break;
    const Shard* waited = nullptr;               // a shard's chunks stand source shard by source shard
    for (size_t i = 0; i < count[d] && !hip.rc; ++i) {
      const rs::CloneChunk& ch = plan.chunks[first[d] + i];
      const Shard* q = src->sh[ch.src_shard];
      if (q != s && q != waited && !hip.step(hipStreamWaitEvent(s->stream, q->cev, 0))) break;
      waited = q;
      hip.step(hipMemcpyAsync(s->gscratch, plan.pairs.data() + ch.pair0,
                              ch.pairs * sizeof(rs::ClonePair), hipMemcpyHostToDevice,
                              s->stream)) &&
          hip.step(hipEventRecord(s->gev[2 * i], s->stream)) &&
          hip.step(rs::launch_clone(s->d, q->d, s->gscratch, (uint32_t)ch.pairs, Y.stride,
                                    s->stream)) &&
          hip.step(hipEventRecord(s->gev[2 * i + 1], s->stream));
    }
  }
  // every started shard is waited for, also after an error: its uploads read the plan
  for (size_t d : started) pack_wait(hip, dst->sh[d], count[d], &Shard::clone_ms);
  if (!hip.rc)
    for (size_t d = 0; d < TG; ++d)
      if (!count[d]) dst->sh[d]->clone_ms = 0;
  return hip.rc ? hip.rc : (int64_t)n;
}

// Diagnostic (not part of include/raftsim.h): device time of the last raft_clone_write's kernels
// into this handle (HIP events around each chunk's kernel on each target shard's stream, summed),
// the maximum over shards, in ms.
extern "C" int raftsim_diag_clone_ms(raft_sim_t* dst, double* ms) {
  return diag_ms(dst, ms, &Shard::clone_ms);
}

// ---------------------------------------------------------------------------------------------
// Node restarts (include/raftsim.h, "Node restarts"; SIM_SPEC §4a). Everything that can refuse a
// call is checked on the host first (restart_host.hpp), so a refused call has touched no device.
// Both forms go through the pack calls' path: the shard's gather scratch takes a chunk's list of
// (cluster, mask) pairs (8 bytes a pair, GATHER_SCRATCH_BYTES at a time) or, for the `where` form,
// the shard's counter; an event pair stands around each kernel; all shards run at once and every
// started shard is waited for (pack_wait). The host's bookkeeping of a touched shard is a
// scatter's without INV_LITE (launch_plan.hpp, ON_RESTART).
static int restart_args_ok(const raft_sim* r, uint32_t mode) {
  if (mode > RAFT_RESTART_DURABLE)
    return fail(-EINVAL, "mode must be RAFT_RESTART_AMNESIA (0) or RAFT_RESTART_DURABLE (1)");
  if (!r) return fail(-EINVAL, "null sim");
  return 0;
}
static int restart_horizon(const raft_sim* r) {
  if (!rs::restart_horizon_ok(r->tick, r->cfg.el_base, r->cfg.el_span))
    return fail(-ERANGE, "tick + el_base + el_span would reach 2^32-1");
  return 0;
}

int64_t raft_restart_write(raft_sim_t* r, const uint32_t* clusters, const uint16_t* nodes,
                           uint32_t n, uint32_t mode) {
  int rc = restart_args_ok(r, mode);
  if (rc) return rc;
  if (n && !clusters) return fail(-EINVAL, "null cluster list");
  if (n && !nodes) return fail(-EINVAL, "null node mask list");
  uint32_t at = 0;
  char what[160];
  switch (rs::restart_list_fault(clusters, nodes, n, r->cfg.n_clusters, r->cfg.nodes, &at)) {
    case rs::RESTART_OK: break;
    case rs::RESTART_OUTSIDE: return pack_cluster_ok(r, clusters, at);
    case rs::RESTART_TWICE:
      snprintf(what, sizeof what, "clusters[%u] = %u is named twice", at, clusters[at]);
      return fail(-EINVAL, "%s", what);
    case rs::RESTART_MASK:
      snprintf(what, sizeof what, "nodes[%u] = 0x%x names no node or a node outside ids 1..%u", at,
               nodes[at], r->cfg.nodes);
      return fail(-EINVAL, "%s", what);
  }
  if ((rc = restart_horizon(r))) return rc;
  if (r->poisoned) return unusable();
  if (!n) return 0;

  const size_t G = r->sh.size();
  const rs::RestartPlan plan = rs::restart_plan(clusters, nodes, n, r->lo.data(), (uint32_t)G,
                                                GATHER_SCRATCH_BYTES / sizeof(rs::RestartPair));
  std::vector<size_t> first(G, 0), count(G, 0);          // per shard: its chunks of the plan
  for (size_t i = 0; i < plan.chunks.size(); ++i) {
    const uint32_t d = plan.chunks[i].shard;
    if (!count[d]) first[d] = i;
    ++count[d];
  }
  const uint32_t T = (uint32_t)r->tick;
  PackCall hip = {"raft_restart_write"};
  std::vector<size_t> started;
  for (size_t d = 0; d < G && !hip.rc; ++d) {
    if (!count[d]) continue;
    Shard* s = r->sh[d];
    started.push_back(d);
    if (!hip.step(hipSetDevice(s->cfg.device))) break;
    rs::invalidate(s->ls, rs::ON_RESTART);
    size_t need = 0;
    for (size_t i = first[d]; i < first[d] + count[d]; ++i)
      need = std::max(need, plan.chunks[i].pairs * sizeof(rs::RestartPair));
    if (!pack_scratch(hip, s, need) || !pack_events(hip, s, count[d])) break;
    for (size_t i = 0; i < count[d] && !hip.rc; ++i) {
      const rs::RestartChunk& ch = plan.chunks[first[d] + i];
      hip.step(hipMemcpyAsync(s->gscratch, plan.pairs.data() + ch.pair0,
                              ch.pairs * sizeof(rs::RestartPair), hipMemcpyHostToDevice,
                              s->stream)) &&
          hip.step(hipEventRecord(s->gev[2 * i], s->stream)) &&
          hip.step(rs::launch_restart(s->d, s->gscratch, (uint32_t)ch.pairs, mode, T, s->stream)) &&
          hip.step(hipEventRecord(s->gev[2 * i + 1], s->stream));
    }
  }
  // every started shard is waited for, also after an error: its uploads read the plan
  for (size_t d : started) pack_wait(hip, r->sh[d], count[d], &Shard::restart_ms);
  if (!hip.rc)
    for (size_t d = 0; d < G; ++d)
      if (!count[d]) r->sh[d]->restart_ms = 0;
  return hip.rc ? hip.rc : (int64_t)plan.nodes;
}

int64_t raft_restart_where(raft_sim_t* r, uint32_t fault_mask, uint32_t mode) {
  if (fault_mask == 0 || fault_mask > 31) return fail(-EINVAL, "fault_mask must be 1..31");
  int rc = restart_args_ok(r, mode);
  if (rc) return rc;
  if ((rc = restart_horizon(r))) return rc;
  if (r->poisoned) return unusable();

  const size_t G = r->sh.size();
  const uint32_t T = (uint32_t)r->tick;
  std::vector<uint32_t> found(G, 0);                     // the shards' counters, read back
  PackCall hip = {"raft_restart_where"};
  size_t started = 0;
  for (size_t d = 0; d < G && !hip.rc; ++d) {
    Shard* s = r->sh[d];
    ++started;
    if (!hip.step(hipSetDevice(s->cfg.device))) break;
    rs::invalidate(s->ls, rs::ON_RESTART);
    if (!pack_scratch(hip, s, sizeof(uint32_t)) || !pack_events(hip, s, 1)) break;
    uint32_t* const dcount = reinterpret_cast<uint32_t*>(s->gscratch);
    hip.step(hipMemsetAsync(dcount, 0, sizeof(uint32_t), s->stream)) &&
        hip.step(hipEventRecord(s->gev[0], s->stream)) &&
        hip.step(rs::launch_restart_where(s->d, fault_mask, mode, T, dcount, s->stream)) &&
        hip.step(hipEventRecord(s->gev[1], s->stream)) &&
        hip.step(d2h(s, &found[d], dcount, 1));
  }
  // every started shard is waited for, also after an error: its copy writes `found`
  for (size_t d = 0; d < started; ++d) pack_wait(hip, r->sh[d], 1, &Shard::restart_ms);
  int64_t total = 0;
  for (uint32_t f : found) total += f;
  return hip.rc ? hip.rc : total;
}

// Diagnostic (not part of include/raftsim.h): device time of the last raft_restart_write's or
// raft_restart_where's kernels (HIP events around each kernel on each shard's stream, summed), the
// maximum over shards, in ms.
extern "C" int raftsim_diag_restart_ms(raft_sim_t* r, double* ms) {
  return diag_ms(r, ms, &Shard::restart_ms);
}

// Build identity (not part of include/raftsim.h): the hash of the kernel sources this library was
// compiled from (raftsim/_build.py; __graft_entry__.build_lib passes it), also findable in the
// file's bytes as "RAFTSIM_SRC_HASH=<hash>" without loading it. A diagnostic build (device.hpp's
// switches) is "diag" whatever hash was passed: raftsim.check_build refuses it.
#ifdef RS_DIAG_BUILD
#undef RAFTSIM_SRC_HASH
#define RAFTSIM_SRC_HASH "diag"
#endif
#ifndef RAFTSIM_SRC_HASH
#define RAFTSIM_SRC_HASH "unknown"
#endif
static const char g_src_tag[] = "RAFTSIM_SRC_HASH=" RAFTSIM_SRC_HASH;
extern "C" const char* raftsim_src_hash(void) { return g_src_tag + 17; }

// Diagnostic (not part of include/raftsim.h): how many launches of the last sync window the
// average of raft_sim_last_step_timing is taken over (every general launch; the first steady
// launch after a sync), summed over shards.
extern "C" int raftsim_last_timed_launches(raft_sim_t* r) {
  if (!r) return fail(-EINVAL, "null sim");
  int n = 0;
  for (Shard* s : r->sh) n += (int)s->last_timed;
  return n;
}

// Diagnostic (not part of include/raftsim.h): clusters the steady kernel handed to the catch-up
// launch in the handle's last tick launch, summed over shards; -1 if that launch did not take the
// steady path (tests use it to check which path ran; results never depend on it).
extern "C" int raftsim_diag_last_bails(raft_sim_t* r) {
  if (!r) return fail(-EINVAL, "null sim");
  int total = 0;
  for (Shard* s : r->sh) {
    if (s->ls.last_path != rs::PATH_STEADY) return -1;
    uint32_t v = 0;
    HIP_OK(hipSetDevice(s->cfg.device));
    HIP_OK(hipStreamSynchronize(s->stream));
    HIP_OK(hipMemcpy(&v, s->nbail2 + (s->ls.steady_parity ^ 1), 4, hipMemcpyDeviceToHost));
    total += (int)v;
  }
  return total;
}

// Diagnostic (not part of include/raftsim.h): clusters the storm kernel listed for the
// lane-per-node STORM body in the last storm-kernel launch (storm_kernel.hip), summed over shards;
// -1 if no shard has run one. Tests bound it: a regression that reruns most clusters shows here.
extern "C" int raftsim_diag_storm_bails(raft_sim_t* r) {
  if (!r) return fail(-EINVAL, "null sim");
  int total = 0;
  bool any = false;
  for (Shard* s : r->sh) {
    if (!s->ls.storm_kernel_ran) continue;
    any = true;
    uint32_t v = 0;
    HIP_OK(hipSetDevice(s->cfg.device));
    HIP_OK(hipStreamSynchronize(s->stream));
    HIP_OK(hipMemcpy(&v, s->d.storm_count, 4, hipMemcpyDeviceToHost));
    total += (int)v;
  }
  return any ? total : -1;
}

#ifdef RS_WAVELOG
// Diagnostic builds only (not part of include/raftsim.h): the per-wave timeline of shard 0's last
// tick-kernel launch, 8 words per wave: start lo/hi, end lo/hi (100 MHz), active ticks, HW_ID,
// XCC_ID, launch t0. Returns the number of waves.
extern "C" int raftsim_diag_wavelog(raft_sim_t* r, uint32_t* out, uint32_t cap_waves) {
  Shard* s = r->sh[0];
  const uint32_t waves = rs::sched_slots_bound(s->C, s->N) / (64 / s->N);
  const uint32_t n = std::min(waves, cap_waves);
  HIP_OK(hipSetDevice(s->cfg.device));
  HIP_OK(hipMemcpy(out, s->d.wavelog, (size_t)n * 192, hipMemcpyDeviceToHost));
  return (int)n;
}
#endif
