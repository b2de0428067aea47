/* raftsim.h — C ABI of libraftsim.so, the MI355X batched Raft simulator.
 *
 * The reference (angelini/raft-simulation) has no FFI; its seams are the handler loop and the
 * three side-effect functions it calls. Each entry point below says which reference interface it
 * replaces. Semantics: SIM_SPEC.md. Conventions: 0 on success, a negative errno on failure
 * (-EINVAL bad argument, -ENOMEM allocation, -EIO HIP error); nothing throws across the ABI;
 * output buffers are caller-allocated; the library owns device memory; a handle is used by one
 * host thread at a time. `raft_sim_last_error()` explains the last failure (thread-local).
 */
#ifndef RAFTSIM_H
#define RAFTSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAFT_SIM_ABI_VERSION 2
#define RAFT_MAX_NODES 9
#define RAFT_MAX_INBOX 16

/* :state values of the node map (core.clj:33,70,76,81,87); 3 is the `:follwer` typo of
 * candidate->follower (core.clj:76), a distinct fourth value. */
enum raft_role { RAFT_FOLLOWER = 0, RAFT_CANDIDATE = 1, RAFT_LEADER = 2, RAFT_FOLLWER = 3 };

/* :type values (server.clj:8-12 for requests, core.clj:95,109 for replies). */
enum raft_msg_type {
  RAFT_MSG_REQUEST_VOTE = 1,
  RAFT_MSG_APPEND_ENTRIES = 2,
  RAFT_MSG_CLIENT_SET = 3,
  RAFT_MSG_VOTE_RESPONSE = 4,
  RAFT_MSG_APPEND_RESPONSE = 5
};

/* Exceptions that end a node's `loop` (core.clj:202-203), SIM_SPEC D8. */
enum raft_fault {
  RAFT_RUNNING = 0,
  RAFT_FAULT_IOOBE = 1,    /* nth past the end: val-at log.clj:23 */
  RAFT_FAULT_NPE = 2,      /* (dec nil): core.clj:146 */
  RAFT_FAULT_CCE = 3,      /* subvec of a LazySeq: log.clj:53 */
  RAFT_FAULT_OVERFLOW = 4  /* log capacity exceeded (simulator limit) */
};

/* Bug-injection / correct-protocol flags (SIM_SPEC §4, §8). */
enum raft_variant {
  RAFT_VARIANT_VOTE_NO_LOG_CHECK = 1, /* drop core.clj:96,99 (with SPEC: drop the up-to-date check) */
  RAFT_VARIANT_SPEC = 2               /* F4 Spec-Raft control: Raft Figure 2 rules (SIM_SPEC §8) */
};

/* How clusters are packed onto waves before each launch. Clusters are independent and Philox is
 * keyed by the global cluster id, so every packing gives bit-identical results; it only decides
 * which clusters share a wave, i.e. how many of a wave's ticks are active. */
enum raft_schedule {
  RAFT_SCHED_ALIGNED = 0, /* regroup clusters by their next event tick before every launch */
  RAFT_SCHED_FIXED = 1    /* cluster c always on wave c / floor(64/N) */
};

/* Replaces `-main`'s argv (core.clj:197-200), the hard-coded timeouts (core.clj:173-174) and the
 * chan buffer sizes (server.clj:37, client.clj:18). Defaults: raft_sim_default_config().
 * Limits (-EINVAL otherwise): cluster_offset + n_clusters <= 2^32 (global ids key Philox), and
 * nodes^2 * n_clusters < 2^31 (per-peer rows are indexed in 32 bits). */
typedef struct raft_sim_config {
  uint32_t n_clusters;     /* clusters simulated by this handle */
  uint32_t cluster_offset; /* global id of the first one (keys Philox: shard-invariant) */
  uint32_t nodes;          /* N, 2..9 */
  uint32_t log_cap;        /* L, max entries per log */
  uint32_t arena_cap;      /* A >= 2L log-arena slots per node; 0 -> 4L */
  uint32_t inbox_cap;      /* Q per queue, 1..16 */
  uint64_t seed;
  uint32_t hb, el_base, el_span;       /* 3000 / 5000 / 5000 ticks */
  uint32_t drop_ppm, dup_ppm, dmin, dmax;
  uint32_t part_ppm, part_epoch;
  uint32_t client_ppm;
  uint32_t variant_flags;
  int32_t device;            /* HIP device ordinal */
  uint32_t ticks_per_launch; /* ticks fused into one kernel launch; 0 -> default */
  uint32_t commit_stream_cap; /* per-node ring of committed :val's (log.clj:69-76); 0 = off */
  uint32_t trace_cap;         /* per-node ring of `wait` events (core.clj:182-186); 0 = off */
  uint32_t trace_entry_cap;   /* per-node ring of the :entries those events carried */
  uint32_t schedule;          /* cluster->wave packing, enum raft_schedule (results identical) */
  /* Client traffic (SIM_SPEC §4 P0, D9/D14/D15): client-sets arrive at client_ppm per tick during
   * bursts of client_burst ticks at the start of every client_period ticks (period 0: always on),
   * and a client follows up to client_redirects redirect-client hops (server.clj:62-63) towards the
   * :leader-id before it abandons the command (0: a redirect ends the command). */
  uint32_t client_period;
  uint32_t client_burst;      /* 1..client_period when client_period > 0 */
  uint32_t client_redirects;  /* 0..16 */
  /* Multi-GPU inside one handle: the clusters are split into n_devices contiguous shards
   * [n*d/G, n*(d+1)/G) (the split raftsim.dist.shard uses), shard d on HIP device
   * (device + d) mod the visible device count, one stream each; steps run on all shards at
   * once and raft_sim_read_counters reduces them (SUM; MIN first violation; MAX payload).
   * 0 means 1. Results are identical for every G (Philox is keyed by the global cluster id). */
  int32_t n_devices;
} raft_sim_config_t;

/* Canonical node record: the node map of init-node (core.clj:31-38) plus the log atom
 * (log.clj:33-34) and simulator bookkeeping. next/match are indexed by id-1; 0 where absent. */
typedef struct raft_node {
  uint8_t role, voted_for, leader_id, fault;
  uint8_t entries_is_seq, ls_present;
  uint16_t votes;   /* bit i: id i in the :votes set */
  uint16_t ls_keys; /* bit i: peer i has :next-index and :match-index keys */
  uint16_t reserved0;
  uint32_t current_term, commit_index, log_len, deadline;
  int32_t next_index[RAFT_MAX_NODES];
  int32_t match_index[RAFT_MAX_NODES];
  uint32_t last_led_term;
  uint32_t arena_base, arena_frontier;
  uint32_t req_count, res_count; /* read-only: set through raft_sim_write_queue */
  uint32_t commit_count;         /* lines apply-entries! has written to node_<id>.log so far */
  uint64_t trace_hash;
} raft_node_t;

/* One queued message (SIM_SPEC §3): hdr = type | src<<3 | flag<<7 | epresent<<8 | pcnt<<16. */
typedef struct raft_msg {
  uint32_t arrival, hdr, term, a, b, eterm, eval, poff;
} raft_msg_t;

typedef struct raft_entry {
  uint32_t term, val;
} raft_entry_t;

/* Per-cluster record: the leader-completeness checker's high-water mark (SIM_SPEC §4 P4) and the
 * client-set injection cursor (next injection tick, draws consumed; SIM_SPEC §4 P0). */
typedef struct raft_cluster {
  uint32_t hwm_index, hwm_term, hwm_val;
  uint32_t client_next, client_count;
  uint32_t reserved[3];
} raft_cluster_t;

/* F3: one iteration of `wait` as it prints (core.clj:182-186): the node map before the handler
 * (`; Node` / `(prn node)`) and the message alts!! returned (`; Message` / `(prn message)`). A
 * timeout (`nil`) has an all-zero msg. An append-entries' :entries are the msg.hdr>>16 entries of
 * the node's trace-entry ring starting at entries_seq (SIM_SPEC §7). */
typedef struct raft_trace_event {
  uint32_t tick;
  uint32_t seq;            /* this node's event number, from 0 */
  raft_msg_t msg;          /* as queued: arrival, hdr, term, a, b, eterm, eval, poff */
  uint8_t role, voted_for, leader_id, ls_present;
  uint16_t votes, ls_keys;
  uint32_t current_term;
  int32_t next_index[RAFT_MAX_NODES];
  int32_t match_index[RAFT_MAX_NODES];
  uint32_t entries_seq;
} raft_trace_event_t;

enum raft_counter {
  RAFT_CTR_EV_RV = 0, RAFT_CTR_EV_AE, RAFT_CTR_EV_CS, RAFT_CTR_EV_VR, RAFT_CTR_EV_AR,
  RAFT_CTR_EV_TIMEOUT, RAFT_CTR_EV_HEARTBEAT, RAFT_CTR_LEADERS, RAFT_CTR_SENT,
  RAFT_CTR_DELIVERED, RAFT_CTR_DROPPED, RAFT_CTR_PARTITIONED, RAFT_CTR_DUPLICATED,
  RAFT_CTR_OVERFLOW, RAFT_CTR_TO_HALTED, RAFT_CTR_CLIENT_INJECTED, RAFT_CTR_HALT_IOOBE,
  RAFT_CTR_HALT_NPE, RAFT_CTR_HALT_CCE, RAFT_CTR_HALT_OVERFLOW, RAFT_CTR_ENTRIES_APPENDED,
  RAFT_CTR_ENTRIES_APPLIED, RAFT_CTR_PAYLOAD_EVICTED, RAFT_CTR_VIOL_ELECTION,
  RAFT_CTR_VIOL_LOG, RAFT_CTR_VIOL_COMPLETE,
  RAFT_CTR_REDIRECTS,        /* client-sets re-sent along a redirect-client (server.clj:62-63) */
  RAFT_CTR_CLIENT_ABANDONED, /* client-sets a non-leader received with no redirect hop left */
  RAFT_CTR_COUNT
};

typedef struct raft_counters {
  uint64_t node_ticks;
  uint64_t first_violation_tick; /* UINT64_MAX when none */
  uint64_t c[RAFT_CTR_COUNT];    /* sums */
  uint64_t payload_max;          /* most :entries any append-entries carried (a maximum) */
} raft_counters_t;

typedef struct raft_sim raft_sim_t;

int raft_sim_abi_version(void);
void raft_sim_default_config(raft_sim_config_t* cfg);

/* Replaces raft-system + component/start (core.clj:23-29,201): allocates every cluster's nodes in
 * HBM in the init-node state (core.clj:31-38) with empty logs (log.clj:33-34). */
int raft_sim_create(const raft_sim_config_t* cfg, raft_sim_t** out);

/* Replaces the `(loop [node ...] (recur (wait system node)))` of -main (core.clj:202-203) for every
 * node of every cluster: advances all clusters by n_ticks (synchronous). A HIP failure part-way
 * through a step leaves the state between ticks the handle cannot name, so the handle is then
 * poisoned: every later step returns -EIO. */
int raft_sim_step(raft_sim_t* sim, uint32_t n_ticks);

/* raft_sim_step without the wait: enqueues the launches for n_ticks on every shard's stream and
 * returns. Reads, digests and the next step are stream-ordered after it; raft_sim_sync waits for
 * everything enqueued and makes raft_sim_last_step_timing cover those launches. Many steps
 * queued between syncs pay no host round trip per step. */
int raft_sim_step_async(raft_sim_t* sim, uint32_t n_ticks);
int raft_sim_sync(raft_sim_t* sim);

/* Ticks simulated so far (the next tick to run). */
uint64_t raft_sim_tick(const raft_sim_t* sim);

/* Resume: set the next tick to run, for state restored through the write_* calls below (deadlines
 * and arrivals are absolute ticks). Steps are refused (-ERANGE) once tick + n_ticks plus the
 * longest timer or delay (max(hb, el_base + el_span, dmax)) could reach 2^32 - 1, the "never"
 * marker, so no deadline or arrival can wrap. */
int raft_sim_set_tick(raft_sim_t* sim, uint64_t tick);

/* Replaces `(prn node)` of wait (core.clj:182-183): canonical records, N per cluster. */
int raft_sim_read_nodes(raft_sim_t* sim, uint32_t c0, uint32_t nc, raft_node_t* out);
int raft_sim_write_nodes(raft_sim_t* sim, uint32_t c0, uint32_t nc, const raft_node_t* in);

/* The req-chan (which=0, server.clj:37) or resp-chan (which=1, client.clj:18) contents of node
 * `node_id` (1..N), head first. read returns the count (>= 0) or a negative errno. */
int raft_sim_read_queue(raft_sim_t* sim, uint32_t cluster, uint32_t node_id, uint32_t which,
                        raft_msg_t* out, uint32_t cap);
int raft_sim_write_queue(raft_sim_t* sim, uint32_t cluster, uint32_t node_id, uint32_t which,
                         const raft_msg_t* in, uint32_t count);

/* The raw log arena (arena_cap entries) behind the Log atom's :entries (log.clj:33-34). */
int raft_sim_read_arena(raft_sim_t* sim, uint32_t cluster, uint32_t node_id, raft_entry_t* out,
                        uint32_t cap);
int raft_sim_write_arena(raft_sim_t* sim, uint32_t cluster, uint32_t node_id,
                         const raft_entry_t* in, uint32_t count);

/* F2: the newest min(count, commit_stream_cap, cap) values apply-entries! wrote to node_<id>.log
 * (log.clj:16-18,69-76), oldest first; returns how many were copied. write_commit_stream stores
 * `count` values as the newest ones ending at the node record's commit_count. */
int raft_sim_read_commit_stream(raft_sim_t* sim, uint32_t cluster, uint32_t node_id,
                                uint32_t* out, uint32_t cap);
int raft_sim_write_commit_stream(raft_sim_t* sim, uint32_t cluster, uint32_t node_id,
                                 const uint32_t* in, uint32_t count);

/* F3: the retained events of node `node_id` with seq >= first_seq, oldest first (the newest
 * trace_cap are kept); returns how many were copied. read_trace_entries copies the entries with
 * ring index first, first+1, ... (at most cap, up to the newest) and returns how many; -ERANGE if
 * entry `first` has already been overwritten (only the newest trace_entry_cap are kept). */
int raft_sim_read_trace(raft_sim_t* sim, uint32_t cluster, uint32_t node_id, uint32_t first_seq,
                        raft_trace_event_t* out, uint32_t cap);
int raft_sim_read_trace_entries(raft_sim_t* sim, uint32_t cluster, uint32_t node_id,
                                uint32_t first, raft_entry_t* out, uint32_t cap);

int raft_sim_read_clusters(raft_sim_t* sim, uint32_t c0, uint32_t nc, raft_cluster_t* out);
int raft_sim_write_clusters(raft_sim_t* sim, uint32_t c0, uint32_t nc, const raft_cluster_t* in);

/* Counters of this handle's clusters (no reference counterpart; see SIM_SPEC §4). */
int raft_sim_read_counters(raft_sim_t* sim, raft_counters_t* out);

/* Per-cluster FNV-1a-64 digest of the canonical state (SIM_SPEC §6). */
int raft_sim_digest(raft_sim_t* sim, uint32_t c0, uint32_t nc, uint64_t* out);

/* Average device time of the tick-kernel launches of the last raft_sim_step (or of the
 * raft_sim_step_async calls since the previous sync, once raft_sim_sync returned) alone, and the
 * launch count; for bench.py's roofline. An event pair in a launch's dispatch packet times it:
 * every general-kernel launch, and of the steady-path launches (~0.025 ms at config 2) only one
 * that comes first after a sync, since such a pair costs ~6 us per launch on MI355X; with
 * RAFTSIM_LAUNCH_EVENTS=1 in the environment at create every launch is timed. */
int raft_sim_last_step_timing(raft_sim_t* sim, double* avg_kernel_ms, uint32_t* launches);

/* Device time of everything the last raft_sim_step (or every raft_sim_step_async since the
 * previous sync, once raft_sim_sync returned) enqueued, from a HIP event before its first launch
 * to one after its last, on each shard's stream; the maximum over shards. Host time spent between
 * steps is not in it; gaps between the queued launches are. For bench.py's throughput. */
int raft_sim_last_span(raft_sim_t* sim, double* span_ms);

void raft_sim_destroy(raft_sim_t* sim);
const char* raft_sim_last_error(void);

/* ---- Violation records (no reference counterpart, and none in the oracle library) ----------
 * The reference has no checker; the counters above say how often and how early the checker
 * (SIM_SPEC §4 P4) fired in the whole handle. These calls say where: the library keeps, per
 * cluster, the earliest tick at which a violation was counted for it and its count of each kind.
 * Every increment of a RAFT_CTR_VIOL_* counter is one increment of one cluster's record with the
 * same tick, so per kind the records sum to the counter and their earliest first_tick is
 * first_violation_tick (until raft_viol_clear, which leaves the counters alone). The records are
 * a log, not state (SIM_SPEC §6): outside the digest, untouched by raft_sim_write_* and
 * raft_sim_set_tick, cleared only by raft_sim_create and raft_viol_clear. */
enum raft_viol_kind { RAFT_VIOL_ELECTION = 1, RAFT_VIOL_LOG = 2, RAFT_VIOL_COMPLETE = 4 };

typedef struct raft_violation {
  uint32_t cluster;    /* handle-local index, as raft_sim_read_nodes takes it */
  uint32_t first_tick; /* earliest tick at which any violation was counted for the cluster */
  uint32_t count[3];   /* election safety, log matching, leader completeness */
  uint32_t kinds;      /* raft_viol_kind bits of the nonzero counts */
} raft_violation_t;

/* The clusters with a nonzero count of a kind in kinds_mask (raft_viol_kind bits, 1..7) whose
 * first_tick lies in [t_lo, t_hi), in ascending cluster order: the first min(total, cap) of them
 * are written to out (which may be null when cap is 0: count only). Returns the number of matching
 * clusters, which may exceed cap, or a negative errno (-EINVAL: kinds_mask 0 or above 7, t_lo >
 * t_hi, null out with cap > 0; -EIO: a HIP error, or a handle poisoned by a failed step). The
 * selection runs on the device, stream-ordered after everything enqueued: valid after
 * raft_sim_step_async, which it waits for. */
int64_t raft_viol_read(raft_sim_t* sim, uint32_t kinds_mask, uint64_t t_lo, uint64_t t_hi,
                       raft_violation_t* out, uint32_t cap);

/* Forget every cluster's record (counters, state and digests are unchanged). */
int raft_viol_clear(raft_sim_t* sim);

/* ---- State census (no reference counterpart, none in the oracle) ---------------------------
 * What state the clusters are in right now, answered on the device from the words
 * raft_sim_read_nodes would decode, without copying them: a census of the whole handle, and the
 * selection of the clusters in given state classes. A class is a predicate over a cluster's N node
 * records (SIM_SPEC.md, "Derived, not state"). With live(k) = (fault == 0), leader(k) = live and
 * role == RAFT_LEADER, nl the number of leaders and quorum = (N+1)>>1, or N/2+1 under
 * RAFT_VARIANT_SPEC: */
enum raft_cluster_class {
  RAFT_CLS_NO_LEADER = 1,          /* nl == 0 */
  RAFT_CLS_ONE_LEADER = 2,         /* nl == 1 */
  RAFT_CLS_MULTI_LEADER = 4,       /* nl >= 2 */
  RAFT_CLS_HALTED = 8,             /* some node has fault != 0 */
  RAFT_CLS_NO_QUORUM = 16,         /* live nodes < quorum */
  RAFT_CLS_SAME_TERM_LEADERS = 32, /* two leaders with equal current_term */
  RAFT_CLS_LOG_FULL = 64,          /* some node (live or halted) has log_len == log_cap */
  RAFT_CLS_CANDIDATE = 128,        /* some live node has role == RAFT_CANDIDATE */
  RAFT_CLS_SETTLED = 256           /* nl == 1 and every live node has that leader's id as
                                      leader_id and its term as current_term */
};
#define RAFT_CLS_ALL 511

typedef struct raft_census {            /* every field uint64_t */
  uint64_t clusters, nodes;
  uint64_t by_class[16];                /* clusters with class bit b set; b >= 9: 0 */
  uint64_t leaders_hist[RAFT_MAX_NODES + 1]; /* clusters with exactly i live leaders */
  uint64_t live_hist[RAFT_MAX_NODES + 1];    /* clusters with exactly i live nodes */
  uint64_t role_nodes[4];               /* live nodes by role (enum raft_role) */
  uint64_t fault_nodes[5];              /* all nodes by fault code (enum raft_fault) */
  uint64_t term_min, term_max, term_sum;       /* over all nodes */
  uint64_t commit_max, commit_sum, len_max, len_sum;
  uint64_t req_queued, res_queued;      /* sums of req_count / res_count */
  uint64_t hwm_max, hwm_sum;            /* the checker's hwm_index per cluster */
} raft_census_t;

typedef struct raft_cluster_state {     /* 32 bytes */
  uint32_t cluster;                     /* handle-local, as raft_sim_read_nodes takes it */
  uint32_t classes;                     /* raft_cluster_class bits */
  uint16_t leaders, halted;             /* bit i: id i is a live leader / is halted (as votes) */
  uint32_t term_max, term_min, commit_max, len_max; /* over all N nodes */
  uint32_t queued;                      /* sum of req_count + res_count */
} raft_cluster_state_t;

/* The census of every cluster of the handle, reduced over its devices (sums; MIN of term_min; MAX
 * of the *_max fields). Both calls run on the device, stream-ordered after everything enqueued
 * (valid after raft_sim_step_async, which they wait for), read the state only (a steady
 * certificate stays), and give bitwise the same answer for the same state. -EINVAL: null
 * argument; -EIO: a HIP error, or a handle poisoned by a failed step. */
int raft_census_read(raft_sim_t* sim, raft_census_t* out);

/* The clusters whose class word `classes` satisfies (any_mask == 0 || classes & any_mask) &&
 * (classes & all_mask) == all_mask && (classes & none_mask) == 0, in ascending cluster order: the
 * first min(total, cap) of them are written to out (which may be null when cap is 0: count only).
 * Returns the number of matching clusters, which may exceed cap, or a negative errno (-EINVAL: a
 * mask above RAFT_CLS_ALL, all_mask & none_mask nonzero, null out with cap > 0, null sim: refused
 * before any device is touched; -EIO as above). */
int64_t raft_census_select(raft_sim_t* sim, uint32_t any_mask, uint32_t all_mask,
                           uint32_t none_mask, raft_cluster_state_t* out, uint32_t cap);

/* ---- Log audit (no reference counterpart, none in the oracle) -------------------------------
 * Whether the nodes' logs agree right now, answered on the device from the log contents as they
 * stand (the entries raft_sim_read_arena would copy, every node of every cluster), without copying
 * them: State Machine Safety and Log Matching read off the state, not counted when they happened.
 * Node k's log is its log_len entries, entry p the (term, val) at arena slot (arena_base + p) mod
 * arena_cap; halted nodes count. For a pair i < j, m = min(len_i, len_j) and d_ij is the smallest
 * p < m at which the two entries differ in term or val, or m (SIM_SPEC.md, "Derived, not state"). */
enum raft_audit_class {
  RAFT_AUD_DIVERGED = 1,        /* some pair has d_ij < m */
  RAFT_AUD_COMMIT_DIVERGED = 2, /* some pair has d_ij < m and d_ij < min(commit_i, commit_j) */
  RAFT_AUD_MATCH_BROKEN = 4,    /* some pair has a p, d_ij <= p < m, with term_i[p] == term_j[p] */
  RAFT_AUD_TERM_ORDER = 8,      /* some node has term[p] > term[p + 1], p + 1 < len */
  RAFT_AUD_IDENTICAL = 16       /* no pair diverges and all N lengths are equal */
};
#define RAFT_AUD_ALL 31

typedef struct raft_audit {             /* every field uint64_t */
  uint64_t clusters;
  uint64_t by_class[8];                 /* clusters with class bit b set; b >= 5: 0 */
  uint64_t entries;                     /* sum of log_len over all nodes */
  uint64_t agree_sum, agree_min, agree_max; /* agree_len over the clusters */
  uint64_t diverged_nodes, commit_diverged_nodes; /* popcounts of the records' masks, summed */
  uint64_t diverge_index_min, commit_diverge_index_min; /* UINT64_MAX when no cluster has one */
} raft_audit_t;

typedef struct raft_audit_record {      /* 32 bytes */
  uint32_t cluster;                     /* handle-local, as raft_sim_read_nodes takes it */
  uint32_t classes;                     /* raft_audit_class bits */
  uint32_t agree_len;                   /* the common prefix of all N logs: min over pairs of d_ij */
  uint32_t diverge_index;               /* min d_ij over diverging pairs; UINT32_MAX: none */
  uint32_t commit_diverge_index;        /* min d_ij over the pairs of bit 2; UINT32_MAX: none */
  uint32_t order_index;                 /* the smallest p of bit 8 in any node; UINT32_MAX: none */
  uint16_t diverged, commit_diverged;   /* bit i: id i is in a pair of bit 1 / bit 2 (as votes) */
  uint32_t len_min;                     /* the shortest log */
} raft_audit_record_t;

/* The audit of every cluster of the handle, reduced over its devices (sums; MIN of agree_min and
 * the *_index_min fields; MAX of agree_max). Both calls run on the device, stream-ordered after
 * everything enqueued (valid after raft_sim_step_async, which they wait for), read the state only
 * (digest, counters, violation records and a steady certificate stay), and give bitwise the same
 * answer for the same state. The per-cluster records a query computes stay valid until the next
 * raft_sim_step, raft_sim_step_async, raft_sim_write_nodes, raft_sim_write_arena or
 * raft_sim_write_clusters: queries in between read the records, not the logs again. -EINVAL: null
 * argument; -EIO: a HIP error, or a handle poisoned by a failed step. */
int raft_audit_read(raft_sim_t* sim, raft_audit_t* out);

/* The clusters whose class word satisfies the predicate of raft_census_select over
 * raft_audit_class bits, in ascending cluster order: the first min(total, cap) records are written
 * to out (which may be null when cap is 0: count only). Returns the number of matching clusters,
 * which may exceed cap, or a negative errno (-EINVAL: a mask above RAFT_AUD_ALL, all_mask &
 * none_mask nonzero, null out with cap > 0, null sim: refused before any device is touched; -EIO
 * as above). */
int64_t raft_audit_select(raft_sim_t* sim, uint32_t any_mask, uint32_t all_mask,
                          uint32_t none_mask, raft_audit_record_t* out, uint32_t cap);

/* ---- Cluster packs (no reference counterpart, none in the oracle) ---------------------------
 * The full canonical state of an arbitrary list of clusters, packed on the device into one
 * contiguous buffer of fixed-size records and copied once per device: what the per-node reads
 * above return one synchronous copy at a time, for the clusters a selection found. A record is the
 * parts asked for, in bit order, each starting on a 16-byte boundary (padding bytes are zero);
 * parts not asked for take no room. The counts of a node's queues, log and commit stream are in
 * its node record (req_count, res_count, log_len, commit_count), so RAFT_GATHER_NODES belongs in
 * every pack that is to be decoded. A pack is a view of the state the digest covers, not state
 * (SIM_SPEC.md §6): one cluster's record holds everything the raft_sim_write_* calls need to
 * restore it in another handle. */
enum raft_gather_part {
  RAFT_GATHER_CLUSTER = 1,  /* raft_cluster_t, reserved words zero (as read_clusters returns it) */
  RAFT_GATHER_NODES   = 2,  /* N raft_node_t, byte-identical to what read_nodes returns */
  RAFT_GATHER_QUEUES  = 4,  /* per node REQ then RES: inbox_cap raft_msg_t, head first, zero past count */
  RAFT_GATHER_LOGS    = 8,  /* per node log_cap raft_entry_t: entry p from slot (arena_base+p) mod A, zero past log_len */
  RAFT_GATHER_ARENAS  = 16, /* per node the raw arena, arena_cap raft_entry_t (what read_arena copies) */
  RAFT_GATHER_STREAMS = 32  /* per node commit_stream_cap u32: newest min(commit_count, cap), oldest first, zero past */
};
#define RAFT_GATHER_ALL 63

typedef struct raft_gather_layout {   /* every field uint64_t */
  uint64_t stride;        /* bytes per cluster, a multiple of 16 */
  uint64_t off[6];        /* byte offset of part bit b in a cluster's record; UINT64_MAX: not asked for */
  uint64_t size[6];       /* its unpadded size in bytes (0: not asked for) */
} raft_gather_layout_t;

/* The layout of a record of `parts` (raft_gather_part bits, 1..RAFT_GATHER_ALL) in this handle: a
 * function of its config and `parts` alone. RAFT_GATHER_STREAMS has size 0 when commit_stream_cap
 * is 0; a log_len above log_cap is clamped to it in RAFT_GATHER_LOGS. -EINVAL: null argument,
 * parts 0 or above RAFT_GATHER_ALL. Touches no device. */
int raft_gather_layout(raft_sim_t* sim, uint32_t parts, raft_gather_layout_t* out);

/* Record i of out is cluster clusters[i] (handle-local indices, in any order, with duplicates,
 * across devices); returns n * stride, the bytes written. -EINVAL: null sim, parts 0 or above
 * RAFT_GATHER_ALL, null clusters or out with n > 0, an index >= n_clusters (the message names the
 * first offending position); -ERANGE: cap_bytes < n * stride; all refused before any device is
 * touched. -EIO: a HIP error, or a handle poisoned by a failed step. n == 0 returns 0 and launches
 * nothing. The packing runs on the device, stream-ordered after everything enqueued (valid after
 * raft_sim_step_async, which it waits for), and reads the state only: digest, counters, violation
 * records, the audit's records and a steady certificate stay, and the next step runs as it would
 * have. Device scratch is bounded (64 MiB per device); larger requests run in chunks. */
int64_t raft_gather_read(raft_sim_t* sim, const uint32_t* clusters, uint32_t n, uint32_t parts,
                         void* out, uint64_t cap_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RAFTSIM_H */
