// node_codec.hpp — how a node's words of a hot block (device.hpp: field-major, field f of node k at
// word HOT_CW + f * N + k) map to its canonical record raft_node_t (include/raftsim.h), stated once
// and word by word, in both directions:
//   node_word   hot block -> record (raft_sim_read_nodes, gather_kernel), resolving an owed timer draw
//   hot_field   record -> hot block (raft_sim_write_nodes, scatter_kernel), FL_DRAW clear
//   ring_words  what a queue ring contributes to the hot block (raft_sim_write_queue, scatter_kernel)
//   hot_clone   hot block -> hot block (clone_kernel): hot_field of node_word without the record
//   hot_restart hot block -> hot block (restart_kernel, restart_where_kernel): a node started again
// Host and device: compiles for the CPU alone too (tests/test_node_codec_host.py checks the first
// three against a by-member-name statement of the same mapping, tests/test_clone_host.py the fourth
// against the first two, tests/test_restart_host.py the fifth against a restatement on the record).
#pragma once
#include <stddef.h>

#include "device.hpp"

namespace rs {

// A raft_node_t as NODE_WORDS little-endian 32-bit words: the word numbers of its members.
constexpr uint32_t NODE_WORDS = sizeof(raft_node_t) / 4;
#define NW_OF(member) ((uint32_t)(offsetof(raft_node_t, member) / 4))
constexpr uint32_t NW_ROLE = NW_OF(role),        // bytes role, voted_for, leader_id, fault
    NW_SEQ = NW_OF(entries_is_seq),              // bytes entries_is_seq, ls_present, then votes
    NW_KEYS = NW_OF(ls_keys),                    // ls_keys, then reserved0
    NW_TERM = NW_OF(current_term), NW_COMMIT = NW_OF(commit_index), NW_LEN = NW_OF(log_len),
    NW_DEADLINE = NW_OF(deadline), NW_NEXT = NW_OF(next_index), NW_MATCH = NW_OF(match_index),
    NW_LED = NW_OF(last_led_term), NW_ABASE = NW_OF(arena_base), NW_AFRONT = NW_OF(arena_frontier),
    NW_REQ_COUNT = NW_OF(req_count), NW_RES_COUNT = NW_OF(res_count),
    NW_COMMIT_COUNT = NW_OF(commit_count), NW_TRACE = NW_OF(trace_hash);   // low word, then high
#undef NW_OF
constexpr uint32_t MSG_WORDS = sizeof(raft_msg_t) / 4;
static_assert(sizeof(raft_node_t) == 136 && sizeof(raft_msg_t) == 32 && sizeof(raft_entry_t) == 8 &&
                  sizeof(raft_cluster_t) == 32,
              "the record sizes the pack's layout is made of");
static_assert(offsetof(raft_node_t, role) == 0 && offsetof(raft_node_t, voted_for) == 1 &&
                  offsetof(raft_node_t, leader_id) == 2 && offsetof(raft_node_t, fault) == 3 &&
                  offsetof(raft_node_t, entries_is_seq) == 4 &&
                  offsetof(raft_node_t, ls_present) == 5 && offsetof(raft_node_t, votes) == 6 &&
                  offsetof(raft_node_t, ls_keys) == 8 && offsetof(raft_node_t, reserved0) == 10 &&
                  NW_TERM == NW_KEYS + 1 && NW_MATCH == NW_NEXT + RAFT_MAX_NODES &&
                  NW_LED == NW_MATCH + RAFT_MAX_NODES && NW_TRACE + 2 == NODE_WORDS &&
                  offsetof(raft_msg_t, arrival) == 0,
              "the bytes inside words 0-2, the two index rows back to back, the trace hash last");

// The fields of a node in a hot block; the queue words among them are not the node record's
// (read-only req_count / res_count apart): raft_sim_write_queue and the tick kernels own them.
__host__ __device__ constexpr uint32_t hot_fields(uint32_t N) { return hf_led(N) + 1; }
__host__ __device__ constexpr bool hf_is_queue(uint32_t f) {
  return f >= HF_QMETA && f <= HF_RES_TAIL;
}
static_assert(HF_RES_TAIL - HF_QMETA == 4 && HF_REQ_ARR > HF_QMETA && HF_RES_ARR > HF_QMETA &&
                  HF_REQ_TAIL > HF_QMETA,
              "the five queue words are one run of fields");

// What exact_deadline needs besides the node: the election timer's config and the Philox keys.
struct DrawKeys {
  uint32_t el_base, el_span, key0, key1;
};

// Word w (0..NODE_WORDS - 1) of the record of node k (id k + 1) of global cluster g. h: the node's
// first hot word (field f at h[f * N]); cc: its commit_count. An owed timer draw (FL_DRAW) is
// resolved as every reader of the state resolves it; padding and reserved bytes are zero.
__host__ __device__ __forceinline__ uint32_t node_word(const uint32_t* h, uint32_t N, uint32_t w,
                                                       uint32_t cc, uint32_t g, uint32_t k,
                                                       const DrawKeys& dk) {
  if (w >= NW_NEXT && w < NW_NEXT + 2 * RAFT_MAX_NODES) {   // next_index, then match_index
    const uint32_t row = w >= NW_MATCH, p = w - NW_NEXT - row * RAFT_MAX_NODES;
    return p < N ? h[(HF_NEXT + row * N + p) * N] : 0u;
  }
  switch (w) {
    case NW_ROLE: {
      const uint32_t fl = h[HF_FLAGS * N];
      return fl_role(fl) | fl_vf(fl) << 8 | fl_lid(fl) << 16 | fl_fault(fl) << 24;
    }
    case NW_SEQ: {
      const uint32_t fl = h[HF_FLAGS * N];
      return fl_seq(fl) | fl_lsp(fl) << 8 | (h[HF_MASKS * N] & 0xFFFFu) << 16;
    }
    case NW_KEYS: return h[HF_MASKS * N] >> 16;             // reserved0 is zero
    case NW_TERM: return h[HF_TERM * N];
    case NW_COMMIT: return h[HF_COMMIT * N];
    case NW_LEN: return h[HF_LEN * N];
    case NW_DEADLINE: {
      const uint32_t dl = h[HF_DEADLINE * N];
      return h[HF_FLAGS * N] & FL_DRAW
                 ? exact_deadline(g, k + 1, dl, dk.el_base, dk.el_span, dk.key0, dk.key1)
                 : dl;
    }
    case NW_LED: return h[hf_led(N) * N];
    case NW_ABASE: return h[hf_abase(N) * N];
    case NW_AFRONT: return h[hf_afront(N) * N];
    case NW_REQ_COUNT: return qm_req_cnt(h[HF_QMETA * N]);
    case NW_RES_COUNT: return qm_res_cnt(h[HF_QMETA * N]);
    case NW_COMMIT_COUNT: return cc;
    case NW_TRACE: return h[HF_TRACE_LO * N];
    case NW_TRACE + 1: return h[HF_TRACE_HI * N];
    default: return 0u;                                     // the padding before trace_hash
  }
}

// Field f (< hot_fields(N), not hf_is_queue) of a node from its record's words nw, FL_DRAW clear:
// a record's deadline is the exact draw. Peer rows past N, req_count, res_count and commit_count
// are not the hot block's.
__host__ __device__ __forceinline__ uint32_t hot_field(const uint32_t* nw, uint32_t N, uint32_t f) {
  if (f >= HF_NEXT && f < HF_NEXT + 2 * N) {                // next_index, then match_index
    const uint32_t row = f >= HF_NEXT + N, p = f - HF_NEXT - row * N;
    return nw[NW_NEXT + row * RAFT_MAX_NODES + p];
  }
  if (f == hf_abase(N)) return nw[NW_ABASE];
  if (f == hf_afront(N)) return nw[NW_AFRONT];
  if (f == hf_led(N)) return nw[NW_LED];
  switch (f) {
    case HF_DEADLINE: return nw[NW_DEADLINE];
    case HF_TRACE_LO: return nw[NW_TRACE];
    case HF_TRACE_HI: return nw[NW_TRACE + 1];
    case HF_FLAGS: {
      const uint32_t a = nw[NW_ROLE], b = nw[NW_SEQ];
      return pack_flags(a & 3, (a >> 8) & 15, (a >> 16) & 15, (a >> 24) & 7, b & 1, (b >> 8) & 1);
    }
    case HF_MASKS: return nw[NW_SEQ] >> 16 | nw[NW_KEYS] << 16;   // votes | ls_keys << 16
    case HF_TERM: return nw[NW_TERM];
    case HF_COMMIT: return nw[NW_COMMIT];
    case HF_LEN: return nw[NW_LEN];
    default: return 0u;
  }
}

// Field f (< hot_fields(N), not hf_is_queue) of a node as hot_field(nw, N, f) gives it for the record
// nw[w] = node_word(h, N, w, cc, g, k, dk), without the record: the deadline is the exact draw, the
// flags keep their six fields (FL_DRAW and the unused bits above it are no field of a record), and
// every other field is the source's word (votes and ls_keys are the two halves of HF_MASKS; the peer
// rows are N fields each on both sides).
__host__ __device__ __forceinline__ uint32_t hot_clone(const uint32_t* h, uint32_t N, uint32_t f,
                                                       uint32_t g, uint32_t k, const DrawKeys& dk) {
  const uint32_t v = h[f * N];
  if (f == HF_DEADLINE)
    return h[HF_FLAGS * N] & FL_DRAW
               ? exact_deadline(g, k + 1, v, dk.el_base, dk.el_span, dk.key0, dk.key1)
               : v;
  if (f == HF_FLAGS) return v & (FL_ROLE | FL_VF | FL_LID | FL_FAULT | FL_SEQ | FL_LSP);
  return v;
}

// What a ring of `count` messages contributes to its node's hot words, as raft_sim_write_queue
// leaves them: its half (mask) of HF_QMETA with head 0, the first message's arrival (INF when
// empty) and the last one's (0 when empty). msgs: the messages in order from the head, MSG_WORDS
// words each, read only below count.
struct RingWords {
  uint32_t mask, qmeta, arr, tail;
};
// (first, last: the arrivals of the first and the last message, looked at only when count > 0)
__host__ __device__ __forceinline__ RingWords ring_words(uint32_t which, uint32_t count,
                                                         uint32_t first, uint32_t last) {
  return {which ? QM_RES : QM_REQ, which ? pack_qmeta(0, 0, 0, count) : pack_qmeta(0, count, 0, 0),
          count ? first : INF, count ? last : 0u};
}
__host__ __device__ __forceinline__ RingWords ring_words(uint32_t which, uint32_t count,
                                                         const uint32_t* msgs) {
  return ring_words(which, count, count ? msgs[0] : INF,
                    count ? msgs[(size_t)(count - 1) * MSG_WORDS] : 0u);
}
// HF_QMETA with that ring put in; the other ring's head and count stay.
__host__ __device__ __forceinline__ uint32_t with_ring(uint32_t qm, const RingWords& r) {
  return (qm & ~r.mask) | r.qmeta;
}
// Field f (hf_is_queue) of a node whose REQ ring contributes rq() and whose RES ring rs(): each is
// asked only for the fields that need it (a ring's words may cost two loads).
template <typename RQ, typename RS>
__host__ __device__ __forceinline__ uint32_t queue_field_of(uint32_t f, const RQ& rq, const RS& rs) {
  switch (f) {
    case HF_QMETA: return with_ring(rq().qmeta, rs());
    case HF_REQ_ARR: return rq().arr;
    case HF_RES_ARR: return rs().arr;
    case HF_REQ_TAIL: return rq().tail;
    default: return rs().tail;
  }
}
// ... of a node whose REQ ring holds the rqc messages at rq and whose RES ring the rsc messages at rs
__host__ __device__ __forceinline__ uint32_t queue_field(uint32_t f, uint32_t rqc,
                                                         const uint32_t* rq, uint32_t rsc,
                                                         const uint32_t* rs) {
  return queue_field_of(f, [=] { return ring_words(0, rqc, rq); },
                        [=] { return ring_words(1, rsc, rs); });
}
// ... of a node whose rings contribute the words rq and rs
__host__ __device__ __forceinline__ uint32_t queue_field(uint32_t f, const RingWords& rq,
                                                         const RingWords& rs) {
  return queue_field_of(f, [&] { return rq; }, [&] { return rs; });
}

// Field f (< hot_fields(N)) of node k (id k + 1) of global cluster g after a restart at tick T
// (include/raftsim.h, "Node restarts"; SIM_SPEC §4a) from the node's words before it. h: the node's
// first hot word. mode 0 (RAFT_RESTART_AMNESIA) is init-node and a fresh log: role 0, term 1, no
// vote, no leader, no fault, an empty log whose arena window starts at the frontier (no arena slot
// is touched: payloads of this node still queued at peers stay readable). mode 1
// (RAFT_RESTART_DURABLE) keeps current_term, voted_for and the log (len, base, frontier). Both
// empty the two rings (queue_field of empty rings: head 0, count 0, arrival INF, tail 0), zero the
// commit index, the masks and the peer rows, and arm the election timer with the INIT draw of tick
// T, stored exact (FL_DRAW clear). The trace hash, the frontier and the last-led term are kept.
__host__ __device__ __forceinline__ uint32_t hot_restart(const uint32_t* h, uint32_t N, uint32_t f,
                                                         uint32_t mode, uint32_t T, uint32_t g,
                                                         uint32_t k, const DrawKeys& dk) {
  const bool durable = mode != 0;
  if (hf_is_queue(f)) return queue_field(f, ring_words(0, 0, 0u, 0u), ring_words(1, 0, 0u, 0u));
  if (f == hf_abase(N)) return h[(durable ? hf_abase(N) : hf_afront(N)) * N];
  if (f == hf_afront(N) || f == hf_led(N)) return h[f * N];
  switch (f) {
    case HF_DEADLINE: {
      const uint4 w = philox(g, (k + 1) | P_INIT << 8, T, 0, dk.key0, dk.key1);
      return T + dk.el_base + (uint32_t)(((uint64_t)w.y * dk.el_span) >> 32);
    }
    case HF_TRACE_LO:
    case HF_TRACE_HI: return h[f * N];
    case HF_FLAGS: return pack_flags(0, durable ? fl_vf(h[HF_FLAGS * N]) : 0u, 0, 0, 0, 0);
    case HF_TERM: return durable ? h[HF_TERM * N] : 1u;
    case HF_LEN: return durable ? h[HF_LEN * N] : 0u;
    default: return 0u;                                     // masks, commit index, next / match
  }
}

}  // namespace rs
