// scatter_host.hpp — the host side of raft_scatter_write (include/raftsim.h, "Cluster packs") that
// plain C++ can state: the predicates a node record and a queue must satisfy before they are
// written (raft_sim_write_nodes and raft_sim_write_queue ask the same ones), the check of a pack
// record against them, the search for a target named twice, and the planner that cuts a list of
// (record, target) pairs into the chunks a shard's scratch takes. Includes nothing from HIP:
// compiles under hipcc with raftsim.hip and under plain g++ with include/raftsim.h alone
// (tests/test_scatter_host.py runs both halves on the CPU).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/raftsim.h"

namespace rs {

// ---- The predicates of the state writers.

// Which clause of node_record_ok a record breaks (0: none); the order is the order of the tests.
enum NodeFault : int {
  NODE_OK = 0, NODE_ROLE, NODE_VOTED_FOR, NODE_LEADER_ID, NODE_FAULT, NODE_VOTES, NODE_LS_KEYS,
  NODE_IS_SEQ, NODE_LS_PRESENT, NODE_LOG_LEN, NODE_ARENA_SHORT, NODE_ARENA_LONG, NODE_LEADER_STATE,
  NODE_KEYS_WITHOUT_STATE
};
// Node `id` (1..N) of an N-node cluster with log_cap L.
inline NodeFault node_record_fault(const raft_node_t& n, uint32_t id, uint32_t N, uint32_t L) {
  const uint32_t all = ((1u << (N + 1)) - 1) & ~1u, peers = all & ~(1u << id);
  if (n.role > 3) return NODE_ROLE;
  if (n.voted_for > N) return NODE_VOTED_FOR;
  if (n.leader_id > N) return NODE_LEADER_ID;
  if (n.fault > 4) return NODE_FAULT;
  if (n.votes & ~all) return NODE_VOTES;
  if (n.ls_keys & ~peers) return NODE_LS_KEYS;
  if (n.entries_is_seq > 1) return NODE_IS_SEQ;
  if (n.ls_present > 1) return NODE_LS_PRESENT;
  if (n.log_len > L) return NODE_LOG_LEN;
  if (n.arena_frontier - n.arena_base < n.log_len) return NODE_ARENA_SHORT;
  if (n.arena_frontier - n.arena_base > L) return NODE_ARENA_LONG;
  if (n.role == RAFT_LEADER && (!n.ls_present || n.ls_keys != peers)) return NODE_LEADER_STATE;
  if (!n.ls_present && n.ls_keys) return NODE_KEYS_WITHOUT_STATE;
  return NODE_OK;
}
inline bool node_record_ok(const raft_node_t& n, uint32_t id, uint32_t N, uint32_t L) {
  return node_record_fault(n, id, N, L) == NODE_OK;
}

// Which clause of queue_ok a queue breaks (0: none).
enum QueueFault : int {
  QUEUE_OK = 0, QUEUE_COUNT, QUEUE_TYPE, QUEUE_SIDE, QUEUE_SRC, QUEUE_SELF, QUEUE_CLIENT_SRC,
  QUEUE_ORDER
};
// The `count` messages of queue `which` (0 REQ, 1 RES) of node `id`, head first; *at: the message.
inline QueueFault queue_fault(const raft_msg_t* in, uint32_t count, uint32_t which, uint32_t id,
                              uint32_t N, uint32_t Q, uint32_t* at = nullptr) {
  if (at) *at = 0;
  if (which > 1 || count > Q || (count && !in)) return QUEUE_COUNT;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t type = in[i].hdr & 7, src = (in[i].hdr >> 3) & 15;
    if (at) *at = i;
    if (type < 1 || type > 5) return QUEUE_TYPE;
    if ((type <= RAFT_MSG_CLIENT_SET ? 0u : 1u) != which) return QUEUE_SIDE;
    if (src > N) return QUEUE_SRC;
    if (src == id) return QUEUE_SELF;
    if ((type == RAFT_MSG_CLIENT_SET) != (src == 0)) return QUEUE_CLIENT_SRC;
    if (i > 0 && in[i].arrival < in[i - 1].arrival) return QUEUE_ORDER;
  }
  return QUEUE_OK;
}
inline bool queue_ok(const raft_msg_t* in, uint32_t count, uint32_t which, uint32_t id,
                     uint32_t N, uint32_t Q) {
  return queue_fault(in, count, which, id, N, Q) == QUEUE_OK;
}
// A queued client-set needs the general kernel (the LITE kernels run no P0).
inline bool queue_has_client_set(const raft_msg_t* in, uint32_t count) {
  for (uint32_t i = 0; i < count; ++i)
    if ((in[i].hdr & 7) == RAFT_MSG_CLIENT_SET) return true;
  return false;
}

// ---- One pack record against them. A queue's count is its node record's req_count / res_count
// and its messages are the first `count` of the ring in the record.
struct RecordShape {
  uint32_t N, Q, L;
  uint64_t off_cluster, off_nodes, off_queues;   // byte offsets of the parts in a record
};
struct RecordVerdict {
  int node_fault, queue_fault;     // NodeFault / QueueFault; both 0: the record may be written
  uint32_t id, which, msg;         // the node (1..N), and for a queue its side and message
  bool general;                    // a client-set is due or queued: the LITE kernels do not apply
  bool ok() const { return !node_fault && !queue_fault; }
};
inline RecordVerdict record_verdict(const uint8_t* rec, const RecordShape& sh) {
  RecordVerdict v = {0, 0, 0, 0, 0, false};
  const raft_node_t* const nodes = reinterpret_cast<const raft_node_t*>(rec + sh.off_nodes);
  const raft_msg_t* const q = reinterpret_cast<const raft_msg_t*>(rec + sh.off_queues);
  for (uint32_t k = 0; k < sh.N; ++k) {
    v.id = k + 1;
    if ((v.node_fault = node_record_fault(nodes[k], k + 1, sh.N, sh.L))) return v;
    for (uint32_t which = 0; which < 2; ++which) {
      const uint32_t count = which ? nodes[k].res_count : nodes[k].req_count;
      const raft_msg_t* const ring = q + ((size_t)k * 2 + which) * sh.Q;
      v.which = which;
      if ((v.queue_fault = queue_fault(ring, count, which, k + 1, sh.N, sh.Q, &v.msg))) return v;
      if (!which && queue_has_client_set(ring, count)) v.general = true;
    }
  }
  if (reinterpret_cast<const raft_cluster_t*>(rec + sh.off_cluster)->client_next != 0xFFFFFFFFu)
    v.general = true;
  return v;
}

// ---- A target named twice. Returns the first position i whose clusters[i] stands at an earlier
// position too (the second occurrence), or n when every target is distinct.
inline uint32_t first_duplicate(const uint32_t* clusters, uint32_t n) {
  std::vector<uint64_t> key(n);                  // (cluster, position): sorted by cluster first
  for (uint32_t i = 0; i < n; ++i) key[i] = (uint64_t)clusters[i] << 32 | i;
  std::sort(key.begin(), key.end());
  uint32_t first = n;
  for (uint32_t i = 1; i < n; ++i)
    if (key[i] >> 32 == key[i - 1] >> 32) first = std::min(first, (uint32_t)key[i]);
  return first;
}

// ---- The planner. The pairs are sorted by (owner shard, record, target); a chunk is a run of
// them inside one shard: its distinct records, uploaded once each, and behind them its list of
// (shard-local cluster, slot of the record in the chunk). A chunk is cut where one more pair would
// take distinct_records * stride + pairs * 8 past `bound`; it always holds one record and one pair
// at least (a stride at or above the bound gives chunks of one record), and a record with more
// targets than fit is uploaded again by the next chunk.
struct ScatterPair {
  uint32_t cluster, slot;          // what the kernel reads: 8 bytes, the gather's list entry
};
struct ScatterChunk {
  uint32_t shard;
  size_t pair0, pairs;             // its pairs: plan.pairs[pair0 .. pair0 + pairs)
  size_t rec0, records;            // its records: plan.records[rec0 .. rec0 + records), slot order
  uint64_t bytes(uint64_t stride) const { return records * stride + pairs * 8; }
};
struct ScatterPlan {
  std::vector<ScatterPair> pairs;
  std::vector<uint32_t> pos;       // pairs[i] is position pos[i] of the caller's lists
  std::vector<uint32_t> records;   // per chunk, the record of every slot
  std::vector<ScatterChunk> chunks;   // shard by shard
};
// lo: shard d owns clusters [lo[d], lo[d + 1]), G + 1 ascending bounds. records null: record i for
// position i. Every clusters[i] < lo[G] (the caller has checked the ranges).
inline ScatterPlan scatter_plan(const uint32_t* clusters, const uint32_t* records, uint32_t n,
                                const uint32_t* lo, uint32_t G, uint64_t stride, uint64_t bound) {
  struct Item {
    uint32_t shard, record, cluster, pos;
  };
  std::vector<Item> it(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = clusters[i];
    const uint32_t d = (uint32_t)(std::upper_bound(lo + 1, lo + G, c) - (lo + 1));
    it[i] = {d, records ? records[i] : i, c - lo[d], i};
  }
  std::sort(it.begin(), it.end(), [](const Item& a, const Item& b) {
    if (a.shard != b.shard) return a.shard < b.shard;
    if (a.record != b.record) return a.record < b.record;
    return a.cluster < b.cluster;
  });
  ScatterPlan p;
  p.pairs.resize(n);
  p.pos.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    const Item& x = it[i];
    bool open = !p.chunks.empty() && p.chunks.back().shard == x.shard;
    if (open) {                                  // an open chunk holds a record and a pair at least
      const ScatterChunk& c = p.chunks.back();
      const uint64_t more = (p.records.back() == x.record ? 0 : stride) + 8;
      open = c.bytes(stride) + more <= bound;
    }
    if (!open) p.chunks.push_back({x.shard, (size_t)i, 0, p.records.size(), 0});
    ScatterChunk& c = p.chunks.back();
    if (!c.records || p.records.back() != x.record) {
      p.records.push_back(x.record);
      ++c.records;
    }
    p.pairs[i] = {x.cluster, (uint32_t)(c.records - 1)};
    p.pos[i] = x.pos;
    ++c.pairs;
  }
  return p;
}

}  // namespace rs
