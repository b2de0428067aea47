"""csrc/scatter_host.hpp on the CPU: the planner that cuts a scatter's (record, target) pairs into
the chunks of a shard's scratch, and the predicates a pack record must satisfy before it is written.

A stand-alone C++ program (its own main, the header and include/raftsim.h alone) is compiled with
g++ -- under ASan and UBSan where the machine has their runtimes -- and run once.

Planner, for random lists (1..4 shards, strides 16..4096, bounds of a few records, records repeated
and not) and the adversarial ones -- one record with 10^7 targets; n records of stride just under,
at and over the bound; the strides 640 and 1,485,040 against the 64-MiB bound; identity lists --:
every pair of the caller's lists lies in exactly one chunk, as (its target's shard-local cluster,
the slot of its record); a chunk's records * stride + pairs * 8 is within the bound, or the chunk
is a single record with at least one pair -- and then no further pair of that record would have
fitted; every pair's slot is below its chunk's record count; a chunk's slots name its records in
ascending order, each used; the pairs of a shard stay in that shard's chunks, which follow each
other.

Validation: a valid record passes; for each clause of the node predicate and of the queue
predicate a record that breaks only that clause is refused with that clause's code, its node and
message; a queue's count is its node record's; a client cursor or a queued client-set marks the
record as needing the general kernel; first_duplicate finds the second occurrence with the
smallest position."""
import hostprog

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "scatter_host.hpp"

using namespace rs;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {                      // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static long checks = 0, bad = 0;
static void expect(bool ok, const char* what, const char* who, long a, long b) {
  ++checks;
  if (!ok && bad++ < 20) printf("MISMATCH %s (%s) at %ld, %ld\n", what, who, a, b);
}

// ---- planner ------------------------------------------------------------------------------------
static void check_plan(const char* who, const std::vector<uint32_t>& clusters,
                       const std::vector<uint32_t>* records, const std::vector<uint32_t>& lo,
                       uint64_t stride, uint64_t bound) {
  const uint32_t n = (uint32_t)clusters.size(), G = (uint32_t)lo.size() - 1;
  const ScatterPlan p = scatter_plan(clusters.data(), records ? records->data() : nullptr, n,
                                     lo.data(), G, stride, bound);
  expect(p.pairs.size() == n && p.pos.size() == n, "a pair per position", who, n, 0);
  if (p.pairs.size() != n || p.pos.size() != n) return;
  std::vector<uint8_t> seen(n, 0);
  size_t next_pair = 0, next_rec = 0;
  uint32_t shard = 0;
  for (size_t ci = 0; ci < p.chunks.size(); ++ci) {
    const ScatterChunk& c = p.chunks[ci];
    expect(c.pair0 == next_pair && c.rec0 == next_rec, "chunks tile the lists", who, ci, 0);
    expect(c.pairs >= 1 && c.records >= 1, "a record and a pair at least", who, ci, 0);
    expect(c.shard >= shard && c.shard < G, "shard by shard", who, ci, c.shard);
    shard = c.shard;
    next_pair = c.pair0 + c.pairs;
    next_rec = c.rec0 + c.records;
    if (next_pair > n || next_rec > p.records.size()) {
      expect(false, "chunk leaves the lists", who, ci, 0);
      return;
    }
    const bool fits = c.bytes(stride) <= bound;
    expect(fits || c.records == 1, "within the bound, or a single record", who, ci, c.records);
    // a record over the bound carries one pair: nothing more fits beside it
    if (!fits) expect(c.pairs == 1, "over the bound only as one record and one pair", who, ci, c.pairs);
    for (size_t k = 1; k < c.records; ++k)
      expect(p.records[c.rec0 + k] > p.records[c.rec0 + k - 1], "a chunk's records ascend", who, ci, k);
    std::vector<uint8_t> used(c.records, 0);
    for (size_t i = c.pair0; i < c.pair0 + c.pairs; ++i) {
      const uint32_t pos = p.pos[i];
      if (pos >= n || p.pairs[i].slot >= c.records) {
        expect(false, "slot below the chunk's records, position in the list", who, ci, i);
        continue;
      }
      ++checks;
      used[p.pairs[i].slot] = 1;
      expect(!seen[pos], "a pair lies in one chunk only", who, pos, ci);
      seen[pos] = 1;
      const uint32_t want_rec = records ? (*records)[pos] : pos;
      expect(p.records[c.rec0 + p.pairs[i].slot] == want_rec, "the slot holds the pair's record",
             who, pos, want_rec);
      const uint32_t g = clusters[pos];
      expect(g >= lo[c.shard] && g < lo[c.shard + 1] && p.pairs[i].cluster == g - lo[c.shard],
             "the target is the shard's local cluster", who, pos, g);
    }
    for (size_t k = 0; k < c.records; ++k) expect(used[k], "every uploaded record is used", who, ci, k);
    // a cut is forced: the next pair of the same shard would not have fitted
    if (ci + 1 < p.chunks.size() && p.chunks[ci + 1].shard == c.shard) {
      const ScatterChunk& d = p.chunks[ci + 1];
      const bool same = p.records[d.rec0] == p.records[c.rec0 + c.records - 1];
      expect(c.bytes(stride) + (same ? 0 : stride) + 8 > bound, "no early cut", who, ci, 0);
    }
  }
  expect(next_pair == n && next_rec == p.records.size(), "chunks cover the lists", who, n, 0);
  for (uint32_t i = 0; i < n; ++i) expect(seen[i], "every pair lies in a chunk", who, i, 0);
}

static std::vector<uint32_t> iota(uint32_t n, uint32_t from = 0) {
  std::vector<uint32_t> v(n);
  for (uint32_t i = 0; i < n; ++i) v[i] = from + i;
  return v;
}
static std::vector<uint32_t> shards(uint32_t C, uint32_t G) {
  std::vector<uint32_t> lo(G + 1);
  for (uint32_t d = 0; d <= G; ++d) lo[d] = (uint32_t)((uint64_t)C * d / G);
  return lo;
}
static void shuffle(std::vector<uint32_t>& v) {
  for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rnd() % i]);
}

static void planner() {
  const uint64_t MiB64 = 64ull << 20;
  // random lists
  for (int rep = 0; rep < 400; ++rep) {
    const uint32_t G = 1 + rnd() % 4, C = G + rnd() % 500, n = rnd() % (C + 1);
    const uint32_t n_records = 1 + rnd() % 40;
    const uint64_t stride = 16 * (1 + rnd() % 256), bound = stride * (1 + rnd() % 6) + 8 * (rnd() % 64);
    std::vector<uint32_t> cl = iota(C);
    shuffle(cl);
    cl.resize(n);
    std::vector<uint32_t> rec(n);
    for (auto& x : rec) x = rnd() % n_records;
    check_plan("random", cl, &rec, shards(C, G), stride, bound);
    if (n) check_plan("random, in order", cl, nullptr, shards(C, G), stride, bound);
  }
  // one record with 10^7 targets: 8 bytes a pair, so two chunks of the 64-MiB bound
  {
    const uint32_t n = 10000000;
    const std::vector<uint32_t> cl = iota(n), rec(n, 3);
    check_plan("fan-out 1e7", cl, &rec, shards(n, 1), 4688, MiB64);
    check_plan("fan-out 1e7, 3 shards", cl, &rec, shards(n, 3), 4688, MiB64);
  }
  // n records of stride just under, at and over the bound
  for (uint64_t bound : {4096ull, 65536ull})
    for (int64_t d : {-16, -8, 0, 8, 16})
      for (uint32_t n : {1u, 2u, 7u}) {
        const uint64_t stride = bound + d - 8;           // stride + 8 is the bound + d
        check_plan("stride near the bound", iota(n), nullptr, shards(n, 1), stride, bound);
        const std::vector<uint32_t> rec(n, 0);
        check_plan("stride near the bound, one record", iota(n), &rec, shards(n, 2), stride, bound);
      }
  // the smallest and the largest record the gather's tests hold
  for (uint64_t stride : {640ull, 1485040ull}) {
    for (uint32_t n : {1u, 45u, 46u, 4096u, 131072u}) {
      check_plan("identity", iota(n), nullptr, shards(n, 1), stride, MiB64);
      check_plan("identity, 3 shards", iota(n), nullptr, shards(n, 3), stride, MiB64);
      std::vector<uint32_t> cl = iota(n), rec(n);
      for (uint32_t i = 0; i < n; ++i) rec[i] = (n - 1 - i) / 3;
      std::reverse(cl.begin(), cl.end());
      check_plan("reversed thirds", cl, &rec, shards(n, 3), stride, MiB64);
    }
  }
  check_plan("empty", {}, nullptr, shards(5, 2), 640, MiB64);
}

// ---- validation ---------------------------------------------------------------------------------
constexpr uint32_t N = 5, Q = 4, L = 8;
struct Record {
  raft_cluster_t cl;
  raft_node_t nodes[N];
  raft_msg_t q[N][2][Q];
};
static const RecordShape shape = {N, Q, L, offsetof(Record, cl), offsetof(Record, nodes),
                                  offsetof(Record, q)};
static uint32_t hdr(uint32_t type, uint32_t src) { return type | src << 3; }

static Record valid() {
  Record r;
  memset(&r, 0, sizeof r);
  r.cl.client_next = 0xFFFFFFFFu;
  for (uint32_t k = 0; k < N; ++k) {
    raft_node_t& n = r.nodes[k];
    n.role = RAFT_FOLLOWER;
    n.leader_id = 1;
    n.log_len = 3;
    n.arena_base = 0xFFFFFFFEu;              // frontier - base wraps: 5
    n.arena_frontier = 3;
  }
  raft_node_t& ld = r.nodes[0];
  ld.role = RAFT_LEADER;
  ld.ls_present = 1;
  ld.ls_keys = 0x3C;                         // peers 2..5
  ld.votes = 0x0E;
  ld.res_count = 2;
  r.q[0][1][0] = {10, hdr(RAFT_MSG_APPEND_RESPONSE, 2), 1, 0, 0, 0, 0, 0};
  r.q[0][1][1] = {10, hdr(RAFT_MSG_APPEND_RESPONSE, 3), 1, 0, 0, 0, 0, 0};
  r.q[0][1][2] = {1, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0};   // past the count: never looked at
  r.nodes[2].req_count = 1;
  r.q[2][0][0] = {12, hdr(RAFT_MSG_APPEND_ENTRIES, 1), 1, 0, 0, 0, 0, 0};
  return r;
}
static RecordVerdict verdict(const Record& r) {
  return record_verdict(reinterpret_cast<const uint8_t*>(&r), shape);
}

static void validation() {
  expect(verdict(valid()).ok() && !verdict(valid()).general, "a valid record passes", "valid", 0, 0);
  // the node predicate, clause by clause, at node 4 (a follower) unless the clause needs the leader
  struct NodeCase {
    int fault;
    uint32_t id;
    void (*breakit)(raft_node_t&);
  };
  static const NodeCase node_cases[] = {
      {NODE_ROLE, 4, [](raft_node_t& n) { n.role = 4; }},
      {NODE_VOTED_FOR, 4, [](raft_node_t& n) { n.voted_for = N + 1; }},
      {NODE_LEADER_ID, 4, [](raft_node_t& n) { n.leader_id = N + 1; }},
      {NODE_FAULT, 4, [](raft_node_t& n) { n.fault = 5; }},
      {NODE_VOTES, 4, [](raft_node_t& n) { n.votes = 1u << (N + 1); }},
      {NODE_VOTES, 4, [](raft_node_t& n) { n.votes = 1; }},
      {NODE_LS_KEYS, 4, [](raft_node_t& n) { n.ls_present = 1; n.ls_keys = 1u << 4; }},
      {NODE_IS_SEQ, 4, [](raft_node_t& n) { n.entries_is_seq = 2; }},
      {NODE_LS_PRESENT, 4, [](raft_node_t& n) { n.ls_present = 2; }},
      {NODE_LOG_LEN, 4, [](raft_node_t& n) { n.log_len = L + 1; n.arena_frontier = n.arena_base + L + 1; }},
      {NODE_ARENA_SHORT, 4, [](raft_node_t& n) { n.arena_frontier = n.arena_base + 2; }},
      {NODE_ARENA_LONG, 4, [](raft_node_t& n) { n.arena_frontier = n.arena_base + L + 1; }},
      {NODE_LEADER_STATE, 1, [](raft_node_t& n) { n.ls_present = 0; n.ls_keys = 0; }},
      {NODE_LEADER_STATE, 1, [](raft_node_t& n) { n.ls_keys = 0x1C; }},
      {NODE_KEYS_WITHOUT_STATE, 4, [](raft_node_t& n) { n.ls_keys = 0x06; }},
  };
  int i = 0;
  for (const NodeCase& c : node_cases) {
    Record r = valid();
    c.breakit(r.nodes[c.id - 1]);
    const RecordVerdict v = verdict(r);
    expect(!v.ok() && v.node_fault == c.fault && v.id == c.id && !v.queue_fault, "node clause",
           "validation", i, v.node_fault);
    expect(!node_record_ok(r.nodes[c.id - 1], c.id, N, L) &&
               node_record_fault(r.nodes[c.id - 1], c.id, N, L) == c.fault,
           "node predicate", "validation", i, 0);
    ++i;
  }
  // the largest legal values pass
  {
    Record r = valid();
    raft_node_t& n = r.nodes[3];
    n.role = 3; n.voted_for = N; n.leader_id = N; n.fault = 4; n.votes = 0x3E; n.entries_is_seq = 1;
    n.ls_present = 1; n.ls_keys = 0x2E; n.log_len = L; n.arena_frontier = n.arena_base + L;
    expect(verdict(r).ok(), "the largest legal values pass", "validation", 0, 0);
  }
  // the queue predicate, clause by clause: node 3's REQ queue, node 1's RES queue
  struct QueueCase {
    int fault;
    uint32_t id, which, msg;
    void (*breakit)(Record&);
  };
  static const QueueCase queue_cases[] = {
      {QUEUE_COUNT, 3, 0, 0, [](Record& r) { r.nodes[2].req_count = Q + 1; }},
      {QUEUE_COUNT, 1, 1, 0, [](Record& r) { r.nodes[0].res_count = 0xFFFFFFFFu; }},
      {QUEUE_TYPE, 3, 0, 0, [](Record& r) { r.q[2][0][0].hdr = hdr(0, 1); }},
      {QUEUE_TYPE, 3, 0, 0, [](Record& r) { r.q[2][0][0].hdr = hdr(6, 1); }},
      {QUEUE_SIDE, 3, 0, 0, [](Record& r) { r.q[2][0][0].hdr = hdr(RAFT_MSG_APPEND_RESPONSE, 1); }},
      {QUEUE_SIDE, 1, 1, 1, [](Record& r) { r.q[0][1][1].hdr = hdr(RAFT_MSG_APPEND_ENTRIES, 3); }},
      {QUEUE_SRC, 3, 0, 0, [](Record& r) { r.q[2][0][0].hdr = hdr(RAFT_MSG_APPEND_ENTRIES, N + 1); }},
      {QUEUE_SELF, 3, 0, 0, [](Record& r) { r.q[2][0][0].hdr = hdr(RAFT_MSG_APPEND_ENTRIES, 3); }},
      {QUEUE_CLIENT_SRC, 3, 0, 0, [](Record& r) { r.q[2][0][0].hdr = hdr(RAFT_MSG_CLIENT_SET, 1); }},
      {QUEUE_CLIENT_SRC, 3, 0, 0, [](Record& r) { r.q[2][0][0].hdr = hdr(RAFT_MSG_APPEND_ENTRIES, 0); }},
      {QUEUE_ORDER, 1, 1, 1, [](Record& r) { r.q[0][1][1].arrival = 9; }},
      // the count is the node record's: a third message comes into view
      {QUEUE_TYPE, 1, 1, 2, [](Record& r) { r.nodes[0].res_count = 3; }},
  };
  i = 0;
  for (const QueueCase& c : queue_cases) {
    Record r = valid();
    c.breakit(r);
    const RecordVerdict v = verdict(r);
    expect(!v.ok() && !v.node_fault && v.queue_fault == c.fault && v.id == c.id &&
               v.which == c.which && v.msg == c.msg, "queue clause", "validation", i, v.queue_fault);
    ++i;
  }
  expect(!queue_ok(nullptr, 1, 0, 1, N, Q) && queue_ok(nullptr, 0, 0, 1, N, Q) &&
             !queue_ok(nullptr, 0, 2, 1, N, Q), "null queue, side 2", "validation", 0, 0);
  // what needs the general kernel
  {
    Record r = valid();
    r.cl.client_next = 77;
    expect(verdict(r).ok() && verdict(r).general, "a client cursor", "validation", 0, 0);
    r = valid();
    r.nodes[3].req_count = 1;
    r.q[3][0][0] = {5, hdr(RAFT_MSG_CLIENT_SET, 0), 0, 9, 0, 0, 0, 0};
    expect(verdict(r).ok() && verdict(r).general, "a queued client-set", "validation", 0, 0);
    r.nodes[3].req_count = 0;                  // outside the count: not queued
    expect(verdict(r).ok() && !verdict(r).general, "a client-set past the count", "validation", 0, 0);
  }
  // duplicates: the second occurrence with the smallest position
  {
    const uint32_t a[] = {5, 9, 2, 9, 5, 2, 9};
    expect(first_duplicate(a, 7) == 3, "second occurrence", "duplicates", first_duplicate(a, 7), 0);
    expect(first_duplicate(a, 3) == 3 && first_duplicate(a, 0) == 0 && first_duplicate(a, 1) == 1,
           "no duplicate", "duplicates", 0, 0);
    const uint32_t b[] = {0xFFFFFFFFu, 0, 0xFFFFFFFFu};
    expect(first_duplicate(b, 3) == 2, "the largest id", "duplicates", 0, 0);
    std::vector<uint32_t> big = iota(100000);
    shuffle(big);
    expect(first_duplicate(big.data(), 100000) == 100000, "a permutation", "duplicates", 0, 0);
    big[77777] = big[123];
    expect(first_duplicate(big.data(), 100000) == 77777, "one repeat", "duplicates", 0, 0);
  }
}

int main() {
  planner();
  validation();
  printf("checks %ld bad %ld\n", checks, bad);
  return bad ? 1 : 0;
}
"""


def test_the_planner_places_every_pair_once_and_the_predicates_refuse_by_clause(tmp_path):
    out = hostprog.run_cpp(tmp_path, "scatter_check", PROGRAM, sanitizers=("undefined", "address"),
                           timeout=300)
    assert hostprog.checks(out) > 1000000
