// restart_host.hpp — the host side of raft_restart_write and raft_restart_where (include/raftsim.h,
// "Node restarts") that plain C++ can state: the checks of the (cluster, node mask) list that need
// no device (the ranges and a cluster named twice are clone_host.hpp's first_outside and
// scatter_host.hpp's first_duplicate; here a mask that names no node or a node the cluster does not
// have), the horizon of the re-armed election timer, and the planner that sorts the pairs by shard,
// translates them to shard-local ids and cuts them into the chunks a shard's scratch takes.
// Includes nothing from HIP: compiles under hipcc with raftsim.hip and under plain g++ with
// include/raftsim.h alone (tests/test_restart_host.py runs it on the CPU).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "clone_host.hpp"

namespace rs {

// ---- The list. Each check returns the first offending position, or n when there is none.

// Bit j of a mask is node id j, as `votes`: the ids of an N-node cluster are bits 1..N.
constexpr uint32_t restart_ids(uint32_t N) { return ((1u << (N + 1)) - 1) & ~1u; }
// The first i whose mask is 0 or has a bit outside ids 1..N.
inline uint32_t first_bad_mask(const uint16_t* nodes, uint32_t n, uint32_t N) {
  const uint32_t ids = restart_ids(N);
  for (uint32_t i = 0; i < n; ++i)
    if (nodes[i] == 0 || (nodes[i] & ~ids)) return i;
  return n;
}

// Which check a list fails (0: none), in the order the call makes them, and where.
enum RestartFault : int { RESTART_OK = 0, RESTART_OUTSIDE, RESTART_TWICE, RESTART_MASK };
inline RestartFault restart_list_fault(const uint32_t* clusters, const uint16_t* nodes, uint32_t n,
                                       uint32_t C, uint32_t N, uint32_t* at) {
  if ((*at = first_outside(clusters, n, C)) < n) return RESTART_OUTSIDE;
  if ((*at = first_duplicate(clusters, n)) < n) return RESTART_TWICE;
  if ((*at = first_bad_mask(nodes, n, N)) < n) return RESTART_MASK;
  return RESTART_OK;
}

// A restart at tick T re-arms the timer below T + el_base + el_span, which must stay below the
// "never" marker 2^32 - 1 (SIM_SPEC D1).
inline bool restart_horizon_ok(uint64_t T, uint32_t el_base, uint32_t el_span) {
  return T + el_base + el_span < 0xFFFFFFFFull;
}

// ---- The planner. The pairs are sorted by cluster, which sorts them by shard (a shard owns a run
// of consecutive clusters); a chunk is a run of them inside one shard, as the kernel reads it:
// (shard-local cluster, mask), 8 bytes a pair, uploaded into the shard's scratch. A shard's run is
// cut every max_pairs pairs (>= 1: what the scratch holds), never earlier.
struct RestartPair {
  uint32_t cluster, mask;          // what the kernel reads: a uint2, x the cluster
};
struct RestartChunk {
  uint32_t shard;
  size_t pair0, pairs;             // its pairs: plan.pairs[pair0 .. pair0 + pairs)
};
struct RestartPlan {
  std::vector<RestartPair> pairs;
  std::vector<uint32_t> pos;       // pairs[i] is position pos[i] of the caller's lists
  std::vector<RestartChunk> chunks;   // shard by shard
  uint64_t nodes = 0;              // the nodes named: the popcounts of the masks, summed
};
// lo: shard d owns clusters [lo[d], lo[d + 1]), G + 1 ascending bounds. Every clusters[i] < lo[G]
// (the caller has checked the ranges).
inline RestartPlan restart_plan(const uint32_t* clusters, const uint16_t* nodes, uint32_t n,
                                const uint32_t* lo, uint32_t G, uint64_t max_pairs) {
  std::vector<uint64_t> key(n);                  // (cluster, position)
  for (uint32_t i = 0; i < n; ++i) key[i] = (uint64_t)clusters[i] << 32 | i;
  std::sort(key.begin(), key.end());
  if (max_pairs < 1) max_pairs = 1;
  RestartPlan p;
  p.pairs.resize(n);
  p.pos.resize(n);
  uint32_t d = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = (uint32_t)(key[i] >> 32), at = (uint32_t)key[i];
    if (c >= lo[d + 1]) d = shard_of(lo, G, c);
    if (p.chunks.empty() || p.chunks.back().shard != d || p.chunks.back().pairs >= max_pairs)
      p.chunks.push_back({d, (size_t)i, 0});
    p.pairs[i] = {c - lo[d], nodes[at]};
    p.pos[i] = at;
    p.nodes += (uint32_t)__builtin_popcount(nodes[at]);
    ++p.chunks.back().pairs;
  }
  return p;
}

}  // namespace rs
