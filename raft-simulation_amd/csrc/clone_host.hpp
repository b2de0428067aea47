// clone_host.hpp — the host side of raft_clone_write (include/raftsim.h, "Cluster clones") that plain
// C++ can state: the checks of the two lists that need no device (the ranges, a target named twice
// -- scatter_host.hpp's first_duplicate --, a cluster of one handle that is both read and written)
// and the planner that groups the (target, source) pairs by the shards they join and cuts each
// group into the chunks a shard's scratch takes. Includes nothing from HIP: compiles under hipcc
// with raftsim.hip and under plain g++ with include/raftsim.h alone (tests/test_clone_host.py runs
// it on the CPU).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <iterator>
#include <vector>

#include "scatter_host.hpp"

namespace rs {

// ---- The lists. Each returns the first offending position, or n when there is none.

// The first i with ids[i] >= C.
inline uint32_t first_outside(const uint32_t* ids, uint32_t n, uint32_t C) {
  for (uint32_t i = 0; i < n; ++i)
    if (ids[i] >= C) return i;
  return n;
}

// src == dst: the first position whose target is a source somewhere in the list or whose source is
// a target somewhere (a clone reads every source as it was before the call, so no cluster may be
// both). *target_is_source: which of the two holds at that position (the target's when both do).
// Two sorted copies and their intersection, n log n; the positions are searched only when the
// intersection is not empty.
inline uint32_t first_source_target(const uint32_t* targets, const uint32_t* sources, uint32_t n,
                                    bool* target_is_source = nullptr) {
  std::vector<uint32_t> t(targets, targets + n), s(sources, sources + n), both;
  std::sort(t.begin(), t.end());
  std::sort(s.begin(), s.end());
  std::set_intersection(t.begin(), t.end(), s.begin(), s.end(), std::back_inserter(both));
  if (both.empty()) return n;
  for (uint32_t i = 0; i < n; ++i) {
    const bool ts = std::binary_search(both.begin(), both.end(), targets[i]);
    if (ts || std::binary_search(both.begin(), both.end(), sources[i])) {
      if (target_is_source) *target_is_source = ts;
      return i;
    }
  }
  return n;
}

// ---- The planner. The pairs are sorted by (target shard, source shard, target); a chunk is a run
// of them that joins one source shard to one target shard, as the kernel reads it: (target, source)
// in shard-local ids, 8 bytes a pair, uploaded into the target shard's scratch. A group is cut
// every max_pairs pairs (>= 1: what the scratch holds), never earlier.
struct ClonePair {
  uint32_t target, source;         // what the kernel reads: a uint2, x the target
};
struct CloneChunk {
  uint32_t dst_shard, src_shard;
  size_t pair0, pairs;             // its pairs: plan.pairs[pair0 .. pair0 + pairs)
};
struct ClonePlan {
  std::vector<ClonePair> pairs;
  std::vector<uint32_t> pos;       // pairs[i] is position pos[i] of the caller's lists
  std::vector<CloneChunk> chunks;  // target shard by target shard
};
// The index of the shard owning cluster c: shard d owns [lo[d], lo[d + 1]), G + 1 ascending bounds.
inline uint32_t shard_of(const uint32_t* lo, uint32_t G, uint32_t c) {
  return (uint32_t)(std::upper_bound(lo + 1, lo + G, c) - (lo + 1));
}
// tlo / TG: the target handle's shards, slo / SG: the source handle's. Every targets[i] < tlo[TG]
// and every sources[i] < slo[SG] (the caller has checked the ranges).
inline ClonePlan clone_plan(const uint32_t* targets, const uint32_t* tlo, uint32_t TG,
                            const uint32_t* sources, const uint32_t* slo, uint32_t SG, uint32_t n,
                            uint64_t max_pairs) {
  struct Item {
    uint32_t dst, src, target, source, pos;
  };
  std::vector<Item> it(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t d = shard_of(tlo, TG, targets[i]), e = shard_of(slo, SG, sources[i]);
    it[i] = {d, e, targets[i] - tlo[d], sources[i] - slo[e], i};
  }
  std::sort(it.begin(), it.end(), [](const Item& a, const Item& b) {
    if (a.dst != b.dst) return a.dst < b.dst;
    if (a.src != b.src) return a.src < b.src;
    return a.target < b.target;
  });
  if (max_pairs < 1) max_pairs = 1;
  ClonePlan p;
  p.pairs.resize(n);
  p.pos.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    const Item& x = it[i];
    if (p.chunks.empty() || p.chunks.back().dst_shard != x.dst ||
        p.chunks.back().src_shard != x.src || p.chunks.back().pairs >= max_pairs)
      p.chunks.push_back({x.dst, x.src, (size_t)i, 0});
    p.pairs[i] = {x.target, x.source};
    p.pos[i] = x.pos;
    ++p.chunks.back().pairs;
  }
  return p;
}

}  // namespace rs
