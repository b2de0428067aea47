"""The host-compilable half of raft_clone_write on the CPU: csrc/clone_host.hpp (the list checks and
the planner) and what clone_kernel takes from csrc/node_codec.hpp and csrc/pack.hpp (the direct
hot-word mapping, the value form of ring_words, the arena access width, the commit-stream rule).

Two stand-alone C++ programs (each its own main), compiled under ASan and UBSan where the compiler
has their runtimes and run once; each ends `checks N bad 0`.

1. The planner (g++, the header and include/raftsim.h alone). For random lists (1..4 shards on
   either side, bounds of 1, 2, 7, 2^23 and random pairs), one source with 10^6 targets on one and
   on three shards, identity lists, and three shards with every (source shard, target shard)
   combination: every position of the caller's lists lies in exactly one chunk, as (its target's,
   its source's) shard-local ids of the chunk's two shards; a chunk holds 1..bound pairs; chunks
   tile the pairs, target shard by target shard and inside one source shard by source shard; no cut
   is early (a chunk followed by one of the same two shards is full). The refusals name the first
   offending position: an id outside the handle, a target named twice, a cluster that is both a
   source and a target -- found in a 10^6-pair list in well under a second (two sorts, not n^2).

2. The codec (hipcc, host only). N = 2..9 over random 32-bit hot words, FL_DRAW set and clear:
   hot_clone equals hot_field(node_word(...)) for every non-queue field, and resolves the draw with
   the id it is given. Q = 1..16, every count 0..Q, random heads: the value form of ring_words and
   queue_field over a ring's own first and last arrivals equals the pointer form over the ring
   linearised as a pack holds it. arena_access_bytes: a copy between two arenas made of the
   accesses it chooses, for even and odd N * A and every pair of source and target cluster (all
   four parities): a 16-byte access only on a 16-byte address with both entries present, and
   always there; the target's entries are the source's and nothing else is written; the last
   entry of an odd total moves alone. stream_slot_kept: the target ring of scatter(gather(ring))
   is the source's slot where it says kept and 0 elsewhere, for commit_count below, at and far
   above the ring's size."""
import hostprog

COMMON = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

static uint64_t rng_state = 0x452821E638D01377ull;
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
"""

PLANNER = COMMON + r"""
#include "clone_host.hpp"

using namespace rs;

static void check_plan(const char* who, const std::vector<uint32_t>& targets,
                       const std::vector<uint32_t>& sources, const std::vector<uint32_t>& tlo,
                       const std::vector<uint32_t>& slo, uint64_t bound) {
  const uint32_t n = (uint32_t)targets.size(), TG = (uint32_t)tlo.size() - 1,
                 SG = (uint32_t)slo.size() - 1;
  const ClonePlan p = clone_plan(targets.data(), tlo.data(), TG, sources.data(), slo.data(), SG, n,
                                 bound);
  expect(p.pairs.size() == n && p.pos.size() == n, "a pair per position", who, n, 0);
  if (p.pairs.size() != n || p.pos.size() != n) return;
  std::vector<uint8_t> seen(n, 0);
  size_t next_pair = 0;
  for (size_t ci = 0; ci < p.chunks.size(); ++ci) {
    const CloneChunk& c = p.chunks[ci];
    expect(c.pair0 == next_pair, "chunks tile the pairs", who, ci, 0);
    expect(c.pairs >= 1 && c.pairs <= bound, "1..bound pairs", who, ci, c.pairs);
    expect(c.dst_shard < TG && c.src_shard < SG, "shards of the handles", who, ci, 0);
    next_pair = c.pair0 + c.pairs;
    if (next_pair > n || c.dst_shard >= TG || c.src_shard >= SG) {
      expect(false, "chunk leaves the lists", who, ci, 0);
      return;
    }
    if (ci) {
      const CloneChunk& b = p.chunks[ci - 1];
      expect(b.dst_shard < c.dst_shard || (b.dst_shard == c.dst_shard && b.src_shard <= c.src_shard),
             "target shard by target shard, then source shard by source shard", who, ci, 0);
      if (b.dst_shard == c.dst_shard && b.src_shard == c.src_shard)
        expect(b.pairs == bound, "no early cut", who, ci, b.pairs);
    }
    for (size_t i = c.pair0; i < next_pair; ++i) {
      const uint32_t pos = p.pos[i];
      if (pos >= n) {
        expect(false, "a position of the lists", who, ci, i);
        continue;
      }
      expect(!seen[pos], "a pair lies in one chunk only", who, pos, ci);
      seen[pos] = 1;
      const uint32_t t = targets[pos], s = sources[pos];
      expect(t >= tlo[c.dst_shard] && t < tlo[c.dst_shard + 1] &&
                 p.pairs[i].target == t - tlo[c.dst_shard],
             "the target is its shard's local cluster", who, pos, t);
      expect(s >= slo[c.src_shard] && s < slo[c.src_shard + 1] &&
                 p.pairs[i].source == s - slo[c.src_shard],
             "the source is its shard's local cluster", who, pos, s);
    }
  }
  expect(next_pair == n, "chunks cover the pairs", who, n, 0);
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
  const uint64_t bounds[] = {1, 2, 7, 1ull << 23};
  for (int rep = 0; rep < 400; ++rep) {
    const uint32_t TG = 1 + rnd() % 4, SG = 1 + rnd() % 4, TC = TG + rnd() % 400,
                   SC = SG + rnd() % 400, n = rnd() % (TC + 1);
    std::vector<uint32_t> t = iota(TC), s(n);
    shuffle(t);
    t.resize(n);
    for (auto& x : s) x = rnd() % SC;
    const uint64_t bound = rep % 5 < 4 ? bounds[rep % 5] : 1 + rnd() % 64;
    check_plan("random", t, s, shards(TC, TG), shards(SC, SG), bound);
  }
  {                                          // one source, 10^6 targets
    const uint32_t n = 1000000;
    const std::vector<uint32_t> t = iota(n, 1), s(n, 0);
    for (uint64_t bound : bounds) {
      if (bound < 7) continue;               // (10^6 chunks of one pair say nothing more)
      check_plan("one source 1e6", t, s, shards(n + 1, 1), shards(n + 1, 1), bound);
      check_plan("one source 1e6, 3 shards", t, s, shards(n + 1, 3), shards(n + 1, 3), bound);
    }
    check_plan("one source 1e5, bound 1", iota(100000, 1), std::vector<uint32_t>(100000, 0),
               shards(100001, 3), shards(100001, 3), 1);
  }
  for (uint32_t n : {1u, 2u, 7u, 8u, 4096u, 131072u})   // identity lists (a snapshot)
    for (uint64_t bound : bounds) {
      check_plan("identity", iota(n), iota(n), shards(n, 1), shards(n, 1), bound);
      check_plan("identity, 3 shards into 1", iota(n), iota(n), shards(n, 1),
                 shards(n, std::min(n, 3u)), bound);
      check_plan("identity, 3 shards", iota(n), iota(n), shards(n, std::min(n, 3u)),
                 shards(n, std::min(n, 3u)), bound);
    }
  {                                          // three shards, every (source shard, target shard)
    const uint32_t C = 3001;
    const std::vector<uint32_t> lo = shards(C, 3);
    std::vector<uint32_t> t, s;
    for (uint32_t a = 0; a < 3; ++a)
      for (uint32_t b = 0; b < 3; ++b)
        for (uint32_t j = 0; j < 100; ++j) {
          t.push_back(lo[a] + b * 100 + j);          // distinct targets of shard a
          s.push_back(lo[b] + 500 + (j * 7 + a) % 400);
        }
    for (uint64_t bound : bounds) {
      check_plan("every combination", t, s, lo, lo, bound);
      const ClonePlan p = clone_plan(t.data(), lo.data(), 3, s.data(), lo.data(), 3,
                                     (uint32_t)t.size(), bound);
      uint32_t combos = 0;
      for (size_t i = 0; i < p.chunks.size(); ++i)
        combos += !i || p.chunks[i].dst_shard != p.chunks[i - 1].dst_shard ||
                  p.chunks[i].src_shard != p.chunks[i - 1].src_shard;
      expect(combos == 9 && p.chunks.size() == 9 * ((100 + bound - 1) / bound),
             "nine groups, each cut every bound pairs", "every combination", combos, p.chunks.size());
    }
  }
  check_plan("empty", {}, {}, shards(5, 2), shards(9, 3), 7);
  // a bound of 0 is a bound of 1: a chunk always holds a pair
  expect(clone_plan(iota(3).data(), shards(3, 1).data(), 1, iota(3).data(), shards(3, 1).data(), 1, 3,
                    0).chunks.size() == 3, "bound 0", "bound", 0, 0);
}

static void refusals() {
  {
    const uint32_t a[] = {0, 4, 5, 9, 2};
    expect(first_outside(a, 5, 10) == 5 && first_outside(a, 5, 9) == 3 &&
               first_outside(a, 5, 5) == 2 && first_outside(a, 5, 0) == 0 &&
               first_outside(a, 0, 0) == 0, "first_outside", "refusals", 0, 0);
    const uint32_t t[] = {5, 9, 2, 9, 5};
    expect(first_duplicate(t, 5) == 3, "a target twice: the second occurrence", "refusals", 0, 0);
  }
  {
    bool ts = false;
    const uint32_t t[] = {10, 11, 12, 13}, s[] = {0, 1, 2, 1};
    expect(first_source_target(t, s, 4, &ts) == 4, "disjoint", "refusals", 0, 0);
    const uint32_t t1[] = {10, 11, 2, 13};           // target 2 is source 2
    expect(first_source_target(t1, s, 4, &ts) == 2 && ts, "the target's position", "refusals", 0, 0);
    const uint32_t s1[] = {0, 13, 2, 1};             // source 13 is target 13 (position 3)
    expect(first_source_target(t, s1, 4, &ts) == 1 && !ts, "the source's position", "refusals", 0, 0);
    const uint32_t t2[] = {7}, s2[] = {7};           // a cluster onto itself
    expect(first_source_target(t2, s2, 1, &ts) == 0 && ts, "onto itself", "refusals", 0, 0);
    expect(first_source_target(t, s, 0) == 0, "empty", "refusals", 0, 0);
    const uint32_t t3[] = {1, 0xFFFFFFFFu}, s3[] = {0xFFFFFFFFu, 5};
    expect(first_source_target(t3, s3, 2, &ts) == 0 && !ts, "the largest id", "refusals", 0, 0);
  }
  {                                          // 10^6 pairs, one cluster on both sides
    const uint32_t n = 1000000;
    std::vector<uint32_t> t = iota(n, n), s(n);
    shuffle(t);
    for (auto& x : s) x = rnd() % n;
    auto seconds = [](auto fn) {
      const auto t0 = std::chrono::steady_clock::now();
      fn();
      return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    const double none = seconds([&] {
      expect(first_source_target(t.data(), s.data(), n) == n, "1e6 disjoint", "refusals", 0, 0);
    });
    s[777777] = t[123456];
    bool ts = false;
    uint32_t at = 0;
    const double one = seconds([&] { at = first_source_target(t.data(), s.data(), n, &ts); });
    expect(at == 123456 && ts, "1e6: the first position, the target's", "refusals", at, ts);
    t[5] = s[999];                                   // an earlier one
    expect(first_source_target(t.data(), s.data(), n, &ts) == 5 && ts, "1e6: an earlier position",
           "refusals", 0, 0);
    // two sorts of 10^6 words and a merge: tens of ms, about 0.35 s under ASan and UBSan at -O1;
    // the n^2 loop would take 10^12 steps. The bound is a second for each call.
    printf("1e6 pairs: %.3f s disjoint, %.3f s with one cluster on both sides\n", none, one);
    expect(none < 1.0 && one < 1.0, "1e6 pairs in under a second", "refusals",
           (long)(none * 1000), (long)(one * 1000));
  }
}

int main() {
  planner();
  refusals();
  printf("checks %ld bad %ld\n", checks, bad);
  return bad ? 1 : 0;
}
"""

CODEC = COMMON + r"""
#include "pack.hpp"

using namespace rs;

static uint32_t rnd32() { return (uint32_t)(rnd() >> 32); }

// ---- hot_clone = hot_field o node_word ------------------------------------------------------------
static void clone_checks(uint32_t N) {
  const uint32_t F = hot_fields(N);
  long differ = 0, draws = 0;
  for (int rep = 0; rep < 200; ++rep) {
    std::vector<uint32_t> h(F * N);
    for (auto& w : h) w = rnd32();
    const DrawKeys dk = {rnd32() % 100000, 1 + rnd32() % 100000, rnd32(), rnd32()};
    const uint32_t g = rnd32(), cc = rnd32();
    for (uint32_t k = 0; k < N; ++k)
      for (int draw = 0; draw < 2; ++draw) {
        uint32_t& fl = h[HF_FLAGS * N + k];
        fl = draw ? fl | FL_DRAW : fl & ~FL_DRAW;
        uint32_t nw[NODE_WORDS];
        for (uint32_t w = 0; w < NODE_WORDS; ++w) nw[w] = node_word(&h[k], N, w, cc, g, k, dk);
        for (uint32_t f = 0; f < F; ++f) {
          if (hf_is_queue(f)) continue;
          const uint32_t got = hot_clone(&h[k], N, f, g, k, dk);
          expect(got == hot_field(nw, N, f), "hot_clone is hot_field of node_word", "codec", N, f);
          if (f == HF_FLAGS) expect(!(got & FL_DRAW), "FL_DRAW is clear", "codec", N, k);
        }
        if (draw) {
          ++draws;
          differ += hot_clone(&h[k], N, HF_DEADLINE, g, k, dk) !=
                    hot_clone(&h[k], N, HF_DEADLINE, g + 1 + k, k, dk);
        } else {
          expect(hot_clone(&h[k], N, HF_DEADLINE, g, k, dk) == h[HF_DEADLINE * N + k],
                 "no draw owed: the stored deadline", "codec", N, k);
        }
      }
  }
  expect(differ * 10 > draws * 9, "another cluster id draws another deadline", "codec", differ, draws);
}

// ---- ring_words (count, first, last) = ring_words (pointer) ---------------------------------------
static void ring_checks() {
  for (uint32_t Q = 1; Q <= RAFT_MAX_INBOX; ++Q)
    for (int rep = 0; rep < 8; ++rep) {
      // a node's two rings as the device holds them, and as a pack holds them: head first
      std::vector<uint32_t> ring[2], lin[2];
      uint32_t head[2], first[2], last[2];
      for (uint32_t cq = 0; cq <= Q; ++cq)
        for (uint32_t cs = 0; cs <= Q; ++cs) {
          const uint32_t cnt[2] = {cq, cs};
          for (int which = 0; which < 2; ++which) {
            ring[which].assign(Q * MSG_WORDS, 0);
            lin[which].assign(Q * MSG_WORDS, 0);
            for (auto& w : ring[which]) w = rnd32();
            head[which] = rnd() % Q;
            for (uint32_t p = 0; p < cnt[which]; ++p)
              memcpy(&lin[which][p * MSG_WORDS], &ring[which][((head[which] + p) % Q) * MSG_WORDS],
                     MSG_WORDS * 4);
            // the ring's own ends (garbage where the ring is empty: never looked at)
            first[which] = ring[which][head[which] * MSG_WORDS];
            last[which] = ring[which][((head[which] + cnt[which] + Q - 1) % Q) * MSG_WORDS];
            const RingWords a = ring_words(which, cnt[which], lin[which].data());
            const RingWords b = ring_words(which, cnt[which], first[which], last[which]);
            expect(a.mask == b.mask && a.qmeta == b.qmeta && a.arr == b.arr && a.tail == b.tail,
                   "the two forms of ring_words", "rings", Q, cnt[which]);
            expect(b.arr == (cnt[which] ? lin[which][0] : INF) &&
                       b.tail == (cnt[which] ? lin[which][(cnt[which] - 1) * MSG_WORDS] : 0u),
                   "arrival INF and tail 0 when empty", "rings", Q, cnt[which]);
          }
          for (uint32_t f = HF_QMETA; f <= HF_RES_TAIL; ++f)
            expect(queue_field(f, cq, lin[0].data(), cs, lin[1].data()) ==
                       queue_field(f, ring_words(0, cq, first[0], last[0]),
                                   ring_words(1, cs, first[1], last[1])),
                   "the two forms of queue_field", "rings", Q, f);
          expect(queue_field(HF_QMETA, ring_words(0, cq, first[0], last[0]),
                             ring_words(1, cs, first[1], last[1])) == pack_qmeta(0, cq, 0, cs),
                 "qmeta: the counts, heads 0", "rings", cq, cs);
        }
    }
}

// ---- arena_access_bytes ---------------------------------------------------------------------------
constexpr uint32_t AC = 4;                    // clusters per shard
alignas(16) static uint64_t src_arena[AC * 9 * 9 + 2], dst_arena[AC * 9 * 9 + 2];

static void arena_checks(uint32_t N, uint32_t A) {
  const uint32_t entries = N * A, chunks = (entries + 1) >> 1;
  for (uint32_t cs = 0; cs < AC; ++cs)
    for (uint32_t ct = 0; ct < AC; ++ct) {
      for (uint32_t i = 0; i < AC * entries + 2; ++i) {
        src_arena[i] = rnd() | 1;
        dst_arena[i] = 0;
      }
      const uint64_t s0 = (uint64_t)cs * entries, t0 = (uint64_t)ct * entries;
      long wide[2] = {0, 0};
      for (uint32_t i = 0; i < chunks; ++i) {
        const uint32_t e = 2 * i;
        const bool both = e + 1 < entries;
        uint64_t v[2] = {0, 0};
        const uint32_t sb = arena_access_bytes(s0, e, entries), tb = arena_access_bytes(t0, e, entries);
        const bool s16 = ((uintptr_t)&src_arena[s0 + e] & 15) == 0 && both;
        const bool t16 = ((uintptr_t)&dst_arena[t0 + e] & 15) == 0 && both;
        expect((sb == 16 || sb == 8) && (sb == 16) == s16,
               "source: 16 bytes exactly where aligned and both exist", "arena", N * 100 + A, e);
        expect((tb == 16 || tb == 8) && (tb == 16) == t16,
               "target: 16 bytes exactly where aligned and both exist", "arena", N * 100 + A, e);
        if (sb == 16 && s16) memcpy(v, &src_arena[s0 + e], 16);      // one aligned access
        else {
          v[0] = src_arena[s0 + e];
          if (both) v[1] = src_arena[s0 + e + 1];
        }
        if (tb == 16 && t16) memcpy(&dst_arena[t0 + e], v, 16);
        else {
          dst_arena[t0 + e] = v[0];
          if (both) dst_arena[t0 + e + 1] = v[1];
        }
        wide[0] += sb == 16;
        wide[1] += tb == 16;
      }
      for (uint32_t i = 0; i < AC * entries + 2; ++i) {
        const bool in = i >= t0 && i < t0 + entries;
        expect(dst_arena[i] == (in ? src_arena[s0 + (i - t0)] : 0),
               "the target's entries are the source's, nothing else is written", "arena", ct, i);
      }
      // an even first slot moves every whole pair wide, an odd one none
      expect(wide[0] == (s0 & 1 ? 0 : entries / 2) && wide[1] == (t0 & 1 ? 0 : entries / 2),
             "wide accesses by parity", "arena", cs, ct);
    }
  if (entries & 1)
    expect(arena_access_bytes(0, entries - 1, entries) == 8 &&
               arena_access_bytes(1, entries - 1, entries) == 8,
           "the last entry of an odd total moves alone", "arena", N, A);
}

// ---- stream_slot_kept = scatter o gather ----------------------------------------------------------
static void stream_checks() {
  for (uint32_t SC = 1; SC <= 17; ++SC) {
    std::vector<uint32_t> ccs;
    for (uint32_t cc = 0; cc <= 3 * SC + 1; ++cc) ccs.push_back(cc);
    for (uint32_t cc : {1000003u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu}) ccs.push_back(cc);
    for (int rep = 0; rep < 20; ++rep) ccs.push_back(rnd32());
    for (uint32_t cc : ccs) {
      std::vector<uint32_t> ring(SC), rec(SC), tgt(SC);
      for (auto& w : ring) w = rnd32() | 1;
      const uint32_t kept = std::min(cc, SC);
      for (uint32_t p = 0; p < SC; ++p)          // gather_kernel: the newest values, oldest first
        rec[p] = p < kept ? ring[(cc - kept + p) % SC] : 0u;
      for (uint32_t s = 0; s < SC; ++s) {        // scatter_kernel: the ring, rotated back
        const uint32_t p = (s + SC - (cc - kept) % SC) % SC;
        tgt[s] = p < kept ? rec[p] : 0u;
      }
      uint32_t n_kept = 0;
      for (uint32_t s = 0; s < SC; ++s) {
        const bool k = stream_slot_kept(s, cc, SC);
        n_kept += k;
        expect(tgt[s] == (k ? ring[s] : 0u), "slot s from slot s where kept, else 0", "streams", SC, cc);
      }
      expect(n_kept == kept, "min(commit_count, SC) slots are kept", "streams", SC, cc);
    }
  }
}

int main() {
  for (uint32_t N = 2; N <= RAFT_MAX_NODES; ++N) {
    clone_checks(N);
    for (uint32_t A : {1u, 4u, 5u, 8u, 9u}) arena_checks(N, A);
  }
  ring_checks();
  stream_checks();
  printf("checks %ld bad %ld\n", checks, bad);
  return bad ? 1 : 0;
}
"""


def test_the_planner_places_every_pair_once_and_the_refusals_name_the_first_position(tmp_path):
    out = hostprog.run_cpp(tmp_path, "clone_plan_check", PLANNER,
                           sanitizers=("undefined", "address"), timeout=300)
    print(out[-400:])
    assert hostprog.checks(out) > 1000000


def test_the_codec_the_arena_width_and_the_stream_rule(tmp_path):
    out = hostprog.run_cpp(tmp_path, "clone_codec_check", CODEC, compiler="hipcc",
                           sanitizers=("address", "undefined"), timeout=300)
    assert hostprog.checks(out) > 100000
