"""The host-compilable half of raft_restart_write / raft_restart_where on the CPU:
csrc/restart_host.hpp (the list checks, the timer's horizon and the planner) and hot_restart of
csrc/node_codec.hpp, the one function both restart kernels take every hot word from.

Two stand-alone C++ programs (each its own main), compiled under ASan and UBSan where the compiler
has their runtimes and run once; each ends `checks N bad 0`.

1. The planner (g++, the header and include/raftsim.h alone). For random lists over 1..4 shards
   with bounds of 1, 2, 7 and random pairs: every position of the caller's lists lies in exactly
   one chunk, as its cluster's shard-local id of the chunk's shard with its own mask; a chunk
   holds 1..bound pairs; chunks tile the pairs shard by shard; no cut is early; the plan's node
   count is the popcount sum of the masks. Every refusal names its first position (an id outside
   the handle, a cluster named twice, a mask that is 0 or names a node the cluster does not have),
   in the order the call makes the checks. A 10^6-pair list is checked and planned within a second.
   The horizon predicate at its edge.

2. The hot-word function (hipcc, host only). N = 2..9, both modes, random 32-bit hot words with
   FL_DRAW set and clear, random ticks: node_word of the restarted hot words equals a restatement
   of raftsim.restart_record on the record node_word gives before the restart, member by member
   (the deadline recomputed from Philox with the INIT purpose and the restart tick), FL_DRAW is
   clear, and the five queue words equal queue_field of two empty rings."""
import hostprog
from test_clone_host import COMMON

PLANNER = COMMON + r"""
#include "restart_host.hpp"

using namespace rs;

static std::vector<uint32_t> shards(uint32_t C, uint32_t G) {
  std::vector<uint32_t> lo(G + 1);
  for (uint32_t d = 0; d <= G; ++d) lo[d] = (uint32_t)((uint64_t)C * d / G);
  return lo;
}
static void shuffle(std::vector<uint32_t>& v) {
  for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rnd() % i]);
}
static uint16_t some_mask(uint32_t N) {
  const uint32_t ids = restart_ids(N);
  uint32_t m = 0;
  while (!m) m = (uint32_t)rnd() & ids;
  return (uint16_t)m;
}

static void check_plan(const char* who, const std::vector<uint32_t>& cl,
                       const std::vector<uint16_t>& masks, const std::vector<uint32_t>& lo,
                       uint64_t bound) {
  const uint32_t n = (uint32_t)cl.size(), G = (uint32_t)lo.size() - 1;
  const RestartPlan p = restart_plan(cl.data(), masks.data(), n, lo.data(), G, bound);
  expect(p.pairs.size() == n && p.pos.size() == n, "a pair per position", who, n, 0);
  if (p.pairs.size() != n || p.pos.size() != n) return;
  std::vector<uint8_t> seen(n, 0);
  size_t next_pair = 0;
  uint64_t nodes = 0;
  for (size_t ci = 0; ci < p.chunks.size(); ++ci) {
    const RestartChunk& c = p.chunks[ci];
    expect(c.pair0 == next_pair, "chunks tile the pairs", who, ci, 0);
    expect(c.pairs >= 1 && c.pairs <= bound, "1..bound pairs", who, ci, c.pairs);
    next_pair = c.pair0 + c.pairs;
    if (next_pair > n || c.shard >= G) {
      expect(false, "chunk leaves the lists or the shards", who, ci, 0);
      return;
    }
    if (ci) {
      const RestartChunk& b = p.chunks[ci - 1];
      expect(b.shard <= c.shard, "shard by shard", who, ci, 0);
      if (b.shard == c.shard) expect(b.pairs == bound, "no early cut", who, ci, b.pairs);
    }
    for (size_t i = c.pair0; i < next_pair; ++i) {
      const uint32_t pos = p.pos[i];
      if (pos >= n) {
        expect(false, "a position of the lists", who, ci, i);
        continue;
      }
      expect(!seen[pos], "a pair lies in one chunk only", who, pos, ci);
      seen[pos] = 1;
      const uint32_t x = cl[pos];
      expect(x >= lo[c.shard] && x < lo[c.shard + 1] && p.pairs[i].cluster == x - lo[c.shard],
             "the cluster is its shard's local one", who, pos, x);
      expect(p.pairs[i].mask == masks[pos], "the pair carries its own mask", who, pos, masks[pos]);
      nodes += (uint64_t)__builtin_popcount(masks[pos]);
    }
  }
  expect(next_pair == n, "chunks cover the pairs", who, n, 0);
  for (uint32_t i = 0; i < n; ++i) expect(seen[i], "every pair lies in a chunk", who, i, 0);
  expect(p.nodes == nodes, "the nodes named", who, (long)p.nodes, (long)nodes);
}

int main() {
  const uint64_t bounds[] = {1, 2, 7};
  for (int rep = 0; rep < 600; ++rep) {
    const uint32_t G = 1 + rnd() % 4, C = G + rnd() % 400, N = 2 + rnd() % 8, n = rnd() % (C + 1);
    std::vector<uint32_t> cl(C);
    for (uint32_t i = 0; i < C; ++i) cl[i] = i;
    shuffle(cl);
    cl.resize(n);
    std::vector<uint16_t> masks(n);
    for (auto& m : masks) m = some_mask(N);
    const uint64_t bound = rep % 4 < 3 ? bounds[rep % 4] : 1 + rnd() % 64;
    check_plan("random", cl, masks, shards(C, G), bound);
    uint32_t at = 12345;
    expect(restart_list_fault(cl.data(), masks.data(), n, C, N, &at) == RESTART_OK && at == n,
           "a good list passes", "random", rep, at);
    if (n < 3) continue;
    // every refusal's first position: two offenders of a kind, the earlier one is named
    const uint32_t a = rnd() % (n - 1), b = a + 1 + rnd() % (n - 1 - a);
    {
      std::vector<uint32_t> bad = cl;
      bad[a] = C + rnd() % 5;
      bad[b] = C;
      expect(restart_list_fault(bad.data(), masks.data(), n, C, N, &at) == RESTART_OUTSIDE && at == a,
             "outside: first position", "refusal", a, at);
    }
    {
      std::vector<uint32_t> bad = cl;
      bad[b] = bad[a];
      expect(restart_list_fault(bad.data(), masks.data(), n, C, N, &at) == RESTART_TWICE && at == b,
             "twice: the second occurrence", "refusal", b, at);
      // ... and a bad mask behind it does not hide it, an id outside before it does
      std::vector<uint16_t> bm = masks;
      bm[0] = 0;
      expect(restart_list_fault(bad.data(), bm.data(), n, C, N, &at) == RESTART_TWICE && at == b,
             "twice before masks", "refusal", b, at);
      bad[n - 1] = C;
      expect(restart_list_fault(bad.data(), bm.data(), n, C, N, &at) == RESTART_OUTSIDE &&
                 at == n - 1,
             "outside before twice", "refusal", n - 1, at);
    }
    {
      std::vector<uint16_t> bm = masks;
      const int kind = rep % 3;
      bm[a] = kind == 0 ? 0 : kind == 1 ? (uint16_t)(masks[a] | 1u) : (uint16_t)(1u << (N + 1));
      bm[b] = 0;
      expect(restart_list_fault(cl.data(), bm.data(), n, C, N, &at) == RESTART_MASK && at == a,
             "mask: first position", "refusal", a, at);
    }
  }
  for (uint32_t N = 2; N <= 9; ++N) {          // every mask of 16 bits against the rule's words
    for (uint32_t m = 0; m < 65536; ++m) {
      const uint16_t mm = (uint16_t)m;
      bool ok = m != 0;
      for (uint32_t j = 0; j < 16; ++j) ok = ok && (!((m >> j) & 1) || (j >= 1 && j <= N));
      expect((first_bad_mask(&mm, 1, N) == 1) == ok, "mask rule", "all masks", N, m);
    }
  }
  {                                            // 10^6 pairs: checked and planned within a second
    const uint32_t n = 1000000, C = 3000000;
    std::vector<uint32_t> cl(n);
    std::vector<uint16_t> masks(n);
    for (uint32_t i = 0; i < n; ++i) cl[i] = 3 * i + (uint32_t)(rnd() % 3);
    shuffle(cl);
    for (auto& m : masks) m = some_mask(5);
    const std::vector<uint32_t> lo = shards(C, 3);
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t at = 0;
    const RestartFault f = restart_list_fault(cl.data(), masks.data(), n, C, 5, &at);
    const RestartPlan p = restart_plan(cl.data(), masks.data(), n, lo.data(), 3, 1ull << 23);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("1e6 pairs checked and planned in %.3f s, %zu chunks\n", sec, p.chunks.size());
    expect(f == RESTART_OK, "the 1e6 list passes", "1e6", at, 0);
    expect(sec < 1.0, "within a second", "1e6", (long)(sec * 1000), 0);
    expect(p.chunks.size() == 3, "one chunk a shard", "1e6", (long)p.chunks.size(), 0);
    check_plan("1e6", cl, masks, lo, 1ull << 23);
    check_plan("1e6 cut", cl, masks, lo, 65536);
    cl[n - 1] = cl[7];
    expect(restart_list_fault(cl.data(), masks.data(), n, C, 5, &at) == RESTART_TWICE && at == n - 1,
           "a cluster twice in 1e6", "1e6", at, 0);
  }
  // the horizon: T + el_base + el_span must stay below 2^32 - 1
  expect(restart_horizon_ok(0, 500, 500), "horizon", "low", 0, 0);
  expect(restart_horizon_ok(0xFFFFFFFFull - 1001, 500, 500), "horizon", "last", 0, 0);
  expect(!restart_horizon_ok(0xFFFFFFFFull - 1000, 500, 500), "horizon", "first refused", 0, 0);
  expect(!restart_horizon_ok(0xFFFFFFFFull, 0, 0), "horizon", "never", 0, 0);
  expect(!restart_horizon_ok(1, 0xFFFFFFFFu, 0xFFFFFFFFu), "horizon", "no wrap", 0, 0);
  printf("checks %ld bad %ld\n", checks, bad);
  return bad != 0;
}
"""

CODEC = COMMON + r"""
#include "node_codec.hpp"

using namespace rs;

// raftsim.restart_record on the record before the restart, member by member
static raft_node_t restart_record(const raft_node_t& b, uint32_t mode, uint32_t T, uint32_t g,
                                  uint32_t id, const DrawKeys& dk) {
  raft_node_t r = b;
  r.role = 0; r.leader_id = 0; r.votes = 0; r.ls_present = 0; r.ls_keys = 0; r.fault = 0;
  r.commit_index = 0; r.entries_is_seq = 0; r.req_count = 0; r.res_count = 0;
  for (int p = 0; p < RAFT_MAX_NODES; ++p) r.next_index[p] = r.match_index[p] = 0;
  const uint4 w = philox(g, id | 1u << 8, T, 0, dk.key0, dk.key1);     // INIT = 1
  r.deadline = T + dk.el_base + (uint32_t)(((uint64_t)w.y * dk.el_span) >> 32);
  if (mode == RAFT_RESTART_AMNESIA) {
    r.current_term = 1; r.voted_for = 0; r.log_len = 0; r.arena_base = b.arena_frontier;
  }
  return r;
}

int main() {
  for (uint32_t N = 2; N <= RAFT_MAX_NODES; ++N) {
    const uint32_t F = hot_fields(N);
    for (int rep = 0; rep < 4000; ++rep) {
      const uint32_t k = rnd() % N, mode = rep & 1, g = (uint32_t)rnd(), cc = (uint32_t)rnd();
      const DrawKeys dk = {(uint32_t)(rnd() % 5000), (uint32_t)(1 + rnd() % 5000), (uint32_t)rnd(),
                           (uint32_t)rnd()};
      const uint32_t T = rep % 7 == 0 ? 0u : (uint32_t)(rnd() % 0xFFFF0000ull);
      std::vector<uint32_t> hot(F * N), after(F * N);
      for (auto& w : hot) w = (uint32_t)rnd();
      uint32_t* const h = hot.data() + k;
      h[HF_FLAGS * N] = (h[HF_FLAGS * N] & ~FL_DRAW) | ((rep >> 1) & 1 ? FL_DRAW : 0u);
      if (h[HF_FLAGS * N] & FL_DRAW) h[HF_DEADLINE * N] |= 0x80000000u;   // lb - el_base stays >= 0
      after = hot;
      // as the kernels do it: in place, field after field, the node's own words alone
      uint32_t* const a = after.data() + k;
      for (uint32_t f = 0; f < F; ++f) a[f * N] = hot_restart(a, N, f, mode, T, g, k, dk);
      for (uint32_t i = 0; i < F * N; ++i)
        if (i % N != k) expect(after[i] == hot[i], "another node's word", "codec", N, i);
      expect(!(a[HF_FLAGS * N] & ~(FL_ROLE | FL_VF | FL_LID | FL_FAULT | FL_SEQ | FL_LSP)),
             "FL_DRAW and the unused bits are clear", "codec", N, rep);
      raft_node_t before, got, want;
      uint32_t nw[NODE_WORDS];
      for (uint32_t w = 0; w < NODE_WORDS; ++w) nw[w] = node_word(h, N, w, cc, g, k, dk);
      memcpy(&before, nw, sizeof nw);
      for (uint32_t w = 0; w < NODE_WORDS; ++w) nw[w] = node_word(a, N, w, cc, g, k, dk);
      memcpy(&got, nw, sizeof nw);
      want = restart_record(before, mode, T, g, k + 1, dk);
      expect(memcmp(&got, &want, sizeof got) == 0, "the record after the restart", "codec", N, rep);
      if (memcmp(&got, &want, sizeof got) != 0 && bad < 5)
        printf("  mode %u term %u/%u vf %u/%u len %u/%u base %u/%u dl %u/%u led %u/%u\n", mode,
               got.current_term, want.current_term, got.voted_for, want.voted_for, got.log_len,
               want.log_len, got.arena_base, want.arena_base, got.deadline, want.deadline,
               got.last_led_term, want.last_led_term);
      // kept whatever the mode: the checker's memory, the trace hash, the frontier, commit_count
      expect(got.last_led_term == before.last_led_term && got.trace_hash == before.trace_hash &&
                 got.arena_frontier == before.arena_frontier && got.commit_count == cc,
             "kept", "codec", N, rep);
      // the emptied rings: queue_field of two empty rings, head 0
      const uint32_t none = 0;
      for (uint32_t f = HF_QMETA; f <= HF_RES_TAIL; ++f)
        expect(a[f * N] == queue_field(f, 0, &none, 0, &none), "an empty ring's word", "codec", N, f);
      expect(a[HF_QMETA * N] == 0 && a[HF_REQ_ARR * N] == INF && a[HF_RES_ARR * N] == INF &&
                 a[HF_REQ_TAIL * N] == 0 && a[HF_RES_TAIL * N] == 0,
             "count 0, head 0, never, tail 0", "codec", N, rep);
    }
  }
  printf("checks %ld bad %ld\n", checks, bad);
  return bad != 0;
}
"""


def test_planner_and_list_checks(tmp_path):
    out = hostprog.run_cpp(tmp_path, "restart_planner", PLANNER, sanitizers=("address", "undefined"))
    print(out)
    assert hostprog.checks(out) > 10 ** 6


def test_hot_restart_against_the_record_restatement(tmp_path):
    out = hostprog.run_cpp(tmp_path, "restart_codec", CODEC, compiler="hipcc",
                           sanitizers=("address", "undefined"))
    print(out)
    assert hostprog.checks(out) > 10 ** 5
