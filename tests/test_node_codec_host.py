"""csrc/node_codec.hpp on the CPU: the hot block <-> raft_node_t mapping that raft_sim_read_nodes,
raft_sim_write_nodes, raft_sim_write_queue, gather_kernel and scatter_kernel share.

A stand-alone C++ program (its own main) is compiled for the host alone with hipcc (the header needs
HIP's vector types, no device) -- under ASan and UBSan where the compiler has their runtimes -- and
run once. Its reference is a decode and an encode of raft_node_t by member name, through
include/raftsim.h's members and device.hpp's HF_* / hf_* / fl_* / qm_* accessors only: no word
number. For N = 2..9, 48 clusters of random records each that node_record_ok accepts, and the
extreme values of every packed field (device.hpp's packed_check):

1. decode: all 34 words of every node of a block the reference encoded give the record byte for
   byte, padding and reserved0 zero; a distinct value planted in one hot field of one node changes
   the decoded records exactly as the reference says, and no other node's;
2. encode: over blocks of equal garbage the encoder's block equals the reference's word for word,
   cluster words, queue words and the trailing pad untouched;
3. round trips: decode(encode(record)) is the record, encode(decode(block)) the block's node fields;
4. an owed draw (FL_DRAW) decodes to exact_deadline of the *global* cluster id (the offset is not 0,
   and most draws differ from the shard-local id's), the flag bytes are those without bit 15, and
   with the flag clear the stored word is returned;
5. queue words: counts 0, 1 and Q on each side give pack_qmeta(0, rq, 0, rs), arrival INF / the
   first message's, tail 0 / the last one's; putting one ring into HF_QMETA keeps the other's head
   and count."""
import hostprog

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "node_codec.hpp"
#include "scatter_host.hpp"

using namespace rs;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd() {                      // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t rnd32() { return (uint32_t)(rnd() >> 32); }

static long checks = 0, bad = 0;
static void expect(bool ok, const char* what, long a, long b, long c) {
  ++checks;
  if (!ok && bad++ < 20) printf("MISMATCH %s at N %ld, node %ld, %ld\n", what, a, b, c);
}

// ---- the reference: by member name ---------------------------------------------------------------
// h: the node's first hot word, field f at h[f * N]
static raft_node_t ref_decode(const uint32_t* h, uint32_t N, uint32_t cc, uint32_t g, uint32_t k,
                              const DrawKeys& dk) {
  auto f = [&](uint32_t fld) { return h[fld * N]; };
  raft_node_t r;
  memset(&r, 0, sizeof r);
  const uint32_t fl = f(HF_FLAGS), mk = f(HF_MASKS), qm = f(HF_QMETA);
  r.role = fl_role(fl); r.voted_for = fl_vf(fl); r.leader_id = fl_lid(fl);
  r.fault = fl_fault(fl); r.entries_is_seq = fl_seq(fl); r.ls_present = fl_lsp(fl);
  r.votes = mk & 0xFFFF; r.ls_keys = mk >> 16;
  r.current_term = f(HF_TERM); r.commit_index = f(HF_COMMIT);
  r.log_len = f(HF_LEN); r.deadline = f(HF_DEADLINE);
  if (fl & FL_DRAW)            // a deferred timer draw still owed in the stored state
    r.deadline = exact_deadline(g, k + 1, r.deadline, dk.el_base, dk.el_span, dk.key0, dk.key1);
  for (uint32_t p = 0; p < N; ++p) {
    r.next_index[p] = (int32_t)f(HF_NEXT + p);
    r.match_index[p] = (int32_t)f(HF_NEXT + N + p);
  }
  r.last_led_term = f(hf_led(N));
  r.arena_base = f(hf_abase(N)); r.arena_frontier = f(hf_afront(N));
  r.req_count = qm_req_cnt(qm); r.res_count = qm_res_cnt(qm);
  r.trace_hash = (uint64_t)f(HF_TRACE_HI) << 32 | f(HF_TRACE_LO);
  r.commit_count = cc;
  return r;
}
static void ref_encode(const raft_node_t& r, uint32_t* h, uint32_t N) {
  auto f = [&](uint32_t fld) -> uint32_t& { return h[fld * N]; };
  f(HF_FLAGS) = pack_flags(r.role, r.voted_for, r.leader_id, r.fault, r.entries_is_seq,
                           r.ls_present);
  f(HF_MASKS) = r.votes | (uint32_t)r.ls_keys << 16;
  f(HF_TERM) = r.current_term; f(HF_COMMIT) = r.commit_index;
  f(HF_LEN) = r.log_len; f(HF_DEADLINE) = r.deadline;
  f(hf_abase(N)) = r.arena_base; f(hf_afront(N)) = r.arena_frontier;
  f(hf_led(N)) = r.last_led_term;
  f(HF_TRACE_LO) = (uint32_t)r.trace_hash; f(HF_TRACE_HI) = (uint32_t)(r.trace_hash >> 32);
  for (uint32_t p = 0; p < N; ++p) {
    f(HF_NEXT + p) = (uint32_t)r.next_index[p];
    f(HF_NEXT + N + p) = (uint32_t)r.match_index[p];
  }
}
// the queue words of a node whose record counts rq and rs messages, with ring heads and arrivals
static void ref_queue_words(const raft_node_t& r, uint32_t* h, uint32_t N) {
  h[HF_QMETA * N] = pack_qmeta(rnd() % 16, r.req_count, rnd() % 16, r.res_count);
  for (uint32_t f : {HF_REQ_ARR, HF_RES_ARR, HF_REQ_TAIL, HF_RES_TAIL}) h[f * N] = rnd32();
}

// ---- the codec under test ------------------------------------------------------------------------
static raft_node_t decode(const uint32_t* h, uint32_t N, uint32_t cc, uint32_t g, uint32_t k,
                          const DrawKeys& dk) {
  uint32_t nw[NODE_WORDS];
  for (uint32_t w = 0; w < NODE_WORDS; ++w) nw[w] = node_word(h, N, w, cc, g, k, dk);
  raft_node_t r;
  memcpy(&r, nw, sizeof r);
  return r;
}
static void encode(const raft_node_t& r, uint32_t* h, uint32_t N) {
  uint32_t nw[NODE_WORDS];
  memcpy(nw, &r, sizeof nw);
  for (uint32_t f = 0; f < hot_fields(N); ++f)
    if (!hf_is_queue(f)) h[f * N] = hot_field(nw, N, f);
}
static bool same(const raft_node_t& a, const raft_node_t& b) { return !memcmp(&a, &b, sizeof a); }

// ---- records -------------------------------------------------------------------------------------
constexpr uint32_t L = 64, CLUSTERS = 48, GOFF = 1000003;
static const DrawKeys DK = {5000, 5000, 0x1234ABCDu, 0x9E3779B9u};

// a record node_record_ok accepts (node id of N), every field random inside what it allows
static raft_node_t valid_record(uint32_t id, uint32_t N) {
  const uint32_t all = ((1u << (N + 1)) - 1) & ~1u, peers = all & ~(1u << id);
  raft_node_t r;
  memset(&r, 0, sizeof r);
  r.role = rnd() % 4; r.voted_for = rnd() % (N + 1); r.leader_id = rnd() % (N + 1);
  r.fault = rnd() % 5; r.entries_is_seq = rnd() % 2; r.ls_present = rnd() % 2;
  r.votes = rnd32() & all;
  if (r.role == RAFT_LEADER) r.ls_present = 1;
  r.ls_keys = r.role == RAFT_LEADER ? peers : r.ls_present ? rnd32() & peers : 0;
  r.current_term = rnd32(); r.commit_index = rnd32(); r.deadline = rnd32();
  r.log_len = rnd() % (L + 1);
  r.arena_base = rnd32();                    // frontier - base wraps for some
  r.arena_frontier = r.arena_base + r.log_len + rnd() % (L - r.log_len + 1);
  for (uint32_t p = 0; p < N; ++p) {
    r.next_index[p] = (int32_t)rnd32();
    r.match_index[p] = (int32_t)rnd32();
  }
  r.last_led_term = rnd32();
  r.req_count = rnd() % (RAFT_MAX_INBOX + 1); r.res_count = rnd() % (RAFT_MAX_INBOX + 1);
  r.commit_count = rnd32();
  r.trace_hash = rnd();
  return r;
}
// the largest value of every packed field (packed_check's): outside node_record_ok, inside the codec
static raft_node_t extreme_record(uint32_t N) {
  raft_node_t r;
  memset(&r, 0xFF, sizeof r);
  r.role = 3; r.voted_for = 15; r.leader_id = 15; r.fault = 7; r.entries_is_seq = 1;
  r.ls_present = 1; r.reserved0 = 0; r.req_count = 31; r.res_count = 31;
  for (uint32_t p = N; p < RAFT_MAX_NODES; ++p) r.next_index[p] = r.match_index[p] = 0;
  uint32_t nw[NODE_WORDS];                   // the padding before trace_hash
  memcpy(nw, &r, sizeof nw);
  nw[NW_COMMIT_COUNT + 1] = 0;
  memcpy(&r, nw, sizeof r);
  return r;
}

struct Shard {
  uint32_t N, HB;
  std::vector<raft_node_t> rec;              // [CLUSTERS][N]
  std::vector<uint32_t> blk;                 // [CLUSTERS][HB], by the reference
  uint32_t* node(uint32_t c, uint32_t k) { return &blk[(size_t)c * HB + HOT_CW + k]; }
};
static Shard make_shard(uint32_t N) {
  Shard s = {N, hot_block_words(N), {}, {}};
  s.blk.resize((size_t)CLUSTERS * s.HB);
  for (auto& w : s.blk) w = rnd32();         // cluster words and pad: anything
  for (uint32_t c = 0; c < CLUSTERS; ++c)
    for (uint32_t k = 0; k < N; ++k) {
      const raft_node_t r = c == 7 ? extreme_record(N) : valid_record(k + 1, N);
      expect(c == 7 || node_record_ok(r, k + 1, N, L), "the generator makes valid records", N, k, c);
      s.rec.push_back(r);
      ref_encode(r, s.node(c, k), N);
      ref_queue_words(r, s.node(c, k), N);
    }
  return s;
}

// ---- 1. decode, 3. round trips -------------------------------------------------------------------
static void decode_checks(Shard& s) {
  const uint32_t N = s.N;
  for (uint32_t c = 0; c < CLUSTERS; ++c)
    for (uint32_t k = 0; k < N; ++k) {
      const raft_node_t& want = s.rec[c * N + k];
      const raft_node_t got = decode(s.node(c, k), N, want.commit_count, GOFF + c, k, DK);
      expect(same(got, want), "decode gives the record", N, k, c);
      expect(same(got, ref_decode(s.node(c, k), N, want.commit_count, GOFF + c, k, DK)),
             "decode agrees with the reference", N, k, c);
      expect(got.reserved0 == 0 && node_word(s.node(c, k), N, NW_COMMIT_COUNT + 1, 1, 0, k, DK) == 0,
             "reserved bytes and padding are zero", N, k, c);
      // encode(decode(block)) on the node-record fields (FL_DRAW is clear in an encoded block)
      std::vector<uint32_t> again(s.blk.begin() + (size_t)c * s.HB,
                                  s.blk.begin() + (size_t)(c + 1) * s.HB);
      for (uint32_t f = 0; f < hot_fields(N); ++f)
        if (!hf_is_queue(f)) again[HOT_CW + f * N + k] = ~again[HOT_CW + f * N + k];
      encode(got, &again[HOT_CW + k], N);
      expect(!memcmp(again.data(), &s.blk[(size_t)c * s.HB], s.HB * 4), "encode(decode(block))", N,
             k, c);
    }
  // a distinct value in one hot field of one node: what the reference says changes, nothing else
  for (uint32_t c : {3u, 7u, 20u})
    for (uint32_t k = 0; k < N; ++k)
      for (uint32_t f = 0; f < hot_fields(N); ++f) {
        uint32_t& word = s.node(c, k)[f * N];
        const uint32_t old = word;
        word = rnd32() | (f == HF_FLAGS && (rnd() & 1) ? FL_DRAW : 0u);
        if (word == old) word = ~old;
        bool changed = false;
        for (uint32_t j = 0; j < N; ++j) {
          const uint32_t cc = s.rec[c * N + j].commit_count;
          const raft_node_t got = decode(s.node(c, j), N, cc, GOFF + c, j, DK);
          expect(same(got, ref_decode(s.node(c, j), N, cc, GOFF + c, j, DK)),
                 "a planted field decodes as the reference says", N, j, f);
          if (j != k) expect(same(got, s.rec[c * N + j]), "no other node's record changes", N, j, f);
          else changed = !same(got, s.rec[c * N + j]);
        }
        // every field shows in the record, unless the planted bits are ones no member holds
        const bool visible = !(f == HF_FLAGS || f == HF_QMETA || f == HF_REQ_ARR ||
                               f == HF_RES_ARR || f == HF_REQ_TAIL || f == HF_RES_TAIL);
        if (visible) expect(changed, "a planted field shows in its node's record", N, k, f);
        word = old;
      }
}

// ---- 2. encode -----------------------------------------------------------------------------------
static void encode_checks(const Shard& s) {
  const uint32_t N = s.N;
  std::vector<uint32_t> a(s.blk.size()), b;
  for (auto& w : a) w = rnd32();
  b = a;
  const std::vector<uint32_t> garbage = a;
  for (uint32_t c = 0; c < CLUSTERS; ++c)
    for (uint32_t k = 0; k < N; ++k) {
      ref_encode(s.rec[c * N + k], &a[(size_t)c * s.HB + HOT_CW + k], N);
      encode(s.rec[c * N + k], &b[(size_t)c * s.HB + HOT_CW + k], N);
      const raft_node_t back =
          decode(&b[(size_t)c * s.HB + HOT_CW + k], N, s.rec[c * N + k].commit_count, GOFF + c, k, DK);
      raft_node_t want = s.rec[c * N + k];   // the queue words are garbage: so are the counts
      want.req_count = back.req_count;
      want.res_count = back.res_count;
      expect(same(back, want), "decode(encode(record))", N, k, c);
    }
  expect(a == b, "the encoder's blocks are the reference's, word for word", N, 0, 0);
  for (uint32_t c = 0; c < CLUSTERS; ++c) {
    const size_t o = (size_t)c * s.HB;
    for (uint32_t w = 0; w < s.HB; ++w) {
      const uint32_t f = w < HOT_CW ? 0 : (w - HOT_CW) / N;
      const bool node_field = w >= HOT_CW && f < hot_fields(N) && f != HF_QMETA && f != HF_REQ_ARR &&
                              f != HF_RES_ARR && f != HF_REQ_TAIL && f != HF_RES_TAIL;
      if (!node_field)
        expect(b[o + w] == garbage[o + w], "cluster, queue and pad words are untouched", N, c, w);
    }
  }
}

// ---- 4. the owed draw ----------------------------------------------------------------------------
static void draw_checks(Shard& s) {
  const uint32_t N = s.N;
  long differ = 0, draws = 0;
  for (uint32_t c = 0; c < CLUSTERS; ++c)
    for (uint32_t k = 0; k < N; ++k) {
      uint32_t* const h = s.node(c, k);
      const uint32_t fl = h[HF_FLAGS * N], stored = h[HF_DEADLINE * N], g = GOFF + c;
      expect(!(fl & FL_DRAW) && node_word(h, N, NW_DEADLINE, 0, g, k, DK) == stored,
             "flag clear: the stored word", N, k, c);
      const uint32_t w0 = node_word(h, N, NW_ROLE, 0, g, k, DK), w1 = node_word(h, N, NW_SEQ, 0, g, k, DK);
      h[HF_FLAGS * N] = fl | FL_DRAW;
      const uint32_t want = exact_deadline(g, k + 1, stored, DK.el_base, DK.el_span, DK.key0, DK.key1);
      expect(node_word(h, N, NW_DEADLINE, 0, g, k, DK) == want, "flag set: the exact deadline", N, k, c);
      expect(node_word(h, N, NW_ROLE, 0, g, k, DK) == w0 && node_word(h, N, NW_SEQ, 0, g, k, DK) == w1,
             "the flag is not in the record's bytes", N, k, c);
      ++draws;
      differ += want != exact_deadline(c, k + 1, stored, DK.el_base, DK.el_span, DK.key0, DK.key1);
      h[HF_FLAGS * N] = fl;
    }
  expect(differ * 10 > draws * 9, "the shard-local id draws another deadline", N, differ, draws);
}

// ---- 5. queue words ------------------------------------------------------------------------------
static void queue_checks() {
  for (uint32_t Q = 1; Q <= RAFT_MAX_INBOX; ++Q) {
    std::vector<raft_msg_t> m(2 * Q);        // a node's REQ ring, then its RES ring, as a pack has them
    for (auto& x : m) {
      x.arrival = rnd32() | 1;
      x.hdr = x.term = x.a = x.b = x.eterm = x.eval = x.poff = rnd32();
    }
    const uint32_t* const rq = reinterpret_cast<const uint32_t*>(m.data());
    const uint32_t* const rs = reinterpret_cast<const uint32_t*>(m.data() + Q);
    for (uint32_t nq : {0u, 1u, Q})
      for (uint32_t ns : {0u, 1u, Q}) {
        const RingWords a = ring_words(0, nq, rq), b = ring_words(1, ns, rs);
        expect(queue_field(HF_QMETA, nq, rq, ns, rs) == pack_qmeta(0, nq, 0, ns) &&
                   (a.qmeta | b.qmeta) == pack_qmeta(0, nq, 0, ns), "qmeta: the counts, heads 0", Q, nq, ns);
        const uint32_t arr_q = nq ? m[0].arrival : INF, arr_s = ns ? m[Q].arrival : INF;
        const uint32_t tail_q = nq ? m[nq - 1].arrival : 0, tail_s = ns ? m[Q + ns - 1].arrival : 0;
        expect(a.arr == arr_q && queue_field(HF_REQ_ARR, nq, rq, ns, rs) == arr_q &&
                   b.arr == arr_s && queue_field(HF_RES_ARR, nq, rq, ns, rs) == arr_s,
               "arrival: the first message's, INF when empty", Q, nq, ns);
        expect(a.tail == tail_q && queue_field(HF_REQ_TAIL, nq, rq, ns, rs) == tail_q &&
                   b.tail == tail_s && queue_field(HF_RES_TAIL, nq, rq, ns, rs) == tail_s,
               "tail: the last message's, 0 when empty", Q, nq, ns);
        // one ring put into a node's HF_QMETA: the other ring's head and count stay
        const uint32_t h0 = rnd() % 16, c0 = rnd() % 32, h1 = rnd() % 16, c1 = rnd() % 32;
        const uint32_t qm = pack_qmeta(h0, c0, h1, c1);
        expect(with_ring(qm, a) == pack_qmeta(0, nq, h1, c1) &&
                   with_ring(qm, b) == pack_qmeta(h0, c0, 0, ns), "the other ring's half stays", Q, nq, ns);
      }
    expect(ring_words(0, 0, nullptr).arr == INF && ring_words(1, 0, nullptr).tail == 0,
           "an empty ring reads no message", Q, 0, 0);
  }
}

int main() {
  for (uint32_t N = 2; N <= RAFT_MAX_NODES; ++N) {
    Shard s = make_shard(N);
    decode_checks(s);
    encode_checks(s);
    draw_checks(s);
  }
  queue_checks();
  printf("checks %ld bad %ld\n", checks, bad);
  return bad ? 1 : 0;
}
"""


def test_the_codec_is_the_by_member_mapping_in_both_directions(tmp_path):
    out = hostprog.run_cpp(tmp_path, "codec_check", PROGRAM, compiler="hipcc",
                           sanitizers=("address", "undefined"))
    assert hostprog.checks(out) > 50000
