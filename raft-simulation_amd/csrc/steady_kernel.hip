// steady_kernel.hip — the steady-state kernel of LITE launches for gfx950 (MI355X).
//
// In a LITE launch (no client traffic, no faults, fixed delay: BASELINE config 2) a cluster that
// has elected its leader repeats one heartbeat round forever: the leader's heartbeat broadcasts an
// empty append-entries (heartbeat-handler, core.clj:162-164; append-entries-rpc 56-67), every
// follower answers it (append-entries-handler 105-123) and the leader takes the answers, one per
// tick (append-response-handler 141-149). This kernel runs exactly those events, bit for bit as
// the general tick body does (SIM_SPEC.md §4), and nothing else: a cluster about to run any other
// event (an election, a log entry, a halt, a message it cannot hold) is stopped ("bailed") before
// that tick with its state written back, and the same workgroup then runs it from that tick to
// the launch's end through the general tick body (tick_wave, CATCH form). Results are therefore
// identical to the general kernel's for any state; only the speed depends on how steady the
// clusters are. One dispatch per launch: there is no separate catch-up launch.
//
// Lane per cluster. One lane runs one whole cluster: the leader and its N-1 followers are named
// registers (follower slot j is the j-th non-leader node in id order, so deliveries in sender
// order are slot order), the messages in flight are registers too (a follower holds at most one
// append-entries from the leader; the leader's append-responses all share one arrival and pop in
// sender id order), and no event needs another lane: no shuffles, ballots or LDS inside the tick
// loop. A wave runs 64 clusters; C2's 65,536 clusters are 1,024 waves, one per SIMD.
//
// What a heartbeat round costs is its multiplies: Philox draws (the followers' election timers)
// and the trace hash. A follower's re-armed deadline (t + el_base + draw) is only compared with
// ticks before the next append-entries reaches it, and in steady state (el_base > hb) none is, so
// the draw is deferred: the deadline holds its lower bound t + el_base and a pending bit, and the
// draw is made when a tick at or past that bound is about to be decided, or at write-back — one
// draw per follower per launch instead of one per round, with identical results.
#include <hip/hip_ext.h>

#include "fixed_point_affine.hpp"
#include "tick_wave.hpp"

namespace rs {

constexpr int LANE_WG = 256;                 // four waves, 64 clusters each

// a ? x : y without a select the compiler could fold into an indexed load
__device__ __forceinline__ uint32_t msel(bool a, uint32_t x, uint32_t y) {
  const uint32_t m = 0u - (uint32_t)a;
  return (x & m) | (y & ~m);
}

// The state image. A wave stages its 64 clusters' blocks (the first IMG_SLOTS 16-B chunks of each:
// four 128-B lines at N >= 4) in LDS: loads and stores then move whole lines, eight lines per wave
// instruction, where a lane reading its own cluster's block straight into registers touches 64
// lines per instruction (one per lane, the texture path's rate) -- the load phase's cost.
// Three parts: line 0 of every cluster, line 1 of every cluster (loaded only when some cluster of
// the wave has no strong certificate, device.hpp), then lines 2-3 (only when some cluster has no
// certificate at all). The LDS-DMA loads (global_load_lds: lane-linear destination, 1 KiB per wave
// instruction) take the swizzles on their source addresses.
// Lines 0 and 1: chunk i of line ln of the wave's cluster l sits in slot (i & 7) ^ img_sw(l) of
// l's 128-B row of that line's 8-KiB part, so one DMA instruction fills eight clusters' rows. A
// lane reading chunk i of its own cluster meets no bank conflict (the 16 lanes of a ds_read_b128
// group have distinct l & 15: the row's half of the 256 B of banks is l & 1, and (l & 1,
// img_sw(l)) is distinct for distinct l & 15), nor does it writing the chunk back (ds_write_b128:
// eight consecutive lanes over 128 B of banks, img_sw distinct), nor do the line stores' reads.
// Lines 2-3: chunk i sits in slot (i & 15) ^ (l & 15) of l's 256-B row.
constexpr int IMG_SLOTS = 32;                               // chunks per cluster, all parts
constexpr uint32_t IMG_LINE = 64 * 8 * 16;                  // 8 KiB: 64 clusters x 8 chunks
constexpr uint32_t IMG_HALF = 2 * IMG_LINE;                 // 16 KiB: lines 0-1, or lines 2-3
constexpr uint32_t IMG_WAVE = 2 * IMG_HALF;                 // 32 KiB per wave
__device__ __forceinline__ uint32_t img_sw(uint32_t l) { return (l ^ (l >> 3)) & 7u; }
__device__ __forceinline__ uint32_t img_off(uint32_t l, uint32_t i) {
  return i < 16 ? (i >> 3) * IMG_LINE + l * 128u + 16u * ((i & 7u) ^ img_sw(l))
                : IMG_HALF + l * 256u + 16u * ((i & 15u) ^ (l & 15u));
}
template <typename T>
__device__ __forceinline__ T* lds_at(char* img, uint32_t off) {
  return reinterpret_cast<T*>(img + off);
}

// Dynamic LDS of a steady workgroup: the four waves' state images. A wave that bailed clusters
// runs them through the general tick body with its own image as that body's LDS block (the image
// is dead once the write-back has read it): the waves of a workgroup never wait for each other.
template <int N>
constexpr size_t steady_lds_bytes() {
  static_assert(block_lds_bytes<N, false>() <= IMG_WAVE, "the catch-up block fits a wave's image");
  return 4 * (size_t)IMG_WAVE;
}

// M2^n and 1 + M2 + ... + M2^(n-1) mod 2^64 (the trace hash's multiplier per event, device.hpp)
template <int n>
__host__ __device__ constexpr uint64_t trace_pow() {
  uint64_t x = 1;
  for (int i = 0; i < n; ++i) x *= TRACE_M2;
  return x;
}
template <int n>
__host__ __device__ constexpr uint64_t trace_geo() {
  uint64_t s = 0, x = 1;
  for (int i = 0; i < n; ++i) {
    s += x;
    x *= TRACE_M2;
  }
  return s;
}

// fixed_point_affine.hpp restates the hash's constants without this project's headers
static_assert(fpa::M == TRACE_M && fpa::M2 == TRACE_M2 && fpa::ROLE_LEADER == RAFT_LEADER &&
                  fpa::ROLE_FOLLWER == RAFT_FOLLWER &&
                  fpa::EV_APPEND_ENTRIES == RAFT_MSG_APPEND_ENTRIES &&
                  fpa::EV_APPEND_RESPONSE == RAFT_MSG_APPEND_RESPONSE,
              "the affine step's hash is the trace hash");

// The affine maps (fixed_point_affine.hpp) of the two counts of whole rounds a launch holds for a
// cluster on the schedule: its first heartbeat th of the launch is in [t0, t0 + P), so it runs
// K1 = K(th = t0) whole rounds or one fewer. A wave builds both on the scalar unit while its
// line-0 load is in flight and keeps them in LDS (scalar registers are what the kernel lacks, and
// 36 vector registers held from the kernel's top to the rounds cost the small-N kernels a wave of
// occupancy); a lane reads the set of its own K, five 16-B reads.
struct alignas(16) SetWords {                         // fpa::Set's maps, K rounds; K1 beside them
  uint64_t la, lx, ly, lz, fa, fx, fy, fz;
  uint32_t ls, fs, K, K1;
  __device__ __forceinline__ fpa::Half lead() const { return fpa::Half{la, lx, ly, lz, ls}; }
  __device__ __forceinline__ fpa::Half fol() const { return fpa::Half{fa, fx, fy, fz, fs}; }
};
struct BandSets {
  SetWords k[2];                                      // k[1] is K1 rounds, k[0] is K1 - 1
};
__device__ __forceinline__ uint32_t vreg(uint32_t s) {   // a uniform value, from the scalar unit
  uint32_t v;
  asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(s));
  return v;
}
__device__ __forceinline__ uint64_t vreg(uint64_t s) {
  return (uint64_t)vreg((uint32_t)(s >> 32)) << 32 | vreg((uint32_t)s);
}
__device__ __forceinline__ SetWords vreg(const fpa::Set& c, uint32_t K1) {
  return SetWords{vreg(c.lead.a), vreg(c.lead.x), vreg(c.lead.y), vreg(c.lead.z),
                  vreg(c.fol.a),  vreg(c.fol.x),  vreg(c.fol.y),  vreg(c.fol.z),
                  vreg(c.lead.s), vreg(c.fol.s),  vreg(c.K),      vreg(K1)};
}
// Lane I of `park` takes the wave-uniform v: v_writelane, kept in program order with the other asm
// statements (the loads' issue before it, their wait behind it).
template <int I>
__device__ __forceinline__ void park_lane(uint32_t& park, uint32_t v) {
  asm volatile("v_writelane_b32 %0, %1, %2"
               : "+v"(park)
               : "s"(__builtin_amdgcn_readfirstlane(v)), "n"(I));
}
// The sets of a launch of nt ticks into *out. Uniform arguments: scalar code, moved to vector
// registers (the stores' data) by instructions the compiler keeps in program order.
// Returns the launch's band (K1, rho, K1 * P), from the same division.
template <int F>
__device__ __forceinline__ fpa::Band band_sets(uint32_t nt, uint32_t d, uint32_t hb, BandSets* out) {
  const fpa::Band b = fpa::band(F, d, hb, nt);
  const uint32_t K1 = b.K1;
  const fpa::Set lo = fpa::build<F>(d, hb, K1 ? K1 - 1 : 0), hi = fpa::step<F>(lo, d, hb);
  out->k[0] = vreg(lo, K1);
  out->k[1] = vreg(hi, K1);
  return b;
}

// A cluster at its fixed point, lane-resident: every follower took the leader's append-entries
// (flags, votes, term and commit are what another one sets again), every response succeeded (next /
// match / keys as another one sets them), the log is empty (a heartbeat ships nothing). With the
// followers' re-armed timers (>= t_ae + el_base) unable to fire before the next round's
// append-entries (el_base >= the round period P = 2d + F - 1 + hb) and the leader's responses all
// before its next heartbeat (hb >= 2d + F), every round is the last one shifted by P: only the
// ticks in the trace hashes change. Follower slot j is node j (j < L) or j + 1 (j >= L).
template <int N>
struct FixedPoint {
  static constexpr int F = N - 1;
  static constexpr bool IN_BAND = false;             // rounds(): any K
  uint32_t L, Lid, Lterm, Lcommit;
  uint64_t Ltr, ftr[F];
  uint32_t Ldl, fdl[F], fpend;                       // fpend: followers whose draw is owed
  uint32_t qmask, qA[F], qT[F], qa[F], qb[F];        // append-entries in flight, per follower
  uint32_t rmask, resA, rT[F], rA[F], rB[F], rH[F];  // responses queued at the leader
  uint32_t nhb, nae, nar;

  __device__ __forceinline__ uint32_t fk(int j) const { return (uint32_t)j + ((uint32_t)j >= L ? 1u : 0u); }

  // The append-entries of the round with heartbeat th reach every follower at ta = th + d.
  __device__ __forceinline__ void append_entries(uint32_t ta, uint32_t d, uint32_t el_base) {
#pragma unroll
    for (int j = 0; j < F; ++j) {
      ftr[j] = trace_event(ftr[j], ta, RAFT_MSG_APPEND_ENTRIES, Lid, Lterm, RAFT_FOLLWER, Lterm, 0);
      fdl[j] = ta + el_base;                          // + the owed draw
      rT[j] = Lterm; rA[j] = Lcommit; rB[j] = 0; rH[j] = 1;
      qA[j] = INF;
    }
    fpend = (1u << F) - 1;
    qmask = 0;
    rmask = (1u << F) - 1;
    resA = ta + d;
    nae += F;
  }
  // The responses of the round with heartbeat th still queued, one per tick in slot order, up to
  // tend - 1.
  __device__ __forceinline__ void responses(uint32_t th, uint32_t tend, uint32_t d, uint32_t hb) {
#pragma unroll
    for (int j = 0; j < F; ++j) {
      const uint32_t tau = th + 2 * d + j;
      if (((rmask >> j) & 1) && tau < tend) {
        Ltr = trace_event(Ltr, tau, RAFT_MSG_APPEND_RESPONSE, fk(j) + 1, Lterm, RAFT_LEADER,
                          Lterm, 0);
        rmask &= ~(1u << j);
        Ldl = tau + hb;
        ++nar;
      }
    }
    if (!rmask) resA = INF;
  }
  // what rounds() and run_launch() (below) ask of a lane state
  __device__ __forceinline__ uint32_t term() const { return Lterm; }
  __device__ __forceinline__ uint32_t sid(int j) const { return fk(j) + 1; }   // slot j's id
  __device__ __forceinline__ void followers(uint64_t a, uint64_t add) {
#pragma unroll
    for (int j = 0; j < F; ++j) ftr[j] = ftr[j] * a + add;
  }
  __device__ __forceinline__ void rearmed(uint32_t v) {   // by an append-entries; the draw owed
#pragma unroll
    for (int j = 0; j < F; ++j) fdl[j] = v;
    fpend = (1u << F) - 1;
  }
  __device__ __forceinline__ void heartbeat(uint32_t ta) {   // its append-entries, arriving at ta
#pragma unroll
    for (int j = 0; j < F; ++j) {
      qA[j] = ta; qT[j] = Lterm; qa[j] = Lcommit; qb[j] = 0;
    }
    qmask = (1u << F) - 1;
  }
  __device__ __forceinline__ bool queued() const { return rmask != 0; }   // responses still queued

  // Write-back. Node k is the leader (k == L) or follower slot k - 1 (k > L) / k (k < L): x of that
  // slot, both candidates at static indices.
  __device__ __forceinline__ int slot(int k) const {
    return (uint32_t)k > L ? (k > 0 ? k - 1 : 0) : (k < F ? k : F - 1);
  }
  __device__ __forceinline__ uint32_t at_node(const uint32_t (&x)[F], int k) const {
    return msel((uint32_t)k > L, x[k > 0 ? k - 1 : 0], x[k < F ? k : F - 1]);
  }
  // node k's words of fields DEADLINE .. RES_TAIL into v[field][k]
  template <int NV>
  __device__ __forceinline__ void node_words(int k, uint32_t (&v)[NV][N]) const {
    const bool isL = (uint32_t)k == L;
    const int jl = k > 0 ? k - 1 : 0, jh = k < F ? k : F - 1;
    const bool lo = (uint32_t)k > L;
    const uint32_t fq = (qmask >> slot(k)) & 1, fqa = at_node(qA, k);
    const uint64_t trf = (uint64_t)msel(lo, (uint32_t)(ftr[jl] >> 32), (uint32_t)(ftr[jh] >> 32)) << 32 |
                         msel(lo, (uint32_t)ftr[jl], (uint32_t)ftr[jh]);
    const uint64_t tr = isL ? Ltr : trf;
    v[HF_DEADLINE][k] = isL ? Ldl : at_node(fdl, k);
    v[HF_TRACE_LO][k] = (uint32_t)tr;
    v[HF_TRACE_HI][k] = (uint32_t)(tr >> 32);
    v[HF_QMETA][k] = isL ? pack_qmeta(0, 0, 0, __popc(rmask)) : pack_qmeta(0, fq, 0, 0);
    v[HF_REQ_ARR][k] = isL ? INF : (fq ? fqa : INF);
    v[HF_RES_ARR][k] = isL ? resA : INF;
    v[HF_REQ_TAIL][k] = isL ? 0u : (fq ? fqa : 0u);
    v[HF_RES_TAIL][k] = isL ? (rmask ? resA : 0u) : 0u;
  }
  // The messages in flight at the launch's end back to cluster c's rings, heads at slot 0 (rare).
  // Every lane of the wave calls it; on: the lane's cluster is written back.
  __device__ __forceinline__ void to_rings(const DevSim& S, uint32_t c, bool on) const {
    if (!__builtin_amdgcn_ballot_w64(on && (qmask || rmask))) return;   // wave-uniform
#pragma unroll
    for (int j = 0; j < F; ++j) {
      if (on && ((qmask >> j) & 1)) {
        uint4* dp = reinterpret_cast<uint4*>(qslots(S, c * N + fk(j), 0));
        dp[0] = make_uint4(qA[j], RAFT_MSG_APPEND_ENTRIES | Lid << 3, qT[j], qa[j]);
        dp[1] = make_uint4(qb[j], 0, 0, 0);
      }
    }
    uint4* rp = reinterpret_cast<uint4*>(qslots(S, c * N + L, 1));
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < F; ++j) {
      if (on && ((rmask >> j) & 1)) {
        uint4* dp = rp + 2 * n;
        dp[0] = make_uint4(resA, RAFT_MSG_APPEND_RESPONSE | sid(j) << 3 | rH[j] << 7, rT[j], rA[j]);
        dp[1] = make_uint4(rB[j], 0, 0, 0);
        ++n;
      }
    }
  }
};

// A cluster under a strong certificate (device.hpp), lane-resident in node order: the line-0 body's
// state. On the fixed point's schedule what FixedPoint keeps per follower slot is one value for all
// followers -- they take the same append-entries at the same tick with the same term, so they share
// its arrival, the deadline it re-arms, their QMETA and tails -- and the responses queued at the
// leader are the last rc slots in slot order, all of the leader's term, successful, with one
// arrival. Only the trace hashes differ, and a hash needs no slot: every hash takes the followers'
// step (one addend for all), slot L's is dead and the leader's own (Ltr) replaces it at write-back.
// Events, ticks and hash terms are FixedPoint's.
template <int N>
struct NodeOrder {
  static constexpr int F = N - 1;
  static constexpr bool IN_BAND = true;              // rounds(): th is in [t0, t0 + P), tested
  uint32_t L, T;                                     // the leader's index; every node's term
  uint64_t tr[N], Ltr;                               // hashes by node (tr[L] dead); the leader's
  uint32_t Ldl;
  bool qin, took;                                    // append-entries in flight; one taken here
  uint32_t qA, fdl;                                  // their arrival; the deadline the taken one set
  uint32_t rc, resA;                                 // responses queued (slots F - rc ..), arrival
  uint32_t nhb, nae, nar;

  __device__ __forceinline__ uint32_t sid(int j) const {   // the id of follower slot j
    return (uint32_t)j + 1 + ((uint32_t)j >= L ? 1u : 0u);
  }
  __device__ __forceinline__ void followers(uint64_t a, uint64_t add) {
#pragma unroll
    for (int k = 0; k < N; ++k) tr[k] = tr[k] * a + add;
  }
  __device__ __forceinline__ void append_entries(uint32_t ta, uint32_t d, uint32_t el_base) {
    followers(TRACE_M2, trace_term(ta, RAFT_MSG_APPEND_ENTRIES, L + 1, T, RAFT_FOLLWER, T, 0));
    took = true;
    fdl = ta + el_base;                               // + the owed draw
    qin = false;
    rc = F;
    resA = ta + d;
    nae += F;
  }
  __device__ __forceinline__ void responses(uint32_t th, uint32_t tend, uint32_t d, uint32_t hb) {
#pragma unroll
    for (int j = 0; j < F; ++j) {
      const uint32_t tau = th + 2 * d + j;
      if ((uint32_t)j + rc >= (uint32_t)F && tau < tend) {   // slot j is queued
        Ltr = trace_event(Ltr, tau, RAFT_MSG_APPEND_RESPONSE, sid(j), T, RAFT_LEADER, T, 0);
        --rc;
        Ldl = tau + hb;
        ++nar;
      }
    }
    if (!rc) resA = INF;
  }
  __device__ __forceinline__ uint32_t term() const { return T; }
  __device__ __forceinline__ void rearmed(uint32_t v) { took = true; fdl = v; }
  __device__ __forceinline__ void heartbeat(uint32_t ta) { qin = true; qA = ta; }
  __device__ __forceinline__ bool queued() const { return rc != 0; }
};

// From the fixed point with the next heartbeat at th, every round to the launch's end: the rounds
// that end before it as trace hashes alone, then the one it cuts (heartbeat, append-entries and
// responses up to tend - 1; what is left stays queued as the general body leaves it). Every next
// event of the cluster is then at or after tend. St: FixedPoint or NodeOrder.
//
// The K whole rounds are one affine step of each hash (fixed_point_affine.hpp) when K is one of
// the two counts the wave's sets hold, as it is for every cluster on the schedule; when some lane
// here has another K (set_tick moved the clock, an election ended mid-launch, ...) all of them
// take the loop over rounds instead.
//
// The band form (St::IN_BAND: the line-0 body, whose decision tested th - t0 < P): K is K1 or
// K1 - 1 by one comparison against the launch's band (fixed_point_affine.hpp, Band), the set is
// picked by it, and the set of no round is the identity, so the step is taken by every lane: no
// division, no read of K1, no ballot and no loop.
struct LaunchBand {
  uint32_t t0;
  fpa::Band b;
};
template <typename St>
__device__ __forceinline__ void rounds(St& s, uint32_t th, uint32_t tend, uint32_t d, uint32_t hb,
                                       uint32_t el_base, const BandSets& bs, const LaunchBand& lb) {
  constexpr int F = St::F;
  const uint32_t P = 2 * d + F - 1 + hb, last = 2 * d + F - 1, T = s.term();
  uint32_t K, tk;
  if constexpr (St::IN_BAND) {
    const uint32_t delta = th - lb.t0;
    K = fpa::band_rounds(lb.b, delta);
    tk = th + fpa::band_ticks(lb.b, P, delta);
    // k[1] holds K1 rounds and k[0] K1 - 1; at K1 = 0 both K's set is k[0], the identity
    const SetWords sw = bs.k[(delta <= lb.b.rho) & (lb.b.K1 != 0)];
    const fpa::Half cl = sw.lead(), cf = sw.fol();
    s.Ltr = fpa::apply_leader<F>(cl, s.Ltr, th, T, s.L);
    s.followers(cf.a, fpa::follower_addend<F>(cf, th, T, s.L));
    if (K) {
      s.rearmed(tk - P + d + el_base);
      s.Ldl = tk;
      s.nhb += K;
      s.nae += F * K;
      s.nar += F * K;
    }
  } else {
    K = tend > th + last ? (tend - th - last - 1) / P + 1 : 0;
    tk = th + K * P;
  }
  if (!St::IN_BAND && K) {
    const uint32_t K1 = bs.k[0].K1;
    const bool top = K == K1;
    if (!__builtin_amdgcn_ballot_w64(!top && K + 1 != K1)) {   // uniform over the lanes here
      const SetWords sw = bs.k[top];                            // the lane's own set (K rounds)
      const fpa::Half cl = sw.lead(), cf = sw.fol();
      s.Ltr = fpa::apply_leader<F>(cl, s.Ltr, th, T, s.L);
      s.followers(cf.a, fpa::follower_addend<F>(cf, th, T, s.L));
    } else {
      // The trace hash is polynomial (device.hpp): a round's F + 1 leader events take the
      // leader's hash h to h * M2^(F+1) + a, with a the Horner sum of the events' terms, and a
      // round P ticks later adds P * M * (1 + M2 + ... + M2^F) to a; a follower's one event per
      // round takes h to h * M2 + c, and c grows by P * M. One multiply-add per hash per round.
      uint64_t a = trace_term(th, 7, 0, 0, RAFT_LEADER, T, 0);
#pragma unroll
      for (int j = 0; j < F; ++j)
        a = a * TRACE_M2 + trace_term(th + 2 * d + j, RAFT_MSG_APPEND_RESPONSE, s.sid(j), T,
                                      RAFT_LEADER, T, 0);
      const uint64_t da = (uint64_t)P * (TRACE_M * trace_geo<F + 1>());
      const uint64_t df = (uint64_t)P * TRACE_M;
      uint64_t cf = trace_term(th + d, RAFT_MSG_APPEND_ENTRIES, s.L + 1, T, RAFT_FOLLWER, T, 0);
      for (uint32_t r = 0; r < K; ++r) {
        s.Ltr = s.Ltr * trace_pow<F + 1>() + a;
        a += da;
        s.followers(TRACE_M2, cf);
        cf += df;
      }
    }
    s.rearmed(tk - P + d + el_base);              // by the last whole round's append-entries
    s.Ldl = tk;                                   // = the last response + hb
    s.nhb += K;
    s.nae += F * K;
    s.nar += F * K;
  }
  if (__builtin_expect(tk < tend, 0)) {           // the round the launch's end cuts (rare)
    s.Ltr = trace_event(s.Ltr, tk, 7, 0, 0, RAFT_LEADER, T, 0);
    ++s.nhb;
    s.Ldl = tk + hb;
    s.heartbeat(tk + d);
    if (tk + d < tend) {                          // the append-entries, then responses in time
      s.append_entries(tk + d, d, el_base);
      s.responses(tk, tend, d, hb);
    }
  }
}

// A launch from t0 for a cluster on the fixed point's schedule: the round in progress at t0 (mid:
// 0 none, 1 its append-entries in flight, 2 its responses as the last launch's end cut them; its
// heartbeat was at th0) to its end or the launch's, then the rounds from the next heartbeat.
template <typename St>
__device__ __forceinline__ void run_launch(St& s, uint32_t mid, uint32_t th0, uint32_t tend,
                                           uint32_t d, uint32_t hb, uint32_t el_base, uint32_t P,
                                           const BandSets& bs, const LaunchBand& lb) {
  bool whole = true;                              // the round in progress finished in this launch
  // (Rare, and tested once for the lanes here: a wave none of whose clusters is in a round at t0
  // branches once, to no block of this, and the common stream falls through.)
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(mid != 0) != 0, 0)) {
    if (mid == 1) {
      if (th0 + d < tend) s.append_entries(th0 + d, d, el_base);
      else whole = false;
    }
    if (mid && whole) {
      s.responses(th0, tend, d, hb);
      whole = !s.queued();
    }
  }
  if (__builtin_expect(whole, 1)) rounds(s, mid ? th0 + P : th0, tend, d, hb, el_base, bs, lb);
}

// Which round of the period-P schedule is in progress at t0, from the leader's deadline Ldl and
// the messages in flight: the followers' request (req: present, arriving at reqA) or the nres
// responses queued at the leader (arriving at resA). on: the cluster is on the schedule -- no
// round (the next heartbeat at Ldl >= t0), append-entries not yet due, or responses exactly as the
// last launch's end cut them; th0 is the round's heartbeat (mid = 0: the next one), nxt the
// followers' next append-entries (or the launch's end): no follower's timer may fire before it.
struct Schedule {
  uint32_t mid, th0, nxt;
  bool on;
};
template <int F>
__device__ __forceinline__ Schedule schedule(uint32_t t0, uint32_t tend, uint32_t d, uint32_t hb,
                                             uint32_t P, uint32_t Ldl, bool req, uint32_t reqA,
                                             uint32_t nres, uint32_t resA) {
  Schedule s{0, Ldl, 0, true};
  if (req) {                                      // the append-entries in flight
    s.mid = 1;
    s.th0 = reqA - d;
    s.on = reqA >= t0 && reqA >= d && Ldl == s.th0 + hb;
  } else if (nres) {                              // the responses the last launch's end cut
    s.mid = 2;
    s.th0 = resA - 2 * d;
    // the leader's deadline is the round's heartbeat + hb until it takes a response, then that
    // response's tick (th + 2d + j0 - 1 for the j0-th) + hb
    const uint32_t j0 = (uint32_t)F - nres;       // responses already taken
    const int64_t cut = (int64_t)t0 - ((int64_t)s.th0 + 2 * d);   // what the last launch's end cut
    s.on = resA >= 2 * d && (int64_t)j0 == (cut < 0 ? 0 : cut > F ? (int64_t)F : cut) &&
           Ldl == (j0 ? s.th0 + 2 * d + j0 - 1 : s.th0) + hb;
  } else {
    s.on = Ldl >= t0;
  }
  s.nxt = min((s.mid == 2 ? s.th0 + P : s.th0) + d, tend);
  return s;
}

// The tail every path of the kernel ends with, one copy of each piece: the line-0 wave runs them
// where its body ends and returns, the other paths where they join.
//
// Dirty lines back to memory whole (dl: bit ln set in the lanes whose cluster's line ln changed,
// ln < LINES): a wave instruction writes eight clusters' line (8 lanes x 16 B each), read from the
// image (line ln of cluster cc is its chunks 8 ln .. 8 ln + 7): the eight reads of a line first,
// then the stores. The stores write through to memory (sc1: the lines leave the XCD's L2 as the
// waves end, not at the launch's end; the next launch reads them from the Infinity Cache either
// way). They are not in the compiler's wait counts: the catch-up waits for them itself.
template <int N, int LINES>
__device__ __forceinline__ void store_lines(const DevSim& S, char* img, uint32_t cbase,
                                            uint32_t lane, uint32_t dl) {
  constexpr uint32_t HB = hot_block_words(N);
  // The lane's address terms are computed here, at each call: the lane id passes through an empty
  // statement. Shared between the two calls they are computed at the kernel's top and stay live
  // across every other path, which cost the N = 2 and N = 3 kernels a wave of occupancy each.
  asm volatile("" : "+v"(lane));
  uint32_t* const wbase = S.hot + (size_t)cbase * HB;      // the wave's first block
  const uint32_t sub = lane >> 3, q8 = lane & 7;
#pragma unroll
  for (int ln = 0; ln < LINES; ++ln) {
    const uint64_t bal = __builtin_amdgcn_ballot_w64((dl >> ln) & 1);
    if (!bal) continue;                                  // wave-uniform
    uint4 xs[8];
#pragma unroll
    for (int gq = 0; gq < 8; ++gq)
      xs[gq] = *lds_at<const uint4>(img, img_off(8 * gq + sub, 8 * ln + q8));
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    if (__builtin_expect(bal == ~0ull, 1)) {
      // every cluster of a full wave (the headline's every wave): eight stores with no
      // predicate, a lane's address in the first group of eight blocks once and one 64-bit add
      // per further group. (Addresses stay in vector registers: a store in an asm statement
      // that took its base from scalar registers would stand outside the compiler's hazard
      // checks, and a scalar register a vector instruction wrote needs five wait states
      // before a memory instruction reads it.)
      uint32_t* const dst0 = wbase + sub * HB + 4 * (8 * ln + q8);
#pragma unroll
      for (int gq = 0; gq < 8; ++gq) {
        const v4u xv = {xs[gq].x, xs[gq].y, xs[gq].z, xs[gq].w};
        uint32_t* const dst = dst0 + (size_t)(8 * gq) * HB;
        asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst), "v"(xv) : "memory");
      }
      continue;
    }
#pragma unroll
    for (int gq = 0; gq < 8; ++gq) {
      const uint32_t cc = 8 * gq + sub;
      if ((bal >> cc) & 1) {
        const v4u xv = {xs[gq].x, xs[gq].y, xs[gq].z, xs[gq].w};
        uint32_t* const dst = wbase + cc * HB + 4 * (8 * ln + q8);
        asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst), "v"(xv) : "memory");
      }
    }
  }
}

// wave wid's copy of the counter block
__device__ __forceinline__ unsigned long long* wave_counters(const DevSim& S, uint32_t wid) {
  return S.ctr + (size_t)(wid % CTR_COPIES) * CTR_STRIDE;
}
// Counters: heartbeats, append-entries, append-responses; every message is delivered. One
// wave-wide sum each, added by five lanes to the wave's copy of the counter block.
template <int N>
__device__ __forceinline__ void add_counters(const DevSim& S, uint32_t lane, uint32_t wid,
                                             uint32_t nhb, uint32_t nae, uint32_t nar) {
  const uint32_t h = wave_sum(nhb), a = wave_sum(nae), r = wave_sum(nar);
  // lane 0 .. 4: heartbeats, append-entries, append-responses, sent, delivered. The index is
  // a nibble of a constant and the value a chain of selects: one branch, around the atomic.
  constexpr uint32_t IDX = RAFT_CTR_EV_HEARTBEAT | RAFT_CTR_EV_AE << 4 | RAFT_CTR_EV_AR << 8 |
                           RAFT_CTR_SENT << 12 | RAFT_CTR_DELIVERED << 16;
  static_assert(RAFT_CTR_DELIVERED < 16, "a nibble per index");
  const uint32_t msgs = (uint32_t)(N - 1) * h + a;
  const uint32_t idx = (IDX >> (4 * (lane & 7))) & 15u;
  const uint32_t v = msel(lane == 0, h, msel(lane == 1, a, msel(lane == 2, r, msgs)));
  if (lane < 5 && v) atomicAdd(&wave_counters(S, wid)[idx], (unsigned long long)v);
}


template <int N>
__global__ void __launch_bounds__(LANE_WG) steady_lane_kernel(DevSim S, uint32_t t0, uint32_t nt) {
  static_assert(N >= 2 && N <= 5, "follower masks and the response queue fit four followers");
  constexpr int F = N - 1;
  constexpr uint32_t HB = hot_block_words(N);
  // the words read: the cluster's (checker hwm) and every node field up to the leader-state rows
  // (device.hpp: words 0-122 at N = 5, four lines) -- the leader's rows are picked from them once
  // its id is known, with no second round trip. The image holds whole lines of the block.
  constexpr int NWORDS = (int)(HOT_CW + hf_abase(N) * N);
  constexpr int NW4 = (NWORDS + 3) / 4;
  constexpr int IMGC = (int)(HB / 4) < IMG_SLOTS ? (int)(HB / 4) : IMG_SLOTS;   // chunks staged
  static_assert(NW4 <= IMGC && IMGC % 8 == 0, "the image holds the words read, in whole lines");
  __shared__ uint32_t bl_c[LANE_WG], bl_t[LANE_WG];   // per wave: bailed cluster, tick it stopped before
  __shared__ BandSets bs_keep[LANE_WG / 64];          // per wave: the launch's affine sets
  extern __shared__ __attribute__((aligned(16))) uint32_t dsm[];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t cbase = blockIdx.x * LANE_WG + wave * 64;      // the wave's clusters, in id order
  const uint32_t c0 = cbase + lane < S.C ? cbase + lane : INF;
  const bool active = c0 != INF;
  const uint32_t c = active ? c0 : 0u;
  const uint32_t g = S.goff + c;
  char* const img = reinterpret_cast<char*>(dsm) + wave * IMG_WAVE;
  uint32_t* const blc = bl_c + wave * 64;
  uint32_t* const blt = bl_t + wave * 64;
  uint32_t nbw = 0;                                   // clusters this wave bailed (uniform)
  // a compaction point: every lane of the wave active
  auto record_bail = [&](bool b, uint32_t tick) {
    const uint64_t m = __builtin_amdgcn_ballot_w64(b);
    if (b) {
      const uint32_t i = nbw + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      blc[i] = c;
      blt[i] = tick;
    }
    nbw += (uint32_t)__popcll(m);
  };
#ifdef RS_WAVELOG   // diagnostic build: per-wave timeline (scripts/lane_timeline.py)
  const uint64_t wl_start = wall_clock64();
  uint32_t wl_trips = 0, wl_first = 0, wl_ph[6] = {0, 0, 0, 0, 0, 0};
  uint64_t wl_loop = 0, wl_ts = 0;
#define RS_LPH(i)                                         \
  do {                                                    \
    const uint64_t now_ = __builtin_amdgcn_s_memtime();   \
    wl_ph[i] += (uint32_t)(now_ - wl_ts);                 \
    wl_ts = now_;                                         \
  } while (0)
#else
#define RS_LPH(i) do {} while (0)
#endif

  // ------------------------------------------- load: the wave's blocks into its image (LDS-DMA)
  // line ln (0 or 1): wave instruction j takes clusters 8j .. 8j + 7, 8 slots each
  auto load_wait = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the wave's own LDS-DMA writes landed
  };
  auto load_line = [&](int ln, bool wait) {
    const uint32_t p = lane & 7;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t cc = 8 * j + (lane >> 3);
      const uint32_t i = 8 * ln + (p ^ img_sw(cc));
      const uint32_t cg = min(cbase + cc, S.C - 1);  // past the shard's end: any block, unused
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)(S.hot + (size_t)cg * HB + 4 * i),
          (__attribute__((address_space(3))) void*)(img + ln * IMG_LINE + j * 1024), 16, 0, 0);
    }
    if (wait) load_wait();
  };
  // lines 2-3: wave instruction j takes clusters 4j .. 4j + 3, 16 slots each
  auto load_half1 = [&]() {
    const uint32_t p = lane & 15;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t cc = 4 * j + (lane >> 4);
      const uint32_t i = 16 + (p ^ (cc & 15u));
      const uint32_t cg = min(cbase + cc, S.C - 1);
      if (i < (uint32_t)IMGC)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(S.hot + (size_t)cg * HB + 4 * i),
            (__attribute__((address_space(3))) void*)(img + IMG_HALF + j * 1024), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  static_assert(IMGC >= 16, "lines 0 and 1 are whole in every block");
  uint32_t w[NW4 * 4];          // (the words past line 0 are set where a wave leaves the line-0 body)
  auto read_chunks = [&](int lo, int hi) {              // chunks [lo, hi) of the image into w[]
#pragma unroll
    for (int i = lo; i < hi; ++i) {
      const uint4 x = *lds_at<const uint4>(img, img_off(lane, i));
      w[4 * i] = x.x; w[4 * i + 1] = x.y; w[4 * i + 2] = x.z; w[4 * i + 3] = x.w;
    }
  };
  // field f of node k; of the leader L; of follower slot j (node j below L, j + 1 from L on)
  auto word = [&](int f, int k) { return w[HOT_CW + f * N + k]; };
  auto lword = [&](int f, uint32_t L) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) v |= word(f, k) & (0u - (uint32_t)(L == (uint32_t)k));
    return v;
  };
  auto fword = [&](int f, int j, uint32_t L) {
    return msel((uint32_t)j >= L, word(f, j + 1), word(f, j));
  };
  // the fields every path writes, DEADLINE .. RES_TAIL of every node, are whole chunks
  static_assert(HF_RES_TAIL + 1 == HF_FLAGS && (HOT_CW + HF_FLAGS * N) % 4 == 0 && HOT_CW % 4 == 0,
                "the fields written: DEADLINE .. RES_TAIL, whole chunks");
  constexpr int CH_END = (int)(HOT_CW + HF_FLAGS * N) / 4;
  // The arguments the affine sets are built from, fetched with the ones the loads' addresses wait
  // for: one scalar round trip at the kernel's top, not a second one between the loads' issue and
  // the build (measured: DESIGN.md, "The line-0 body in node order").
  asm volatile("" ::"s"(nt), "s"(t0), "s"(S.dmin), "s"(S.hb), "s"(S.el_base));
  load_line(0, false);
  // The previous steady launch's bail count (complete: that launch has ended) to the host, which
  // picks the next launches' path from it (speed only); that word is this launch's successor's
  // (host memory is written only when there is something to report: the host zeroes its copy
  // when it acts on it, and a store there holds the launch's end for a bus round trip). Read
  // behind the line-0 loads, in their shadow: nothing here needs it before the kernel ends.
  const bool reporter = blockIdx.x == 0 && threadIdx.x == 0;
  uint32_t prev_bails = 0;
  if (reporter) prev_bails = *S.nbail_zero;
  // The launch's affine sets, while the load is in flight: nt passes through an empty statement
  // after the load's instructions, so nothing of the build is scheduled before them, and the
  // sets' moves out of the scalar registers (band_sets) stand before the wait.
  uint32_t nt_s = nt;
  asm volatile("" : "+s"(nt_s));
  const BandSets& bs = bs_keep[wave];
  // The launch's band (K1, rho, K1 * P: scalar values of the same build) waits for the rounds in
  // three lanes of one vector register, written here in the load's shadow and read back on the
  // scalar unit behind the wait (v_writelane / v_readlane, as the compiler's own scalar spills):
  // no LDS round trip, no scalar register held across the decision.
  uint32_t park = 0;
  {
    const fpa::Band b = band_sets<F>(nt_s, S.dmin, S.hb, &bs_keep[wave]);
    park_lane<0>(park, b.K1);
    park_lane<1>(park, b.rho);
    park_lane<2>(park, b.K1P);
  }
  load_wait();
  asm volatile("" : "+v"(park));               // (no read of it moves above the wait)
  auto parked_band = [&]() {
    return fpa::Band{(uint32_t)__builtin_amdgcn_readlane(park, 0),
                     (uint32_t)__builtin_amdgcn_readlane(park, 1),
                     (uint32_t)__builtin_amdgcn_readlane(park, 2)};
  };
  if (__builtin_expect(reporter && prev_bails, 0)) {
    if (S.bail_report) *S.bail_report = prev_bails;
    *S.nbail_zero = 0;
  }
  static_assert(NW4 >= 8, "line 0 is read whole");
  read_chunks(0, 8);
  const uint32_t tend = t0 + nt, d = S.dmin, hb = S.hb, el_base = S.el_base;
  const uint32_t P = 2 * d + F - 1 + hb, allF = (1u << F) - 1;
  uint32_t dl = 0, nhb = 0, nae = 0, nar = 0;  // lines of the block changed; events run
  bool el = false;                             // the cluster's election ran here (general path)
  uint32_t el_to = 0;                          // its timeouts (two candidates: a tie)
#ifdef RS_WAVELOG
  uint64_t wl_x1 = 0, wl_x2 = 0, wl_x3 = 0, wl_lend = 0, wl_sb = 0;
  uint32_t wl_cut = 0;
  asm volatile("" ::"v"(w[CL_CERT]), "v"(w[HOT_CW]));
  wl_loop = wall_clock64();                   // line 0 loaded
  // the wave's record, behind its line stores (wl_sb: stamped before their first image read)
  auto wave_record = [&]() __attribute__((always_inline)) {
    const uint64_t wl_end = wall_clock64();
    const uint32_t wl_events = nhb + nae + nar;
    const uint32_t emax = ~wave_min(~wl_events), emin = wave_min(wl_events);
    if (lane == 0 && S.wavelog) {
      uint32_t hw, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      uint4* rec = reinterpret_cast<uint4*>(S.wavelog + (size_t)(blockIdx.x * 4 + wave) * 32);
      rec[0] = make_uint4((uint32_t)wl_start, (uint32_t)(wl_start >> 32), (uint32_t)wl_end,
                          (uint32_t)(wl_end >> 32));
      rec[1] = make_uint4(wl_trips, hw, xcc, wl_first);
      rec[2] = make_uint4((uint32_t)(wl_loop - wl_start), (uint32_t)(wl_lend - wl_start), emin, emax);
      rec[3] = make_uint4(wl_ph[0], wl_ph[1], wl_ph[2], wl_ph[3]);
      rec[4] = make_uint4(wl_ph[4], 0, 0, (uint32_t)(wl_sb - wl_start));
      rec[5] = make_uint4((uint32_t)(wl_x1 - wl_start), (uint32_t)(wl_x2 - wl_start),
                          (uint32_t)(wl_x3 - wl_start), wl_cut);
    }
  };
  // the wave's end: its stores issued, counted, its catch-up run
  auto wave_done = [&]() __attribute__((always_inline)) {
    if (lane == 0 && S.wavelog) {
      const uint64_t wl_done = wall_clock64();
      uint32_t* rec = S.wavelog + (size_t)(blockIdx.x * 4 + wave) * 32;
      rec[17] = (uint32_t)wl_done;
      rec[18] = (uint32_t)(wl_done >> 32);
    }
  };
#endif

  // ------------------------------------------- the certified path from line 0 alone
  // A wave whose every cluster holds a strong certificate (device.hpp) runs the whole launch from
  // the first line of its blocks: the leader's id and term are in the certificate's chunk, the
  // deadlines, trace hashes and QMETA words are in line 0 (every N), and whatever else the
  // certified path below reads from the later lines (flags, the term, the head arrivals of the
  // messages in flight) is what the certificate says it is. What picks the round in progress at
  // t0 is tested on first-line words: the followers' QMETA (no request, or one each), the leader's
  // (its response count) and the deadlines against t0 (set_tick moves the clock under a
  // certificate). A cluster that fails a test sends its wave to the two-line path below.
  static_assert(HOT_CW + (HF_QMETA + 1) * N <= 32 && HF_DEADLINE < HF_QMETA &&
                    HF_TRACE_LO < HF_QMETA && HF_TRACE_HI < HF_QMETA && CL_CTERM < HOT_CW,
                "every word the line-0 path reads is in line 0; REQ_ARR, RES_ARR, the flags and "
                "the term are derived (device.hpp)");
  // The tests and the state are in node order (NodeOrder): nothing is gathered into follower
  // slots. A follower is "a node that is not L".
  NodeOrder<N> no;
  uint32_t lmid = 0, lth0 = 0;
  const bool cfg_ok = el_base >= P && hb >= 2 * d + F && S.Q >= (uint32_t)F;
  // (The tests are combined with & on values already in registers and the three cases of the
  // round in progress are selects: no branch in the decision.)
  bool strong = active & cfg_ok & ((w[CL_CERT] & 0xFFFF0000u) == CERT_STRONG) &
                ((w[CL_CERT] & 0xFFFFu) < (uint32_t)N);
  {
    const uint32_t L = w[CL_CERT] & 0xFFFFu;
    no.L = L; no.T = w[CL_CTERM];
    no.Ldl = lword(HF_DEADLINE, L);
    no.Ltr = (uint64_t)lword(HF_TRACE_HI, L) << 32 | lword(HF_TRACE_LO, L);
#pragma unroll
    for (int k = 0; k < N; ++k) no.tr[k] = (uint64_t)word(HF_TRACE_HI, k) << 32 | word(HF_TRACE_LO, k);
    no.took = false; no.fdl = 0;
    no.nhb = no.nae = no.nar = 0;
    const uint32_t Lqm = lword(HF_QMETA, L), rsc = qm_res_cnt(Lqm);
    // a certified block's rings have their heads at slot 0: the followers' QMETA words are all
    // "no message" or all "one request", the leader's is its response count
    const uint32_t qm0 = L ? word(HF_QMETA, 0) : word(HF_QMETA, 1);   // the first follower's
    const bool need = qm0 != 0;                     // the append-entries in flight
    const bool cutr = !need & (rsc != 0);           // the responses the last launch's end cut
    const uint32_t one_req = pack_qmeta(0, 1, 0, 0), only_res = pack_qmeta(0, 0, 0, rsc);
    strong = strong & ((qm0 & ~one_req) == 0) & (Lqm == only_res) & (rsc <= (uint32_t)F) &
             !(need & (rsc != 0));
#pragma unroll
    for (int k = 0; k < N; ++k) strong = strong & ((L == (uint32_t)k) | (word(HF_QMETA, k) == qm0));
    // The round's heartbeat lth0 (none in progress: the next one) is `back` ticks before the
    // leader's deadline: hb until it takes a response, then that response's tick
    // (th + 2d + j0 - 1 for the j0-th) + hb.
    const uint32_t j0 = (uint32_t)F - rsc;
    const uint32_t back = msel(need | cutr, hb + msel(cutr & (j0 != 0), 2 * d + j0 - 1, 0u), 0u);
    lmid = msel(need, 1u, msel(cutr, 2u, 0u));
    lth0 = no.Ldl - back;
    const uint32_t ta = lth0 + d, ra = lth0 + 2 * d;
    const int64_t cut = (int64_t)t0 - (int64_t)ra;
    const bool on_need = ta >= t0;
    const bool on_cut = (int64_t)j0 == (cut < 0 ? 0 : cut > F ? (int64_t)F : cut);
    const bool on_none = no.Ldl >= t0;
    strong = strong & (no.Ldl >= back) & (need ? on_need : cutr ? on_cut : on_none);
    no.qin = need;
    no.qA = msel(need, ta, 0u);
    no.rc = msel(cutr, rsc, 0u);
    no.resA = msel(cutr, ra, INF);
    // no follower's timer fires before its next append-entries. (The followers' deadlines as
    // loaded need not be equal: set_tick or an election's exact draw may leave them apart. The
    // body never reads them again: it writes back the common re-armed one, or the words as loaded.)
    const uint32_t nxt = min(msel(cutr, lth0 + P, lth0) + d, tend);   // the next AE (or end)
#pragma unroll
    for (int k = 0; k < N; ++k)
      strong = strong & ((L == (uint32_t)k) | (word(HF_DEADLINE, k) >= nxt));
    // the band: the first heartbeat of the launch's rounds is in [t0, t0 + P) (unsigned: one
    // before t0 fails too), so the body's rounds() has K from one comparison. A cluster outside
    // it (set_tick moved the clock) sends its wave to the two-line path, which runs any K.
    strong = strong & (msel(lmid != 0, lth0 + P, lth0) - t0 < P);
  }
  const bool line0_wave = !__builtin_amdgcn_ballot_w64(active && !strong);   // uniform
  if (__builtin_expect(line0_wave, 1)) {
    // ----------------------------------------- the line-0 body: the whole launch in node order
    // (It stands right behind the decision: its state is dead before the other paths load their
    // lines. Behind them it stayed live across them and cost the N = 2 kernel a wave of occupancy.)
    // The wave ends here, where its body ends: its line stores, its counters and its return stand
    // in the instruction stream right behind the body, not behind the other paths' code.
#ifdef RS_WAVELOG
    asm volatile("" ::"v"(no.Ltr), "v"(no.Ldl), "v"(no.tr[0]), "v"(lth0));
    wl_x1 = wl_x2 = wall_clock64();           // fields extracted, the path decided
#endif
    if (__builtin_expect(active, 1)) {
      const LaunchBand lb{t0, parked_band()};
      run_launch(no, lmid, lth0, tend, d, hb, el_base, P, bs, lb);
      nhb = no.nhb; nae = no.nae; nar = no.nar;
#ifdef RS_WAVELOG
      asm volatile("" ::"v"(no.Ltr), "v"(no.tr[0]), "v"(no.Ldl));
      wl_x3 = wall_clock64();                 // the rounds done
#endif
      // Fields DEADLINE .. RES_TAIL of every node: the leader's value (at k == L) or the followers'
      // common one. A follower's deadline is the one its last append-entries of this launch set,
      // or the word as loaded when it took none.
      const uint32_t fqm = pack_qmeta(0, no.qin ? 1u : 0u, 0, 0), Lqm = pack_qmeta(0, 0, 0, no.rc);
      const uint32_t fra = no.qin ? no.qA : INF, frt = no.qin ? no.qA : 0u;
      const uint32_t Lrt = no.rc ? no.resA : 0u;
      auto val = [&](int q) -> uint32_t {
        const int f = (q - (int)HOT_CW) / N, k = (q - (int)HOT_CW) % N;
        const bool isL = no.L == (uint32_t)k;
        switch (f) {
          case HF_DEADLINE: return isL ? no.Ldl : no.took ? no.fdl : w[q];
          case HF_TRACE_LO: return (uint32_t)(isL ? no.Ltr : no.tr[k]);
          case HF_TRACE_HI: return (uint32_t)((isL ? no.Ltr : no.tr[k]) >> 32);
          case HF_QMETA: return isL ? Lqm : fqm;
          case HF_REQ_ARR: return isL ? INF : fra;
          case HF_RES_ARR: return isL ? no.resA : INF;
          case HF_REQ_TAIL: return isL ? 0u : frt;
          default: return isL ? Lrt : 0u;     // HF_RES_TAIL
        }
      };
      auto chunk = [&](int i) {
        return make_uint4(val(4 * i), val(4 * i + 1), val(4 * i + 2), val(4 * i + 3));
      };
      // There is no old line 1 to compare with: line 0 goes through the image, and the chunks past
      // it (the head and tail arrivals of messages in flight) change only for a cluster with a
      // round in progress at the launch's start or its end -- stored from registers.
      // Line 0 is dirty when the cluster ran an event here (an event changes a trace hash) and
      // clean when it ran none (every word written below is then the word as loaded, or derived
      // from it as the certificate says): no compare of the words.
#pragma unroll
      for (int i = (int)HOT_CW / 4; i < (CH_END < 8 ? CH_END : 8); ++i)
        *lds_at<uint4>(img, img_off(lane, i)) = chunk(i);
      dl = (nhb | nae | nar) != 0;
      if (CH_END > 8 && __builtin_expect(lmid || no.qin || no.rc, 0)) {   // rare
        uint4* const bp = reinterpret_cast<uint4*>(S.hot + (size_t)c * HB);
#pragma unroll
        for (int i = 8; i < CH_END; ++i) bp[i] = chunk(i);
      }
    }
    // messages in flight at the launch's end back to the rings, heads at slot 0 (rare)
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(active && (no.qin || no.rc)) != 0, 0)) {   // wave-uniform
      if (active && no.qin) {
#pragma unroll
        for (int k = 0; k < N; ++k) {
          if (no.L != (uint32_t)k) {
            uint4* dp = reinterpret_cast<uint4*>(qslots(S, c * N + k, 0));
            dp[0] = make_uint4(no.qA, RAFT_MSG_APPEND_ENTRIES | (no.L + 1) << 3, no.T, 0);
            dp[1] = make_uint4(0, 0, 0, 0);
          }
        }
      }
      uint4* rp = reinterpret_cast<uint4*>(qslots(S, c * N + no.L, 1));
      uint32_t n = 0;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        if (active && (uint32_t)j + no.rc >= (uint32_t)F) {
          uint4* dp = rp + 2 * n;
          dp[0] = make_uint4(no.resA, RAFT_MSG_APPEND_RESPONSE | no.sid(j) << 3 | 1u << 7, no.T, 0);
          dp[1] = make_uint4(0, 0, 0, 0);
          ++n;
        }
      }
    }
#ifdef RS_WAVELOG
    wl_lend = wall_clock64();                   // the image and the rings written
    // some cluster of the wave had a round in progress at the launch's start or at its end
    wl_cut = __builtin_amdgcn_ballot_w64(active && (lmid || no.qin || no.rc)) ? 1u : 0u;
    wl_sb = wall_clock64();
#endif
    // Only line 0 can be dirty here. The wave bailed no cluster (run_launch records none) and ran
    // no election (el is the general path's): no catch-up, no election counters. The kernel has
    // no workgroup barrier, so the wave's siblings run on without it.
    store_lines<N, 1>(S, img, cbase, lane, dl);
#ifdef RS_WAVELOG
    wave_record();
#endif
    add_counters<N>(S, lane, blockIdx.x * 4 + wave, nhb, nae, nar);
#ifdef RS_WAVELOG
    wave_done();
#endif
    return;
  }

  // The steady certificate (device.hpp): a cluster the last steady launch left at its fixed point
  // with leader L needs only the first two lines. The rest is loaded when some cluster of the wave
  // lacks one; otherwise those words read as the fixed point's (zero).
  uint32_t Lc = 0;
  bool cert = false, full = false;
  {
    load_line(1, true);
#pragma unroll
    for (int i = 32; i < NW4 * 4; ++i) w[i] = 0;
    read_chunks(8, NW4 < 16 ? NW4 : 16);
    uint32_t nlc = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const bool lead = fl_role(w[HOT_CW + HF_FLAGS * N + k]) == RAFT_LEADER;
      Lc = lead ? (uint32_t)k : Lc;
      nlc += lead;
    }
    static_assert(HOT_CW + (HF_FLAGS + 1) * N <= 64, "the flags are in the first two lines");
    cert = active && nlc == 1 &&
           (w[CL_CERT] == (CERT_MAGIC | Lc) || w[CL_CERT] == (CERT_STRONG | Lc));
    full = IMGC > 16 && __builtin_amdgcn_ballot_w64(active && !cert) != 0;   // uniform
    if (full) {
      load_half1();
      read_chunks(16, NW4);
    }
  }
  const bool vouched = cert && !full;         // its lines past the second are the fixed point's

  // ------------------------------------------- the certified path from two lines
  // A wave whose every cluster is vouched for by a certificate (device.hpp), on the fixed
  // point's period-P schedule (its round in progress at t0: none, the append-entries in flight, or
  // the responses the last launch's end cut) and with its followers' draws owed (FL_DRAW) runs the
  // whole launch from the first two lines of its blocks: the rest of that round, then the
  // rounds (run_launch). Queued messages are not read: a certified cluster's are the fixed point's
  // (whatever else writes a ring clears the certificate), and so are its leader's commit (0) and
  // the rest of its state. It leaves every cluster with a strong certificate: the next launch
  // takes the line-0 path above. Any other wave takes the general path below.
  FixedPoint<N> fx;                           // (set below, by the waves that use it)
  const LaunchBand no_band{t0, fpa::Band{0, 0, 0}};   // (FixedPoint's rounds() reads none of it)
  bool lean = false;
  {
    lean = vouched && cfg_ok;
    const uint32_t L = Lc;
    fx.L = L; fx.Lid = L + 1; fx.Lterm = lword(HF_TERM, L); fx.Lcommit = 0;
    fx.Ldl = lword(HF_DEADLINE, L);
    fx.Ltr = (uint64_t)lword(HF_TRACE_HI, L) << 32 | lword(HF_TRACE_LO, L);
    fx.qmask = fx.rmask = 0; fx.resA = INF; fx.fpend = allF; fx.nhb = fx.nae = fx.nar = 0;
    const uint32_t Lqm = lword(HF_QMETA, L);
    const uint32_t rsc = qm_res_cnt(Lqm);
    uint32_t need = 0;
#pragma unroll
    for (int j = 0; j < F; ++j) {
      fx.fdl[j] = fword(HF_DEADLINE, j, L);
      fx.ftr[j] = (uint64_t)fword(HF_TRACE_HI, j, L) << 32 | fword(HF_TRACE_LO, j, L);
      const uint32_t qm = fword(HF_QMETA, j, L);
      // (qm >> 4) & 31 is qm_req_cnt(qm), spelled out: through the reader the kernel's code changes
      lean = lean && (fword(HF_FLAGS, j, L) & FL_DRAW) && ((qm >> 4) & 31) <= 1 && !qm_res_cnt(qm);
      need |= (qm_req_cnt(qm) ? 1u : 0u) << j;
      fx.qA[j] = INF; fx.qT[j] = fx.qa[j] = fx.qb[j] = 0;
      fx.rT[j] = fx.rA[j] = fx.rB[j] = fx.rH[j] = 0;
    }
    lean = lean && !qm_req_cnt(Lqm) && rsc <= (uint32_t)F && !(need && rsc) &&
           (need == 0 || need == allF);
    const uint32_t ta = fword(HF_REQ_ARR, 0, L), ra = lword(HF_RES_ARR, L);
    const Schedule sc = schedule<F>(t0, tend, d, hb, P, fx.Ldl, need != 0, ta, rsc, ra);
    lean = lean && sc.on;
    lmid = sc.mid;
    lth0 = sc.th0;
    if (lmid == 1) {                                // every follower holds the append-entries
#pragma unroll
      for (int j = 0; j < F; ++j) {
        lean = lean && fword(HF_REQ_ARR, j, L) == ta;
        fx.qA[j] = ta; fx.qT[j] = fx.Lterm;
      }
      fx.qmask = allF;
    } else if (lmid == 2) {                         // the last rsc slots' responses, successful
      fx.rmask = allF & ~((1u << ((uint32_t)F - rsc)) - 1);
      fx.resA = ra;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        fx.rT[j] = fx.Lterm; fx.rH[j] = 1;
      }
    }
#pragma unroll
    for (int j = 0; j < F; ++j) lean = lean && fx.fdl[j] >= sc.nxt;
  }
  const bool lean_wave = !__builtin_amdgcn_ballot_w64(active && !lean);   // uniform
  bool wb = false;
  if (lean_wave) {
#ifdef RS_WAVELOG
    asm volatile("" ::"v"(fx.Ltr), "v"(fx.fdl[0]), "v"(fx.ftr[0]), "v"(lth0));
    wl_x1 = wl_x2 = wall_clock64();           // fields extracted, the path decided
#endif
    if (active) {
      run_launch(fx, lmid, lth0, tend, d, hb, el_base, P, bs, no_band);
      nhb = fx.nhb; nae = fx.nae; nar = fx.nar;
#ifdef RS_WAVELOG
      asm volatile("" ::"v"(fx.Ltr), "v"(fx.ftr[0]), "v"(fx.Ldl));
      wl_x3 = wall_clock64();                 // the rounds done
#endif
      // fields DEADLINE .. RES_TAIL of every node back into the image (the rest is unchanged)
      uint32_t v[HF_FLAGS][N];
#pragma unroll
      for (int k = 0; k < N; ++k) fx.node_words(k, v);
      auto val = [&](int q) { return v[(q - HOT_CW) / N][(q - HOT_CW) % N]; };
      auto chunk = [&](int i) {
        return make_uint4(val(4 * i), val(4 * i + 1), val(4 * i + 2), val(4 * i + 3));
      };
#pragma unroll
      for (int i = (int)HOT_CW / 4; i < CH_END; ++i) {
        const int q = 4 * i;
        const uint4 x = chunk(i);
        *lds_at<uint4>(img, img_off(lane, i)) = x;
        dl |= (uint32_t)(x.x != w[q] || x.y != w[q + 1] || x.z != w[q + 2] || x.w != w[q + 3])
              << (i / 8);
      }
      // the strong certificate and the leader's term (device.hpp), one chunk
      const uint32_t cn = CERT_STRONG | fx.L;
      *lds_at<uint4>(img, img_off(lane, CL_CERT / 4)) =
          make_uint4(w[CL_CERT - 3], w[CL_CERT - 2], fx.Lterm, cn);
      static_assert(CL_CTERM == CL_CERT - 1 && CL_CERT % 4 == 3, "one chunk");
      dl |= (uint32_t)(cn != w[CL_CERT] || fx.Lterm != w[CL_CTERM]);
    }
    fx.to_rings(S, c, active);
#ifdef RS_WAVELOG
    wl_lend = wall_clock64();                   // the image and the rings written
#endif
  } else {
#ifdef RS_WAVELOG
    wl_loop = wall_clock64();
#endif
    // ------------------------------------------- the election from init-node, in closed form
    // A cluster still in init-node's state (core.clj:31-38: every node a follower of the same term
    // with no vote, leader, log, leader-state or message; no checker mark) elects the node whose
    // timer fires first, and with no faults, no client and a fixed delay d that election is one
    // script when no other timer fires before the request-vote reaches it (D_k >= t1 + d):
    //   t1            candidate c times out (timeout-handler 166-169): term T + 1, request-vote
    //                 to every peer;
    //   t1 + d        every follower grants it (request-vote-handler 91-103: vote, no term change);
    //   t1 + 2d + i   c takes the i-th vote response in sender order (vote-response-handler
    //                 125-139) and is leader at the one that makes a majority (i_L), broadcasting
    //                 an empty append-entries (candidate->leader 80-84, append-entries-rpc 56-67);
    //   tL + d        every follower takes it (append-entries-handler 105-123: term T + 1, :follwer,
    //                 leader id) and answers; c takes the rest of the votes, then the F responses
    //                 one per tick from max(t1 + 2d + F, tL + 2d) (append-response-handler 141-149).
    // Every timer re-arm is one the general body defers (followers' draws stay owed), the leader's
    // rows end as init-node's (next = mb = 0, match = 0) and nothing is left queued: the script
    // writes the cluster's state after its last event into the registers below, and the cluster is
    // then at the fixed point, which the rest of this path runs to the launch's end (trace hashes,
    // deadlines and counters as the general body gives them). Two timers firing in the same tick
    // (delay 1) have a script of their own below. Anything else -- near ties, three timers, an
    // election cut by the launch's end, a state that only looks like init-node -- is bailed.
    {
      auto ifield = [&](int f, int k) { return w[HOT_CW + f * N + k]; };
      bool pat = active && w[CL_HWM_IDX] == 0 && S.Q >= 2u * F && el_base >= P && hb >= 2 * d + F;
      const uint32_t T = ifield(HF_TERM, 0);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        pat = pat && ifield(HF_FLAGS, k) == 0 && ifield(HF_MASKS, k) == 0 &&
              ifield(HF_TERM, k) == T && ifield(HF_COMMIT, k) == 0 && ifield(HF_LEN, k) == 0 &&
              ifield(HF_QMETA, k) == 0 && ifield(HF_REQ_ARR, k) == INF &&
              ifield(HF_RES_ARR, k) == INF;
#pragma unroll
        for (int p = 0; p < 2 * N; ++p) pat = pat && ifield(HF_NEXT + p, k) == 0;
      }
      pat = pat && T != INF;
      // the candidate: the earliest deadline (the lower index of two equal ones, a tie)
      uint32_t cidx = 0, t1 = INF, ntie = 0, bidx = 0;
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const uint32_t dk = ifield(HF_DEADLINE, k);
        cidx = dk < t1 ? (uint32_t)k : cidx;
        t1 = min(t1, dk);
      }
      bool single = true;
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const uint32_t dk = ifield(HF_DEADLINE, k);
        ntie += dk == t1;
        bidx = dk == t1 && (uint32_t)k != cidx ? (uint32_t)k : bidx;
        single = single && ((uint32_t)k == cidx || (uint64_t)dk >= (uint64_t)t1 + d);
      }
      // two timers firing together (the delay 1: every other one is then at least d later)
      const bool tie = ntie == 2 && d == 1 && N >= 3;
      constexpr uint32_t iL = (N + 1) / 2 >= 2 ? (N + 1) / 2 - 2 : 0;   // the electing response
      const uint64_t tL = (uint64_t)t1 + 2 * d + iL;
      const uint64_t tau0 = max((uint64_t)t1 + 2 * d + F, tL + 2 * d);  // the first response
      const uint64_t tlast = tau0 + F - 1;
      pat = pat && (single || tie) && t1 >= t0 && (tie || tlast < tend) &&
            (uint64_t)t1 + 4 * N + 8 < 0xFFFFFFFFull;
      // the election-safety check (P4) compares the new leader's led term with the others'
      // (words past the image: read only when some cluster of the wave qualifies)
      if (__builtin_amdgcn_ballot_w64(pat)) {                 // wave-uniform
        const uint32_t* lp = S.hot + (size_t)c * HB + HOT_CW + hf_led(N) * N;
        uint32_t led[N];
#pragma unroll
        for (int k = 0; k < N; ++k) led[k] = lp[k];
#pragma unroll
        for (int k = 0; k < N; ++k) pat = pat && ((uint32_t)k == cidx || led[k] != T + 1);
      }
      const uint32_t T1 = T + 1, cid = cidx + 1, peers = ((1u << (N + 1)) - 1) & ~1u & ~(1u << cid);
      if (pat && single) {
        el = true;
        el_to = 1;
        // the candidate's events (node cidx), then each follower's
        uint64_t hc = 0;
#pragma unroll
        for (int k = 0; k < N; ++k)
          if ((uint32_t)k == cidx)
            hc = (uint64_t)ifield(HF_TRACE_HI, k) << 32 | ifield(HF_TRACE_LO, k);
        hc = trace_event(hc, t1, 6, 0, 0, RAFT_CANDIDATE, T1, 0);
#pragma unroll
        for (int i = 0; i < F; ++i) {
          const uint32_t sid = (uint32_t)i + ((uint32_t)i >= cidx ? 2u : 1u);   // slot i's id
          hc = trace_event(hc, t1 + 2 * d + i, RAFT_MSG_VOTE_RESPONSE, sid, T,
                           (uint32_t)i >= iL ? RAFT_LEADER : RAFT_CANDIDATE, T1, 0);
        }
#pragma unroll
        for (int j = 0; j < F; ++j) {
          const uint32_t sid = (uint32_t)j + ((uint32_t)j >= cidx ? 2u : 1u);
          hc = trace_event(hc, (uint32_t)tau0 + j, RAFT_MSG_APPEND_RESPONSE, sid, T, RAFT_LEADER,
                           T1, 0);
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const bool isc = (uint32_t)k == cidx;
          uint64_t h = (uint64_t)ifield(HF_TRACE_HI, k) << 32 | ifield(HF_TRACE_LO, k);
          h = trace_event(h, t1 + d, RAFT_MSG_REQUEST_VOTE, cid, T1, RAFT_FOLLOWER, T, 0);
          h = trace_event(h, (uint32_t)tL + d, RAFT_MSG_APPEND_ENTRIES, cid, T1, RAFT_FOLLWER, T1, 0);
          h = isc ? hc : h;
          w[HOT_CW + HF_FLAGS * N + k] = isc ? pack_flags(RAFT_LEADER, 0, cid, 0, 0, 1)
                                             : pack_flags(RAFT_FOLLWER, 0, cid, 0, 0, 0) | FL_DRAW;
          w[HOT_CW + HF_MASKS * N + k] = isc ? peers << 16 : 0u;
          w[HOT_CW + HF_TERM * N + k] = T1;
          w[HOT_CW + HF_DEADLINE * N + k] = isc ? (uint32_t)tlast + hb
                                                : (uint32_t)tL + d + el_base;     // + the owed draw
          w[HOT_CW + HF_REQ_TAIL * N + k] = 0;
          w[HOT_CW + HF_RES_TAIL * N + k] = 0;
          w[HOT_CW + HF_TRACE_LO * N + k] = (uint32_t)h;
          w[HOT_CW + HF_TRACE_HI * N + k] = (uint32_t)(h >> 32);
        }
        nae = F;                                    // the followers' append-entries and their
        nar = F;                                    // responses (the rest is counted as el_to)
      } else if (pat && tie) {
        // Two timers at t1 (d = 1): candidates a < b (ids A, B) both time out and send
        // request-votes; at t1 + 1 every other node grants A's (the lower id's, queued first) and
        // a and b deny each other (each voted for itself); at t1 + 2 those nodes deny B's. a takes
        // its vote responses one per tick from t1 + 2 in sender order and is leader at the
        // majority's one (tL); b takes a's denial at t1 + 2, then the others' from t1 + 3, and
        // a's append-entries when it arrives at tL + 1 -- when both of b's queues are ready the
        // alts!! bit of its EVENT draw picks (core.clj:181), and that draw re-arms its timer
        // exactly. a then takes the responses: the others' at tL + 2 and b's the tick after b
        // took the append-entries, by (arrival, sender id).
        const uint32_t a = cidx, b = bidx, B = b + 1;
        const uint32_t A = cid;
        constexpr uint32_t M = (N + 1) / 2;                  // majority? (core.clj:19-21)
        uint64_t ha = 0, hbb = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const uint64_t h0 = (uint64_t)ifield(HF_TRACE_HI, k) << 32 | ifield(HF_TRACE_LO, k);
          if ((uint32_t)k == a) ha = h0;
          if ((uint32_t)k == b) hbb = h0;
        }
        ha = trace_event(ha, t1, 6, 0, 0, RAFT_CANDIDATE, T1, 0);
        ha = trace_event(ha, t1 + 1, RAFT_MSG_REQUEST_VOTE, B, T1, RAFT_CANDIDATE, T1, 0);
        uint32_t votes = 1, tLt = INF, role = RAFT_CANDIDATE;
#pragma unroll
        for (int k = 0; k < N; ++k) {                        // a's vote responses, id order
          if ((uint32_t)k == a) continue;
          const uint32_t i = (uint32_t)k - ((uint32_t)k > a ? 1u : 0u), tau = t1 + 2 + i;
          const bool grant = (uint32_t)k != b;
          if (grant && role == RAFT_CANDIDATE && ++votes >= M) {
            role = RAFT_LEADER;
            tLt = tau;
          }
          ha = trace_event(ha, tau, RAFT_MSG_VOTE_RESPONSE, (uint32_t)k + 1, grant ? T : T1, role,
                           T1, 0);
        }
        // b: the denials, then a's append-entries
        hbb = trace_event(hbb, t1, 6, 0, 0, RAFT_CANDIDATE, T1, 0);
        hbb = trace_event(hbb, t1 + 1, RAFT_MSG_REQUEST_VOTE, A, T1, RAFT_CANDIDATE, T1, 0);
        hbb = trace_event(hbb, t1 + 2, RAFT_MSG_VOTE_RESPONSE, A, T1, RAFT_CANDIDATE, T1, 0);
        uint32_t tb = t1 + 3, j = 0, tbae = INF, brole = RAFT_CANDIDATE, bdl = 0;
        bool bexact = false;
        for (int it = 0; it < N + 1; ++it) {
          const bool res = j < (uint32_t)N - 2, req = tbae == INF;
          if (!res && !req) break;
          if (!res && tb < tLt + 1) tb = tLt + 1;             // idle until the append-entries
          const bool rq = req && tb >= tLt + 1;
          bool take_req = rq;
          bexact = false;
          if (res && rq) {                                    // alts!! (core.clj:181)
            const uint4 ew = event_draw(g, B, tb, S);
            take_req = !(ew.x & 1);
            bexact = true;
            bdl = tb + el_base + __umulhi(ew.y, S.el_span);
          }
          if (take_req) {                                     // append-entries-handler 105-123
            hbb = trace_event(hbb, tb, RAFT_MSG_APPEND_ENTRIES, A, T1, RAFT_FOLLWER, T1, 0);
            brole = RAFT_FOLLWER;
            tbae = tb;
          } else {                                            // the j-th other node's denial
            uint32_t fid = 0, cnt = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) {
              const bool other = (uint32_t)k != a && (uint32_t)k != b;
              fid = other && cnt == j ? (uint32_t)k + 1 : fid;
              cnt += other;
            }
            hbb = trace_event(hbb, tb, RAFT_MSG_VOTE_RESPONSE, fid, T, brole, T1, 0);
            ++j;
          }
          if (!bexact) bdl = tb + el_base;                    // + the owed draw
          ++tb;
        }
        const uint32_t tbl = tb - 1;                          // b's last event
        // a's responses: the others' at tLt + 2, b's at tbae + 1, by (arrival, sender id)
        uint32_t ta = t1 + N + 1;                             // after its N - 1 vote responses
        const uint32_t fa = tLt + 2, ba = tbae + 1;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          if ((uint32_t)k == a) continue;
          const bool isb = (uint32_t)k == b;
          if (isb && ba != fa) continue;
          ta = max(ta, fa);
          ha = trace_event(ha, ta, RAFT_MSG_APPEND_RESPONSE, (uint32_t)k + 1, isb ? T1 : T,
                           RAFT_LEADER, T1, 0);
          ++ta;
        }
        if (ba != fa) {
          ta = max(ta, ba);
          ha = trace_event(ha, ta, RAFT_MSG_APPEND_RESPONSE, B, T1, RAFT_LEADER, T1, 0);
          ++ta;
        }
        const uint32_t tal = ta - 1;                          // a's last event
        if (tbae != INF && tLt != INF && max(tal, tbl) < tend) {
          el = true;
          el_to = 2;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const bool isa = (uint32_t)k == a, isb = (uint32_t)k == b;
            uint64_t h = (uint64_t)ifield(HF_TRACE_HI, k) << 32 | ifield(HF_TRACE_LO, k);
            h = trace_event(h, t1 + 1, RAFT_MSG_REQUEST_VOTE, A, T1, RAFT_FOLLOWER, T, 0);
            h = trace_event(h, t1 + 2, RAFT_MSG_REQUEST_VOTE, B, T1, RAFT_FOLLOWER, T, 0);
            h = trace_event(h, tLt + 1, RAFT_MSG_APPEND_ENTRIES, A, T1, RAFT_FOLLWER, T1, 0);
            h = isa ? ha : isb ? hbb : h;
            w[HOT_CW + HF_FLAGS * N + k] =
                isa ? pack_flags(RAFT_LEADER, 0, A, 0, 0, 1)
                    : pack_flags(RAFT_FOLLWER, 0, A, 0, 0, 0) | (isb && bexact ? 0u : FL_DRAW);
            w[HOT_CW + HF_MASKS * N + k] = isa ? peers << 16 : 0u;
            w[HOT_CW + HF_TERM * N + k] = T1;
            w[HOT_CW + HF_DEADLINE * N + k] = isa ? tal + hb : isb ? bdl : tLt + 1 + el_base;
            w[HOT_CW + HF_REQ_TAIL * N + k] = 0;
            w[HOT_CW + HF_RES_TAIL * N + k] = 0;
            w[HOT_CW + HF_TRACE_LO * N + k] = (uint32_t)h;
            w[HOT_CW + HF_TRACE_HI * N + k] = (uint32_t)(h >> 32);
          }
          nae = F;
          nar = F;
        }
      }
    }
    // exactly one leader; every node running; only the leader has leader-state
    uint32_t L = 0, nlead = 0, badn = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const uint32_t f = word(HF_FLAGS, k);
      const bool lead = fl_role(f) == RAFT_LEADER;
      L = lead ? (uint32_t)k : L;
      nlead += lead;
      badn |= fl_fault(f) | (lead != (fl_lsp(f) != 0)) | (lead && (f & FL_DRAW));
    }
    bool bad = !active || nlead != 1 || badn != 0 || S.Q < (uint32_t)F;
    const uint32_t Lid = L + 1;
    // The leader's registers and, per follower slot, the followers'. What the fixed point's events
    // change -- deadlines, trace hashes, the messages in flight, the counters -- is fx's, so those
    // events (run_launch, rounds) run on this path's state as it stands.
    const uint32_t Lfl = lword(HF_FLAGS, L), Lterm = lword(HF_TERM, L);
    const uint32_t Lcommit = lword(HF_COMMIT, L), Llen = lword(HF_LEN, L);
    uint32_t Lmk = lword(HF_MASKS, L);
    fx.L = L; fx.Lid = Lid; fx.Lterm = Lterm; fx.Lcommit = Lcommit;
    fx.Ldl = lword(HF_DEADLINE, L);
    fx.Ltr = (uint64_t)lword(HF_TRACE_HI, L) << 32 | lword(HF_TRACE_LO, L);
    fx.nhb = nhb; fx.nae = nae; fx.nar = nar;        // (an election's, above)
    uint32_t ffl[F], fmk[F], fterm[F], fcommit[F], flen[F];
    // the leader's rows for its followers: next_index / match_index of peer id fk(j) + 1; and as
    // loaded: unchanged words are not stored back
    int32_t nx[F], mt[F], nx0[F], mt0[F];
#pragma unroll
    for (int j = 0; j < F; ++j) {
      ffl[j] = fword(HF_FLAGS, j, L);
      fmk[j] = fword(HF_MASKS, j, L);
      fterm[j] = fword(HF_TERM, j, L);
      fcommit[j] = fword(HF_COMMIT, j, L);
      flen[j] = fword(HF_LEN, j, L);
      fx.fdl[j] = fword(HF_DEADLINE, j, L);
      fx.ftr[j] = (uint64_t)fword(HF_TRACE_HI, j, L) << 32 | fword(HF_TRACE_LO, j, L);
      const bool up = (uint32_t)j >= L;
      nx[j] = nx0[j] = (int32_t)msel(up, lword(HF_NEXT + j + 1, L), lword(HF_NEXT + j, L));
      mt[j] = mt0[j] = (int32_t)msel(up, lword(HF_NEXT + N + j + 1, L), lword(HF_NEXT + N + j, L));
    }
    const bool ackbad = Llen > w[CL_HWM_IDX];          // a success response would be checker work (P4)
    const uint32_t Lkeys = Lmk >> 16;
    // heartbeats need full leader-state, no LazySeq log and commit within the log
    // (append-entries-rpc's IOOBE/NPE/CCE checks, core.clj:56-67): constant over the launch
    bad = bad || (Lkeys & (((1u << (N + 1)) - 1) & ~1u & ~(1u << Lid))) !=
                     (((1u << (N + 1)) - 1) & ~1u & ~(1u << Lid)) ||
          (Lfl & FL_SEQ) || Lcommit > Llen;

#ifdef RS_WAVELOG
    asm volatile("" ::"v"(fx.Ltr), "v"(fx.fdl[0]), "v"(nx[0]));
    wl_x1 = wall_clock64();                     // fields extracted
#endif
    // ---------------------------------------------------------------- queued messages
    fx.qmask = 0; fx.rmask = 0; fx.resA = INF;
#pragma unroll
    for (int j = 0; j < F; ++j) {
      fx.qA[j] = INF; fx.qT[j] = fx.qa[j] = fx.qb[j] = 0;
      fx.rT[j] = fx.rA[j] = fx.rB[j] = fx.rH[j] = 0;
    }
    if (!bad) {
      const uint32_t Lqm = lword(HF_QMETA, L);
      bad = qm_req_cnt(Lqm);                                   // the leader's REQ queue is empty
      const uint32_t rsh = qm_res_head(Lqm), rsc = qm_res_cnt(Lqm);
      uint32_t need = 0, rqh[F];
#pragma unroll
      for (int j = 0; j < F; ++j) {
        const uint32_t qm = fword(HF_QMETA, j, L);
        const uint32_t rqc = qm_req_cnt(qm);
        rqh[j] = qm_req_head(qm);
        bad = bad || rqc > 1 || qm_res_cnt(qm) != 0;       // <= 1 request, no responses
        need |= (uint32_t)(rqc != 0) << j;
      }
      bad = bad || rsc > (uint32_t)F;
      // The messages: loaded by every lane of a wave in which any lane has one (a message in flight
      // at the launch's start is rare), all loads issued before any is looked at -- one memory round
      // trip, where loads under per-lane branches each waited for the last. Slot indices are
      // clamped into the ring for lanes whose queue words are not looked at.
      uint4 qm0[F], qm1[F], rm0[F], rm1[F];
      if (__builtin_amdgcn_ballot_w64(!bad && (need || rsc))) {     // wave-uniform
#pragma unroll
        for (int j = 0; j < F; ++j) {                          // the leader's append-entries
          const uint4* mp = reinterpret_cast<const uint4*>(
              qslots(S, c * N + fx.fk(j), 0) + min(rqh[j], S.Q - 1) * qstride(S, 0));
          qm0[j] = mp[0];
          qm1[j] = mp[1];
        }
#pragma unroll
        for (int i = 0; i < F; ++i) {                          // append-responses, sender order
          const uint4* mp = reinterpret_cast<const uint4*>(
              qslots(S, c * N + L, 1) + min(wrapq(rsh + i, S.Q), S.Q - 1) * qstride(S, 1));
          rm0[i] = mp[0];
          rm1[i] = mp[1];
        }
      }
      if (!bad) {
#pragma unroll
        for (int j = 0; j < F; ++j) {
          if ((need >> j) & 1) {
            const uint4 m0 = qm0[j], m1 = qm1[j];
            bad = bad || m0.y != (RAFT_MSG_APPEND_ENTRIES | Lid << 3) || m1.y || m1.z || m1.w;
            fx.qmask |= 1u << j;
            fx.qA[j] = m0.x; fx.qT[j] = m0.z; fx.qa[j] = m0.w; fx.qb[j] = m1.x;
          }
        }
        uint32_t last = 0;
#pragma unroll
        for (int i = 0; i < F; ++i) {
          if ((uint32_t)i < rsc && !bad) {
            const uint4 m0 = rm0[i], m1 = rm1[i];
            const uint32_t hdr = m0.y, src = (hdr >> 3) & 15;
            bad = (hdr & 7) != RAFT_MSG_APPEND_RESPONSE || (hdr >> 8) || m1.y || m1.z || m1.w ||
                  src <= last || src > (uint32_t)N || src == Lid || (i && m0.x != fx.resA);
            last = src;
            fx.resA = m0.x;
            const uint32_t j = src - 1 - (src > Lid ? 1u : 0u);
            if (!bad) {
              fx.rmask |= 1u << j;
#pragma unroll
              for (int jj = 0; jj < F; ++jj) {
                if ((uint32_t)jj == j) {
                  fx.rT[jj] = m0.z; fx.rA[jj] = m0.w; fx.rB[jj] = m1.x; fx.rH[jj] = (hdr >> 7) & 1;
                }
              }
            }
          }
        }
      }
      if (!fx.rmask) fx.resA = INF;
    }
    record_bail(active && bad, t0);           // outside the model from the start: bail at t0
    wb = active && !bad;
    bool run = wb;

    // ---------------------------------------------------------------- the cluster's ticks
    uint32_t tn = t0;
    // followers whose deadline holds its lower bound t_ae + el_base (the draw is deferred)
    // (a draw owed from an earlier launch: FL_DRAW in the follower's flags, device.hpp)
    fx.fpend = 0;
#pragma unroll
    for (int j = 0; j < F; ++j) fx.fpend |= ((ffl[j] & FL_DRAW) ? 1u : 0u) << j;
    auto draw_deadlines = [&](uint32_t due) {
#pragma unroll
      for (int j = 0; j < F; ++j) {
        if ((due >> j) & 1) {
          const uint4 wd = event_draw(g, fx.fk(j) + 1, fx.fdl[j] - el_base, S);   // D4, core.clj:174
          fx.fdl[j] += __umulhi(wd.y, S.el_span);
        }
      }
      fx.fpend &= ~due;
    };
    auto next_event = [&]() {
      uint32_t m = min(fx.Ldl, fx.resA);
#pragma unroll
      for (int j = 0; j < F; ++j) m = min(m, min(fx.fdl[j], fx.qA[j]));
      return m;
    };
    // The cluster at its fixed point: every follower took the leader's append-entries (flags,
    // votes, term and commit are what another one sets again), every response succeeded (next /
    // match / keys as another one sets them), the log is empty (a heartbeat ships nothing) and no
    // message is in flight. If the followers' re-armed timers (>= t_ae + el_base) cannot fire
    // before the next round's append-entries (el_base >= the round period P) and the leader's
    // responses all fit before its next heartbeat (hb >= 2d + F), every later round is this one
    // shifted by a multiple of P: only the ticks in the trace hashes change.
    auto at_fixed_point_state = [&]() {
      bool ok = Llen == 0 && !ackbad;
#pragma unroll
      for (int j = 0; j < F; ++j)
        ok = ok && fterm[j] == Lterm &&
             (ffl[j] & FL_FOLLOW) == pack_flags(RAFT_FOLLWER, 0, Lid, 0, 0, 0) &&
             fcommit[j] == flen[j] && (fmk[j] & 0xFFFFu) == 0 && nx[j] == 0 &&
             mt[j] == (int32_t)Lcommit;
      return ok;
    };
    auto at_fixed_point = [&]() {
      return el_base >= P && hb >= 2 * d + F && !fx.qmask && !fx.rmask && at_fixed_point_state();
    };
    auto fixed_point_rounds = [&](uint32_t th) { rounds(fx, th, tend, d, hb, el_base, bs, no_band); };

    // ------------------------------------------- the fixed-point path (C2's steady state)
    // A cluster at its fixed point (above) whose round in progress at t0 is on the period-P
    // schedule -- none (the next heartbeat at Ldl >= t0), its append-entries in flight, or its
    // responses pending exactly as the last launch's end cut them -- and whose followers' timers
    // cannot fire before their next append-entries runs every event of the launch here: the rest
    // of that round, then the rounds (run_launch). Everything else is the general loop's.
    bool fp = wb && el_base >= P && hb >= 2 * d + F && (vouched || at_fixed_point_state());
    // (the round's heartbeat th0; mid: 1 append-entries in flight, 2 responses)
    const Schedule sc = schedule<F>(t0, tend, d, hb, P, fx.Ldl, fx.qmask != 0, fx.qA[0],
                                    __popc(fx.rmask), fx.resA);
    const uint32_t th0 = sc.th0, mid = sc.mid;
    fp = fp && sc.on;
    if (mid == 1) {                            // every follower holds the same empty append-entries
      fp = fp && fx.qmask == allF && !fx.rmask;
#pragma unroll
      for (int j = 0; j < F; ++j)
        fp = fp && fx.qA[j] == fx.qA[0] && fx.qT[j] == Lterm && fx.qa[j] == Lcommit && fx.qb[j] == 0;
    } else if (mid == 2) {                     // the last slots' responses, successful
      fp = fp && fx.rmask == (allF & ~((1u << ((uint32_t)F - __popc(fx.rmask))) - 1));
#pragma unroll
      for (int j = 0; j < F; ++j)
        fp = fp && (!((fx.rmask >> j) & 1) ||
                    (fx.rT[j] == Lterm && fx.rA[j] == Lcommit && fx.rB[j] == 0 && fx.rH[j] == 1));
    }
#pragma unroll
    for (int j = 0; j < F; ++j) fp = fp && fx.fdl[j] >= sc.nxt;
    // A vouched cluster off the fixed-point path (set_tick moved the clock, ...) has no full state
    // here: the general body runs it from t0.
    const bool vbail = vouched && wb && !fp;
    record_bail(vbail, t0);
    if (vbail) wb = run = false;
#ifdef RS_WAVELOG
    asm volatile("" ::"v"(fp), "v"(th0));
    wl_x2 = wall_clock64();                     // queued messages read, fixed-point path decided
#endif
    if (fp) {
      run = false;
      run_launch(fx, mid, th0, tend, d, hb, el_base, P, bs, no_band);
    }
#ifdef RS_WAVELOG
    asm volatile("" ::"v"(fx.Ltr), "v"(fx.ftr[0]), "v"(fx.Ldl));
    wl_x3 = wall_clock64();                     // the fixed-point path's rounds done
#endif
#ifdef RS_WAVELOG
    wl_ts = __builtin_amdgcn_s_memtime();
#endif
    bool pbail = false;                        // bailed in the last trip, not yet recorded
    uint32_t pbt = 0;
    for (;;) {
      record_bail(pbail, pbt);                 // the loop's head: every lane active
      pbail = false;
      uint32_t t = max(tn, next_event());
      // a deferred deadline at or before the tick to decide is drawn first (it can only move later)
      for (;;) {
        uint32_t due = 0;
#pragma unroll
        for (int j = 0; j < F; ++j) due |= (uint32_t)(fx.fdl[j] <= t) << j;
        due &= fx.fpend;
        if (!run || t >= tend || !due) break;
        draw_deadlines(due);
        t = max(tn, next_event());
      }
      const bool on = run && t < tend;
      if (!__builtin_amdgcn_ballot_w64(on)) break;
#ifdef RS_WAVELOG
      if (!wl_trips) wl_first = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(on));
      ++wl_trips;
#endif
      RS_LPH(0);
      if (!on) continue;
      // ------------------------------------------------ decide on the pre-tick state
      const bool lres = fx.rmask != 0 && fx.resA <= t;               // a message beats the deadline
      const bool lhb = !lres && fx.Ldl <= t;
      uint32_t fae = 0, fto = 0;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        const bool a = fx.qA[j] <= t;
        fae |= (uint32_t)a << j;
        fto |= (uint32_t)(!a && fx.fdl[j] <= t) << j;
      }
      bool bail = fto != 0;                                    // a follower's election timeout
      if (lhb) {
        bail = bail || fx.qmask != 0;                             // a follower still holds one
#pragma unroll
        for (int j = 0; j < F; ++j) {
          const uint32_t pv = nx[j] - 1 > 0 ? (uint32_t)(nx[j] - 1) : 0u;
          bail = bail || pv < Llen || pv >= (1u << 24);        // entries to ship
        }
      }
      const int hs = __builtin_ctz(fx.rmask | (1u << F));
      uint32_t xT = 0, xH = 0;
#pragma unroll
      for (int j = 0; j < F; ++j) {
        if (j == hs) {
          xT = fx.rT[j]; xH = fx.rH[j];
        }
      }
      const uint32_t xid = (uint32_t)hs + 1 + ((uint32_t)hs >= L ? 1u : 0u);
      if (lres)
        bail = bail || xT > Lterm || (xH ? ackbad : ((Lmk >> (16 + xid)) & 1) == 0);
      if (fae) {
        bail = bail || fx.rmask != 0;                             // responses of two ticks
#pragma unroll
        for (int j = 0; j < F; ++j)
          if ((fae >> j) & 1)
            bail = bail || fx.qb[j] != 0 || !(fx.qT[j] < fterm[j] || flen[j] <= fcommit[j]);
      }
      RS_LPH(1);
      if (bail) {                              // the general tick body runs this tick
        pbail = true;
        pbt = t;
        run = false;
        continue;
      }
      // ------------------------------------------------ run
      uint32_t tl = t;                         // the last tick run (a round or a drain runs more)
      bool round = false;
      if (lhb) {                               // heartbeat-handler: empty append-entries to all
#pragma unroll
        for (int j = 0; j < F; ++j) {
          fx.qA[j] = t + d; fx.qT[j] = Lterm; fx.qa[j] = Lcommit;
          fx.qb[j] = nx[j] - 1 > 0 ? (uint32_t)(nx[j] - 1) : 0u;
        }
        fx.qmask = (1u << F) - 1;
        fx.Ldl = t + hb;
        fx.Ltr = trace_event(fx.Ltr, t, 7, 0, 0, RAFT_LEADER, Lterm, 0);
        ++fx.nhb;
        // The whole heartbeat round in this trip when nothing else can happen before its last
        // response: every follower takes the append-entries at t + d (no follower deadline before
        // it; the handler's checks pass), the followers' re-armed deadlines (>= t + d + el_base) and
        // the leader's (t + hb) fall after the responses at t + 2d .. t + 2d + F - 1, and the
        // append-entries come before the launch ends (and no older response is still queued). The
        // responses then run in slot order up to the launch end (the rest stay queued) and stop at
        // one outside the model (the next trip decides it). A deferred deadline counts with its
        // lower bound here (a round not taken is run tick by tick).
        round = fx.rmask == 0 && hb >= 2 * d + F && el_base >= d + F && tend - t > d;
#pragma unroll
        for (int j = 0; j < F; ++j)
          round = round && fx.fdl[j] >= t + d && fx.qb[j] == 0 &&
                  (Lterm < fterm[j] || flen[j] <= fcommit[j]);
      }
      RS_LPH(2);
      // A trip runs exactly one of: a whole round (below), a heartbeat alone (its round did not fit:
      // the append-entries are taken one tick later as `fae`), append-entries that arrived (fae),
      // or queued responses (lres): a heartbeat with a follower still holding an append-entries,
      // and append-entries with responses still queued, were bailed above.
      auto append_entries = [&](uint32_t ta, uint32_t fa) {   // append-entries-handler, followers fa
#pragma unroll
        for (int j = 0; j < F; ++j) {
          if ((fa >> j) & 1) {
            const uint32_t mterm = fx.qT[j], rterm = fterm[j];
            const bool ok = mterm >= fterm[j];
            const uint32_t nfl2 = ok ? (ffl[j] & ~FL_FOLLOW) |
                                           pack_flags(RAFT_FOLLWER, 0, Lid, 0, 0, 0)
                                     : ffl[j];
            const uint32_t nterm = ok ? mterm : fterm[j];
            fx.ftr[j] = trace_event(fx.ftr[j], ta, RAFT_MSG_APPEND_ENTRIES, Lid, mterm, fl_role(nfl2),
                                    nterm, 0);
            if (ok) {
              fcommit[j] = flen[j];                            // apply-entries! (nothing applied)
              fmk[j] &= 0xFFFF0000u;
            }
            fterm[j] = nterm;
            ffl[j] = nfl2;
            // the response: to the leader's RES queue, in sender id order
            fx.rT[j] = rterm; fx.rA[j] = ok ? fx.qa[j] : 0u; fx.rB[j] = 0; fx.rH[j] = ok;
            fx.qA[j] = INF;
            fx.fdl[j] = ta + el_base;                             // + the deferred draw
          }
        }
        fx.fpend |= fa;
        fx.qmask &= ~fa;
        fx.rmask = fa;
        fx.resA = ta + d;
        fx.nae += __popc(fa);
        tl = ta;
      };
      // append-response-handler for follower slot j's response at tick tau (core.clj:141-149);
      // false (and nothing done) when it is outside the model: a newer term, a success response
      // that would be checker work, or a failure without the peer's key (NPE)
      auto response = [&](int j, uint32_t tau, uint32_t yT, uint32_t yA, uint32_t yB, uint32_t yH,
                          int32_t& nxj, int32_t& mtj) {
        const uint32_t yid = fx.fk(j) + 1;
        if (yT > Lterm || (yH ? ackbad : ((Lmk >> (16 + yid)) & 1) == 0)) return false;
        fx.rmask &= ~(1u << j);
        Lmk |= yH << (16 + yid);
        nxj = yH ? (int32_t)yB : nxj - 1;
        mtj = yH ? (int32_t)yA : mtj;
        fx.Ldl = tau + hb;
        fx.Ltr = trace_event(fx.Ltr, tau, RAFT_MSG_APPEND_RESPONSE, yid, yT, RAFT_LEADER, Lterm, 0);
        ++fx.nar;
        tl = tau;
        return true;
      };
      if (round) {
        // every follower at t + d, then the responses at t + 2d .. t + 2d + F - 1 in slot order (the
        // round's conditions put them all before the launch end and every follower's next event):
        // straight-line code, every index static
        append_entries(t + d, (1u << F) - 1);
        bool go = true;
#pragma unroll
        for (int j = 0; j < F; ++j)     // (a round cut by the launch end leaves the rest queued)
          go = go && t + 2 * d + j < tend &&
               response(j, t + 2 * d + j, fx.rT[j], fx.rA[j], fx.rB[j], fx.rH[j], nx[j], mt[j]);
        if (!fx.rmask) fx.resA = INF;
        if (at_fixed_point()) {
          fixed_point_rounds(t + P);
          tl = tend - 1;                       // nothing of the cluster is left before tend
        }
      } else if (fae || lres) {
        // fae: the append-entries at t, then their responses from t + d in the same trip unless
        // the leader's heartbeat falls due before them. The responses run one per tick, heads in
        // sender order, while nothing else in the cluster is due (the followers' next events and
        // the launch end; the leader's own deadline moves past each); lres: the first one at t
        // was decided above. A response outside the model ends the run and the next trip
        // decides it. A round finished here (one the last launch cut) continues at the fixed point.
        uint32_t tau0 = t;
        if (fae) {
          append_entries(t, fae);
          tau0 = fx.Ldl >= t + d ? t + d : tend;
        }
        uint32_t E = tend;
#pragma unroll
        for (int j = 0; j < F; ++j) E = min(E, min(fx.fdl[j], fx.qA[j]));
        if (lres) E = max(E, t + 1);
        for (uint32_t tau = tau0; fx.rmask && tau < E; ++tau) {
          const int h2 = __builtin_ctz(fx.rmask);
          bool ok = true;
#pragma unroll
          for (int j = 0; j < F; ++j)
            if (j == h2) ok = response(j, tau, fx.rT[j], fx.rA[j], fx.rB[j], fx.rH[j], nx[j], mt[j]);
          if (!ok) break;
          if (!fx.rmask) fx.resA = INF;
        }
        // The round finished here need not be on the period-P schedule. Responses that waited
        // behind the leader's other events (an election's vote responses, one per tick), or a
        // deadline the host wrote, put its next heartbeat after th + P, while el_base >= P keeps a
        // follower's timer (>= t_ae + el_base) no earlier than th + P + d: with el_base at or near
        // P it fires before the next append-entries. The cluster continues from the fixed point
        // only if every follower's deadline (its lower bound, where the draw is owed) holds until
        // that append-entries arrives (a tie: the message wins, SIM_SPEC P1) or to the launch's
        // end; otherwise it is run tick by tick.
        bool quiet = at_fixed_point() && fx.Ldl > tl;
        {
          // the next AE (or the end)
          const uint32_t nxt = (uint32_t)min((uint64_t)fx.Ldl + d, (uint64_t)tend);
#pragma unroll
          for (int j = 0; j < F; ++j) quiet = quiet && fx.fdl[j] >= nxt;
        }
        if (quiet) {
          fixed_point_rounds(fx.Ldl);
          tl = tend - 1;
        }
      }
      RS_LPH(4);
      tn = tl + 1;
    }
    // the draws still owed stay owed in the stored state (FL_DRAW): a cluster at its fixed point
    // makes none at all

#ifdef RS_WAVELOG
    wl_lend = wall_clock64();
#endif
    // ---------------------------------------------------------------- write back
    if (S.shist) {
      // packing key for the next launch (bailed clusters get theirs from the catch-up below); the
      // wave's clusters share a few keys: one histogram atomic per distinct key
      const bool kl = wb && run;
      const uint32_t key = kl ? sched_bucket(next_event(), tend) : INF;
      if (kl) S.skey[c] = key;
      uint64_t pend = __builtin_amdgcn_ballot_w64(kl);
      while (pend) {
        const uint32_t k = (uint32_t)__shfl((int)key, (int)__builtin_ctzll(pend));
        const uint64_t same = __builtin_amdgcn_ballot_w64(kl && key == k);
        if (lane == (uint32_t)__builtin_ctzll(pend)) atomicAdd(&S.shist[k], (uint32_t)__popcll(same));
        pend &= ~same;
      }
    }
    // (a cluster that ran its election here changed flags, masks and terms too)
    const bool wfp = !__builtin_amdgcn_ballot_w64(wb && (!fp || el));
    if (wb) {
      // every word of fields DEADLINE..LEN, from registers (LEN unchanged): fx's, and beside them
      // the fields only this path holds
      constexpr int NV = HF_NEXT;
      uint32_t v[NV][N];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const bool isL = (uint32_t)k == L;
        fx.node_words(k, v);
        v[HF_FLAGS][k] = isL ? Lfl : (fx.at_node(ffl, k) & ~FL_DRAW) |
                                         (((fx.fpend >> fx.slot(k)) & 1) ? FL_DRAW : 0u);
        v[HF_MASKS][k] = isL ? Lmk : fx.at_node(fmk, k);
        v[HF_TERM][k] = isL ? Lterm : fx.at_node(fterm, k);
        v[HF_COMMIT][k] = isL ? Lcommit : fx.at_node(fcommit, k);
        v[HF_LEN][k] = isL ? Llen : fx.at_node(flen, k);
      }
      auto live = [](int q) { return q >= (int)HOT_CW && q < (int)(HOT_CW + HF_NEXT * N); };
      auto val = [&](int q) { return v[(q - HOT_CW) / N][(q - HOT_CW) % N]; };
      // The changed chunks into the image (in a heartbeat round the deadlines and trace hashes
      // change, all in the block's first line; flags, terms, masks, commits, queue words and rows
      // come back unchanged); the lines they dirty go back to memory whole, below.
      // A wave whose written-back clusters all took the fixed-point path changed nothing past the
      // queue words and the flags' FL_DRAW (masks, terms, commits, lengths and rows are the fixed
      // point's).
      const int ch_end = wfp ? (int)(HOT_CW + (HF_FLAGS + 1) * N + 3) / 4
                             : (int)(HOT_CW + HF_NEXT * N + 3) / 4;
      // (every chunk is written back to the image, changed or not: no branch per chunk)
#pragma unroll
      for (int i = (int)HOT_CW / 4; i < (int)(HOT_CW + HF_NEXT * N + 3) / 4; ++i) {
        if (i < ch_end) {                                    // wave-uniform
          const int q = 4 * i;
          const uint4 x = make_uint4(live(q) ? val(q) : w[q], live(q + 1) ? val(q + 1) : w[q + 1],
                                     live(q + 2) ? val(q + 2) : w[q + 2],
                                     live(q + 3) ? val(q + 3) : w[q + 3]);
          *lds_at<uint4>(img, img_off(lane, i)) = x;
          dl |= (uint32_t)(x.x != w[q] || x.y != w[q + 1] || x.z != w[q + 2] || x.w != w[q + 3])
                << (i / 8);
        }
      }
      if (el) {
        // the words the election changed are compared with the registers it wrote: its lines are
        // dirty; and the new leader's led term (P4), in the image or past it
        dl |= (1u << ((HOT_CW + HF_NEXT * N + 31) / 32)) - 1;
        const uint32_t q = HOT_CW + hf_led(N) * N + L;
        if (q < (uint32_t)IMGC * 4) {
          *lds_at<uint32_t>(img, img_off(lane, q / 4) + 4 * (q % 4)) = Lterm;
          dl |= 1u << (q / 32);
        } else {
          S.hot[(size_t)c * HB + q] = Lterm;
        }
      }
      // the steady certificate for the next launch: the cluster stays at its fixed point
      const uint32_t cn = fp || (full && at_fixed_point_state()) ? (CERT_MAGIC | L) : 0u;
      *lds_at<uint4>(img, img_off(lane, CL_CERT / 4)) = make_uint4(w[CL_CERT - 3], w[CL_CERT - 2], w[CL_CERT - 1], cn);
      dl |= (uint32_t)(cn != w[CL_CERT]);
      // the leader's rows (node L): next / match of peer fk(j) + 1
      if (!wfp) {
#pragma unroll
        for (int j = 0; j < F; ++j) {
          const uint32_t qn = HOT_CW + (HF_NEXT + fx.fk(j)) * N + L;
          const uint32_t qt = HOT_CW + (HF_NEXT + N + fx.fk(j)) * N + L;
          if (nx[j] != nx0[j]) {
            *lds_at<uint32_t>(img, img_off(lane, qn / 4) + 4 * (qn % 4)) = (uint32_t)nx[j];
            dl |= 1u << (qn / 32);
          }
          if (mt[j] != mt0[j]) {
            *lds_at<uint32_t>(img, img_off(lane, qt / 4) + 4 * (qt % 4)) = (uint32_t)mt[j];
            dl |= 1u << (qt / 32);
          }
        }
      }
    }
    fx.to_rings(S, c, wb);
    nhb = fx.nhb; nae = fx.nae; nar = fx.nar;
  }   // the general path
  // The tail (store_lines, add_counters above): every line of the image may be dirty here.
#ifdef RS_WAVELOG
  wl_sb = wall_clock64();
#endif
  store_lines<N, IMGC / 8>(S, img, cbase, lane, dl);
#ifdef RS_WAVELOG
  wave_record();
#endif
  add_counters<N>(S, lane, blockIdx.x * 4 + wave, nhb, nae, nar);
  // Elections run here add a timeout, F request-votes and F vote responses, a leader, and the
  // request-vote, vote-response and append-entries messages (3F; the responses are in nae).
  if (__builtin_amdgcn_ballot_w64(el)) {                   // wave-uniform
    // per election: el_to timeouts, F request-votes and F vote responses per timeout, one
    // leader, and the request-vote, vote-response and append-entries messages
    unsigned long long* const ctr = wave_counters(S, blockIdx.x * 4 + wave);
    const uint32_t ne = wave_sum(el ? 1u : 0u), nt = wave_sum(el_to);
    if (lane < 6) {
      const int idx = lane == 0 ? RAFT_CTR_EV_TIMEOUT : lane == 1 ? RAFT_CTR_EV_RV
                    : lane == 2 ? RAFT_CTR_EV_VR : lane == 3 ? RAFT_CTR_LEADERS
                    : lane == 4 ? RAFT_CTR_SENT : RAFT_CTR_DELIVERED;
      const uint32_t v = lane == 0 ? nt : lane == 3 ? ne : lane <= 2 ? (uint32_t)F * nt
                                                                 : (uint32_t)F * (2 * nt + ne);
      atomicAdd(&ctr[idx], (unsigned long long)v);
    }
  }
  // ---------------------------------------------------------------- catch-up
  // The wave's bailed clusters, each from the tick it stopped before to the launch's end, through
  // the general tick body, with the wave's image as its LDS block (the write-back above read the
  // image: a wave's LDS operations complete in order). The blocks it reads are this wave's own
  // stores: they are waited for first.
  if (nbw) {                                                  // wave-uniform
    if (lane == 0) atomicAdd(S.nbail, nbw);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    tick_wave<N, false, false, true, true>(S, t0, nt, reinterpret_cast<uint32_t*>(img), (int)lane,
                                           0, 1, blc, nbw, blt, blockIdx.x * 4 + wave);
  }
#ifdef RS_WAVELOG
  wave_done();
#endif
}

hipError_t configure_steady() {
  hipError_t e = hipSuccess;
#define RS_CFG(NN)                                                                         \
  if (e == hipSuccess)                                                                     \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(steady_lane_kernel<NN>),         \
                            hipFuncAttributeMaxDynamicSharedMemorySize,                    \
                            (int)steady_lds_bytes<NN>());
  RS_CFG(2) RS_CFG(3) RS_CFG(4) RS_CFG(5)
#undef RS_CFG
  return e;
}

// The steady kernel for N <= 5 (LITE launches; the caller checks): one thread per cluster, in id
// order. Its timestamps go into ev0/ev1 through its dispatch packet.
hipError_t launch_steady(const DevSim& S, uint32_t t0, uint32_t nt, hipStream_t st,
                         hipEvent_t ev0, hipEvent_t ev1) {
  if (S.perm) return hipErrorInvalidValue;                     // clusters in id order only
  const dim3 grid((S.C + LANE_WG - 1) / LANE_WG);
  switch (S.N) {
#define RS_LANE(NN)                                                                             \
  case NN:                                                                                      \
    hipExtLaunchKernelGGL((steady_lane_kernel<NN>), grid, dim3(LANE_WG), steady_lds_bytes<NN>(), \
                          st, ev0, ev1, 0, S, t0, nt);                                          \
    break;
    RS_LANE(2) RS_LANE(3) RS_LANE(4) RS_LANE(5)
#undef RS_LANE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace rs
