// fixed_point_affine.hpp — K whole heartbeat rounds of a cluster at its fixed point as one affine
// step of each trace hash. Plain C++17: no HIP header, so a CPU program checks it exhaustively
// (tests/test_fixed_point_affine.py); steady_kernel.hip ties its constants to device.hpp's.
//
// The trace hash (SIM_SPEC §4) takes h to h * M^2 + (x0 * M + x1) per event, with
// x0 = t + hdr * 2^32 (every tick is below 2^32), hdr = ev | src << 3 | role << 7 and
// x1 = msg_term + term * 2^32: linear mod 2^64 in t, in hdr and in the term T.
//
// Leader. The round with its heartbeat at tick tau has F + 1 leader events, all of role LEADER and
// term T: the heartbeat (ev 7, src 0, msg_term 0) at tau, then response j = 0 .. F-1 (src =
// j + 1 + (j >= L), msg_term T) at tau + 2d + j. Event e of the round is weighted by M2^(F - e), so
// the round takes h to h * A + alpha(tau) with A = M2^(F+1) and
//   alpha(tau) = tau * x1 + T * y1 + z1 + 2^32 * lo32(w[L])        (mod 2^64)
//   x1 = M * geo(F+1)                                  geo(n) = 1 + M2 + ... + M2^(n-1)
//   y1 = 2^32 * M2^F + (1 + 2^32) * geo(F)
//   z1 = M * (2d * geo(F) + sum_j j * M2^(F-1-j)) + 2^32 * lo32(M * H),
//        H = hdr_hb * M2^F + sum_j (hdr_ar + 8 (j + 1)) * M2^(F-1-j)
//   w[L] = 8 * M * sum_{j >= L} M2^(F-1-j)             (the (j >= L) bit of the sender ids)
// Follower. One event per round, the append-entries (src L + 1, msg_term T, role FOLLWER, term T)
// at tau + d: A = M2, x1 = M, y1 = 1 + 2^32, z1 = d * M + 2^32 * lo32(M * (hdr_ae + 8)),
// w[L] = 8 * M * L. Only h differs between the followers of a cluster.
//
// K rounds, P ticks apart, from the heartbeat at th: a map of the same form,
//   h -> h * a + th * x + T * y + z + 2^32 * lo32(w[L] * s)
// (a Half below). Two such maps compose into a third (compose_half: the second one's rounds start
// K_first * P ticks later), so the map of K rounds is built from the one-round map in O(log K)
// compositions by doubling, and the map of K + 1 rounds from K's in one. The coefficients depend
// on (F, d, hb, K) alone: wave-uniform in a launch, where K takes two adjacent values.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FPA_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define FPA_FN inline
#endif

namespace rs {
namespace fpa {

constexpr uint64_t M = 0x9E3779B97F4A7C15ull;        // device.hpp's TRACE_M
constexpr uint64_t M2 = M * M;
constexpr uint32_t EV_HEARTBEAT = 7, EV_APPEND_ENTRIES = 2, EV_APPEND_RESPONSE = 5;
constexpr uint32_t ROLE_LEADER = 2, ROLE_FOLLWER = 3;
constexpr uint32_t HDR_HB = EV_HEARTBEAT | ROLE_LEADER << 7;
constexpr uint32_t HDR_AR = EV_APPEND_RESPONSE | ROLE_LEADER << 7;   // + 8 * sender id
constexpr uint32_t HDR_AE = EV_APPEND_ENTRIES | ROLE_FOLLWER << 7;   // + 8 * leader id

constexpr uint64_t pow_m2(int n) {
  uint64_t x = 1;
  for (int i = 0; i < n; ++i) x *= M2;
  return x;
}
constexpr uint64_t geo_m2(int n) {
  uint64_t s = 0, x = 1;
  for (int i = 0; i < n; ++i) {
    s += x;
    x *= M2;
  }
  return s;
}

// One hash's map over a run of whole rounds (above).
struct Half {
  uint64_t a, x, y, z;
  uint32_t s;
};
// The maps of K rounds: the leader's hash and a follower's.
struct Set {
  uint32_t K;
  Half lead, fol;
};

// The compile-time parts of the one-round maps of an (F + 1)-node cluster.
template <int F>
struct Round {
  static constexpr uint64_t lead_a = pow_m2(F + 1);
  static constexpr uint64_t lead_x = M * geo_m2(F + 1);
  static constexpr uint64_t lead_y = (pow_m2(F) << 32) + geo_m2(F) + (geo_m2(F) << 32);
  static constexpr uint64_t lead_jsum() {              // sum_j j * M2^(F-1-j)
    uint64_t s = 0;
    for (int j = 0; j < F; ++j) s += (uint64_t)j * pow_m2(F - 1 - j);
    return s;
  }
  static constexpr uint32_t lead_hdr() {               // lo32(M * H)
    uint64_t h = HDR_HB * pow_m2(F);
    for (int j = 0; j < F; ++j) h += (uint64_t)(HDR_AR + 8 * (j + 1)) * pow_m2(F - 1 - j);
    return (uint32_t)(M * h);
  }
  static constexpr uint32_t lead_w(int L) {            // lo32(8 M * sum_{j >= L} M2^(F-1-j))
    uint64_t s = 0;
    for (int j = L; j < F; ++j) s += pow_m2(F - 1 - j);
    return (uint32_t)(8 * M * s);
  }
  static constexpr uint32_t fol_hdr = (uint32_t)(M * (HDR_AE + 8));
  static constexpr uint32_t fol_w(int L) { return (uint32_t)(8 * M * (uint64_t)L); }
};

template <int F>
FPA_FN Set one_round(uint32_t d) {
  using R = Round<F>;
  Set c;
  c.K = 1;
  c.lead.a = R::lead_a;
  c.lead.x = R::lead_x;
  c.lead.y = R::lead_y;
  c.lead.z = M * (2 * (uint64_t)d * geo_m2(F) + R::lead_jsum()) + ((uint64_t)R::lead_hdr() << 32);
  c.lead.s = 1;
  c.fol.a = M2;
  c.fol.x = M;
  c.fol.y = 1 + (1ull << 32);
  c.fol.z = (uint64_t)d * M + ((uint64_t)R::fol_hdr << 32);
  c.fol.s = 1;
  return c;
}

// The map "f's rounds, then g's": g's first heartbeat is kp = K_f * P ticks after f's.
FPA_FN Half compose_half(const Half& f, const Half& g, uint64_t kp) {
  Half r;
  r.a = f.a * g.a;
  r.x = g.a * f.x + g.x;
  r.y = g.a * f.y + g.y;
  r.z = g.a * f.z + g.z + kp * g.x;
  r.s = (uint32_t)g.a * f.s + g.s;
  return r;
}
FPA_FN Set compose(const Set& f, const Set& g, uint32_t P) {
  const uint64_t kp = (uint64_t)f.K * P;
  Set r;
  r.K = f.K + g.K;
  r.lead = compose_half(f.lead, g.lead, kp);
  r.fol = compose_half(f.fol, g.fol, kp);
  return r;
}

FPA_FN uint32_t period(int F, uint32_t d, uint32_t hb) { return 2 * d + (uint32_t)F - 1 + hb; }

// The band of a launch of nt ticks from t0. A cluster on the schedule has its first heartbeat of
// the launch at th = t0 + delta with 0 <= delta < P, and runs
//   K(delta) = tend > th + last ? (tend - th - last - 1) / P + 1 : 0      (last = 2d + F - 1)
// whole rounds before tend = t0 + nt. With R = nt - last - 1 = (K1 - 1) P + rho, 0 <= rho < P:
// delta <= rho leaves (R - delta) / P = K1 - 1, so K = K1; rho < delta < P leaves
// R - delta = (K1 - 2) P + (P + rho - delta) with 0 < P + rho - delta < P, so K = K1 - 1 (at
// K1 = 1: R = rho < delta, tend <= th + last, K = 0). Hence K(delta) = K1 - (delta > rho): one
// comparison per cluster against launch constants, no division. nt <= last: K = K1 = 0 for every
// delta, and rho is a value no delta exceeds. The K rounds end at tk = th + K P, with
// K1P = K1 * P and K1P - P both launch constants.
struct Band {
  uint32_t K1, rho, K1P;
};
FPA_FN Band band(int F, uint32_t d, uint32_t hb, uint32_t nt) {
  const uint32_t P = period(F, d, hb), last = 2 * d + (uint32_t)F - 1;
  Band b;
  if (nt > last) {
    const uint32_t R = nt - last - 1, q = R / P;
    b.K1 = q + 1;
    b.rho = R - q * P;
    b.K1P = b.K1 * P;
  } else {
    b.K1 = 0;
    b.rho = 0xFFFFFFFFu;
    b.K1P = 0;
  }
  return b;
}
// The whole rounds of the cluster at delta, and the ticks they take.
FPA_FN uint32_t band_rounds(const Band& b, uint32_t delta) { return b.K1 - (uint32_t)(delta > b.rho); }
FPA_FN uint32_t band_ticks(const Band& b, uint32_t P, uint32_t delta) {
  return b.K1P - (delta > b.rho ? P : 0u);
}

// K's set from (K - 1)'s.
template <int F>
FPA_FN Set step(const Set& c, uint32_t d, uint32_t hb) {
  return compose(c, one_round<F>(d), period(F, d, hb));
}

// The set of K rounds, by doubling from K's top bit down. K = 0: the identity.
template <int F>
FPA_FN Set build(uint32_t d, uint32_t hb, uint32_t K) {
  const uint32_t P = period(F, d, hb);
  Set r;
  r.K = 0;
  r.lead.a = r.fol.a = 1;
  r.lead.x = r.lead.y = r.lead.z = r.fol.x = r.fol.y = r.fol.z = 0;
  r.lead.s = r.fol.s = 0;
  if (!K) return r;
  r = one_round<F>(d);
  for (int b = 30 - __builtin_clz(K); b >= 0; --b) {
    r = compose(r, r, P);
    if ((K >> b) & 1) r = step<F>(r, d, hb);
  }
  return r;
}

FPA_FN uint64_t apply_half(const Half& c, uint64_t h, uint32_t th, uint32_t T, uint32_t w) {
  return h * c.a + (uint64_t)th * c.x + (uint64_t)T * c.y + c.z + ((uint64_t)(w * c.s) << 32);
}
// What a cluster's leader index adds to the headers of its events, by masks: an indexed table
// would be a load per lane.
template <int F>
FPA_FN uint32_t lead_w(uint32_t L) {
  uint32_t w = 0;
  if (F >= 1) w |= Round<F>::lead_w(0) & (0u - (uint32_t)(L == 0u));
  if (F >= 2) w |= Round<F>::lead_w(1) & (0u - (uint32_t)(L == 1u));
  if (F >= 3) w |= Round<F>::lead_w(2) & (0u - (uint32_t)(L == 2u));
  if (F >= 4) w |= Round<F>::lead_w(3) & (0u - (uint32_t)(L == 3u));
  static_assert(F >= 1 && F <= 4 && Round<F>::lead_w(F) == 0, "the leader index is 0 .. F");
  return w;
}
template <int F>
FPA_FN uint32_t fol_w(uint32_t L) {
  uint32_t w = 0;
  if (F >= 1) w |= Round<F>::fol_w(1) & (0u - (uint32_t)(L == 1u));
  if (F >= 2) w |= Round<F>::fol_w(2) & (0u - (uint32_t)(L == 2u));
  if (F >= 3) w |= Round<F>::fol_w(3) & (0u - (uint32_t)(L == 3u));
  if (F >= 4) w |= Round<F>::fol_w(4) & (0u - (uint32_t)(L == 4u));
  static_assert(Round<F>::fol_w(0) == 0, "leader index 0 adds nothing");
  return w;
}

// The leader's hash after the lead map's rounds from the heartbeat at th (term T, leader index L).
template <int F>
FPA_FN uint64_t apply_leader(const Half& lead, uint64_t h, uint32_t th, uint32_t T, uint32_t L) {
  return apply_half(lead, h, th, T, lead_w<F>(L));
}
// What the fol map adds to every follower's hash: h -> h * fol.a + follower_addend(...).
template <int F>
FPA_FN uint64_t follower_addend(const Half& fol, uint32_t th, uint32_t T, uint32_t L) {
  return apply_half(fol, 0, th, T, fol_w<F>(L));
}
template <int F>
FPA_FN uint64_t apply_follower(const Half& fol, uint64_t h, uint32_t th, uint32_t T, uint32_t L) {
  return h * fol.a + follower_addend<F>(fol, th, T, L);
}

}  // namespace fpa
}  // namespace rs
