"""csrc/fixed_point_affine.hpp against the trace hash run event by event (SIM_SPEC §4), on the CPU.

A stand-alone C++ program (its own main, the header alone) is compiled with g++ -- under UBSan
where the machine has its runtime -- and run once. For every F = 1..4, d in {1, 2, 3},
hb in {2d + F, 2d + F + 2, 3000}, leader index L = 0..F and K in {1, 2, 3, 4, 5, 17, 1000, 7001}
it checks, for random hashes h, terms T and first heartbeats th:
  * the leader's hash and each follower's after build + apply equal the hashes after the K rounds'
    events, one at a time, as the spec states the hash (not as device.hpp restates it);
  * the set of K + 1 rounds made from K's by one step equals the set built directly.
Ticks: every event tick of a simulation is below 2^32 (the kernels' horizon check), so th is drawn
such that the last round's last event is; half of the draws end within 10^5 ticks of 2^32 - 1."""
import hostprog

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "fixed_point_affine.hpp"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {                      // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// SIM_SPEC §4: h <- (h * M + x0) * M + x1, x0 = t | (ev | src << 3 | role << 7 | fault << 9) << 32,
// x1 = msg_term | current_term << 32
static const uint64_t SPEC_M = 0x9E3779B97F4A7C15ull;
static uint64_t event(uint64_t h, uint32_t t, uint32_t ev, uint32_t src, uint32_t mterm,
                      uint32_t role, uint32_t term) {
  const uint64_t x0 = (uint64_t)t | (uint64_t)(ev | src << 3 | role << 7) << 32;
  const uint64_t x1 = (uint64_t)mterm | (uint64_t)term << 32;
  return (h * SPEC_M + x0) * SPEC_M + x1;
}

static long checks = 0, bad = 0;
static void expect(bool ok, const char* what, int F, uint32_t d, uint32_t hb, uint32_t L,
                   uint32_t K) {
  ++checks;
  if (!ok && bad++ < 20) printf("MISMATCH %s F=%d d=%u hb=%u L=%u K=%u\n", what, F, d, hb, L, K);
}
static bool same_half(const rs::fpa::Half& p, const rs::fpa::Half& q) {
  return p.a == q.a && p.x == q.x && p.y == q.y && p.z == q.z && p.s == q.s;
}

template <int F>
static void run() {
  using namespace rs::fpa;
  static const uint32_t Ks[] = {1, 2, 3, 4, 5, 17, 1000, 7001};
  for (uint32_t d = 1; d <= 3; ++d) {
    const uint32_t hbs[] = {2 * d + F, 2 * d + F + 2, 3000};
    for (uint32_t hb : hbs) {
      const uint32_t P = 2 * d + F - 1 + hb;
      for (uint32_t K : Ks) {
        const Set c = build<F>(d, hb, K);
        const Set c1 = build<F>(d, hb, K + 1), s1 = step<F>(c, d, hb);
        expect(c.K == K && s1.K == K + 1 && c1.K == K + 1, "K", F, d, hb, 0, K);
        expect(same_half(c1.lead, s1.lead), "step lead", F, d, hb, 0, K);
        expect(same_half(c1.fol, s1.fol), "step fol", F, d, hb, 0, K);
        // the last event of the K rounds is at th + (K - 1) P + 2d + F - 1 <= 2^32 - 1
        const uint64_t span = (uint64_t)(K - 1) * P + 2 * d + F - 1;
        const uint64_t th_max = 0xFFFFFFFFull - span;
        for (uint32_t L = 0; L <= (uint32_t)F; ++L) {
          for (int rep = 0; rep < 4; ++rep) {
            const uint32_t th = (uint32_t)(rep & 1 ? th_max - rnd() % 100000 : rnd() % (th_max + 1));
            const uint32_t T = rep == 3 ? 0xFFFFFFFFu : (uint32_t)rnd() >> (rnd() % 32);
            uint64_t hl = rnd(), hf[F], gl = hl, gf[F];
            for (int j = 0; j < F; ++j) gf[j] = hf[j] = rnd();
            for (uint32_t r = 0; r < K; ++r) {
              const uint32_t tau = th + r * P;
              gl = event(gl, tau, 7, 0, 0, 2, T);
              for (int j = 0; j < F; ++j) {
                const uint32_t node = (uint32_t)j + ((uint32_t)j >= L ? 1u : 0u);   // 0-based
                gl = event(gl, tau + 2 * d + j, 5, node + 1, T, 2, T);
                gf[j] = event(gf[j], tau + d, 2, L + 1, T, 3, T);
              }
            }
            expect(apply_leader<F>(c.lead, hl, th, T, L) == gl, "leader", F, d, hb, L, K);
            const uint64_t add = follower_addend<F>(c.fol, th, T, L);
            for (int j = 0; j < F; ++j) {
              expect(hf[j] * c.fol.a + add == gf[j], "follower", F, d, hb, L, K);
              expect(apply_follower<F>(c.fol, hf[j], th, T, L) == gf[j], "follower", F, d, hb, L, K);
            }
          }
        }
      }
    }
  }
  const rs::fpa::Set id = rs::fpa::build<F>(2, 9, 0);
  expect(rs::fpa::apply_leader<F>(id.lead, 77, 5, 3, 0) == 77 &&
             rs::fpa::apply_follower<F>(id.fol, 78, 5, 3, F) == 78, "identity", F, 2, 9, 0, 0);
}

int main() {
  run<1>();
  run<2>();
  run<3>();
  run<4>();
  printf("checks %ld bad %ld\n", checks, bad);
  return bad ? 1 : 0;
}
"""


def test_affine_step_equals_events(tmp_path):
    assert hostprog.checks(hostprog.run_cpp(tmp_path, "fpa_check", PROGRAM)) > 20000
