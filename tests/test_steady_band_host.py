"""The launch band of csrc/fixed_point_affine.hpp (Band, band(), band_rounds(), band_ticks())
against the division the steady kernel's general rounds() makes per cluster, on the CPU.

A cluster on the fixed point's schedule has its first heartbeat of a launch at th = t0 + delta,
0 <= delta < P. rounds() counts its whole rounds as
    K = tend > th + last ? (tend - th - last - 1) / P + 1 : 0,   tk = th + K * P
(tend = t0 + nt, last = 2d + F - 1, P = 2d + F - 1 + hb). The line-0 body takes K from one
comparison against the launch's band instead: K = K1 - (delta > rho), tk = th + K1 * P - (delta >
rho ? P : 0). A stand-alone C++ program (its own main, the header alone) is compiled with g++ --
under UBSan where the machine has its runtime -- and compares the two for F = 1..4, d = 1..3,
hb from 2d + F to 2d + F + 40 and 3000, every nt in 0 .. 4P + last + 2 plus 10,000 and 65,536, and
every delta in [0, P)."""
import hostprog

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include "fixed_point_affine.hpp"

static long long checks = 0, bad = 0;

static void one(int F, uint32_t d, uint32_t hb, uint32_t nt, uint32_t t0) {
  using namespace rs::fpa;
  const uint32_t P = period(F, d, hb), last = 2 * d + (uint32_t)F - 1, tend = t0 + nt;
  const Band b = band(F, d, hb, nt);
  // what band_sets() builds its two sets from: K1 = K(th = t0)
  const uint32_t K1 = nt > last ? (nt - last - 1) / P + 1 : 0;
  bool ok = b.K1 == K1 && b.K1P == K1 * P && (K1 == 0 || b.rho < P);
  for (uint32_t delta = 0; delta < P; ++delta) {
    const uint32_t th = t0 + delta;
    // today's rounds(), the general form
    const uint32_t K = tend > th + last ? (tend - th - last - 1) / P + 1 : 0;
    const uint32_t tk = th + K * P;
    const uint32_t Kb = band_rounds(b, delta), tkb = th + band_ticks(b, P, delta);
    ok = ok && Kb == K && tkb == tk && (Kb == b.K1 || Kb + 1 == b.K1);
    ++checks;
  }
  if (!ok && bad++ < 20)
    printf("MISMATCH F=%d d=%u hb=%u nt=%u t0=%u (K1 %u rho %u K1P %u)\n", F, d, hb, nt, t0, b.K1,
           b.rho, b.K1P);
}

int main() {
  for (int F = 1; F <= 4; ++F)
    for (uint32_t d = 1; d <= 3; ++d)
      for (uint32_t i = 0; i <= 41; ++i) {
        const uint32_t hb = i <= 40 ? 2 * d + (uint32_t)F + i : 3000;
        const uint32_t P = rs::fpa::period(F, d, hb), last = 2 * d + (uint32_t)F - 1;
        const uint32_t t0 = 1000003u * (uint32_t)F + 7u * d + i;
        for (uint32_t nt = 0; nt <= 4 * P + last + 2; ++nt) one(F, d, hb, nt, t0);
        one(F, d, hb, 10000, t0);
        one(F, d, hb, 65536, t0);
        one(F, d, hb, 10000, 0);
        one(F, d, hb, 65536, 0);
      }
  printf("checks %lld bad %lld\n", checks, bad);
  return bad ? 1 : 0;
}
"""


def test_band_equals_division(tmp_path):
    out = hostprog.run_cpp(tmp_path, "band_check", PROGRAM, opt="-O2")
    assert hostprog.checks(out) > 100_000_000
