"""csrc/summary_host.hpp on the CPU: the scratch layout of the census's and the audit's queries, and
the algebra that folds their summaries.

A stand-alone C++ program (its own main, the header and include/raftsim.h alone) is compiled with
g++ -- under UBSan where the machine has its runtime -- and run once.

Layout, for C in {1, 2, 3, 4, 5, 3001, 8191, 8192, 8193, 8197, 32767, 32768, 32769, 32789, 115138,
1048576}, the census at N = 2..9 and the audit at both group widths: the partial records [0, grid)
of either width's grid, the folded record and the compaction's chunks + 1 counts are pairwise
disjoint and lie inside the words the layout says to allocate; total_ptr is the last count; the
chunks cover C clusters. 3001 and 8197 are there for the fault of the pull request that added the
audit: its scratch was sized by the narrow width's grid and written by the wide one's, an illegal
memory access on the GPU at 3,001 clusters. With aud_parts put back to the narrow grid this check
fails at both sizes.

Algebra, for every u64 field of raft_census_t and raft_audit_t: the header's op is the one the
field's name demands (the minima and maxima are written out below, everything else is a sum); unit
is the identity of fold; fold is commutative and associative on random triples; summary_init and
k summary_combine's give the field-wise fold computed directly, the structs written and read
through their member names in raftsim/_abi.py's order."""
import ctypes

import hostprog
from raftsim import _abi

MINIMA = {"census": ("term_min",),
          "audit": ("agree_min", "diverge_index_min", "commit_diverge_index_min")}
MAXIMA = {"census": ("term_max", "commit_max", "len_max", "hwm_max"), "audit": ("agree_max",)}

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "summary_host.hpp"

using namespace rs;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {                      // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// every magnitude, and the two ends
static uint64_t value() {
  const uint64_t k = rnd() % 16;
  return k == 0 ? 0 : k == 1 ? ~0ull : rnd() >> (rnd() % 64);
}

static long checks = 0, bad = 0;
static void expect(bool ok, const char* what, const char* who, long a, long b) {
  ++checks;
  if (!ok && bad++ < 20) printf("MISMATCH %s (%s) at %ld, %ld\n", what, who, a, b);
}

// ---- layout -------------------------------------------------------------------------------------
struct Region {
  size_t lo, hi;                             // in u32 words of the scratch array
};
static void check_layout(const SummaryLayout& lay, uint32_t grid_a, uint32_t grid_b,
                         const char* who, uint32_t C, uint32_t v) {
  std::vector<unsigned long long> scratch(lay.words());
  const uint32_t* const base = reinterpret_cast<const uint32_t*>(scratch.data());
  std::vector<Region> r;
  for (uint32_t p = 0; p < std::max(grid_a, grid_b); ++p)
    r.push_back({2 * lay.part(p), 2 * (lay.part(p) + lay.F)});
  r.push_back({2 * lay.result(), 2 * (lay.result() + lay.F)});
  const uint32_t* const cnt = lay.counts_ptr(scratch.data());
  r.push_back({(size_t)(cnt - base), (size_t)(cnt - base) + lay.chunks + 1});
  expect(lay.total_ptr(scratch.data()) == cnt + lay.chunks, "total is the last count", who, C, v);
  expect(grid_a >= 1 && grid_b >= 1 && lay.F >= 1, "nothing to lay out", who, C, v);
  std::sort(r.begin(), r.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
  for (size_t i = 0; i < r.size(); ++i) {
    expect(r[i].lo < r[i].hi, "empty region", who, C, v);
    expect(r[i].hi <= (i + 1 < r.size() ? r[i + 1].lo : 2 * lay.words()),
           "regions overlap or leave the array", who, C, v);
  }
}

static void layouts() {
  static const uint32_t Cs[] = {1, 2, 3, 4, 5, 3001, 8191, 8192, 8193, 8197, 32767, 32768, 32769,
                                32789, 115138, 1048576};
  for (uint32_t C : Cs) {
    for (uint32_t N = 2; N <= 9; ++N) {
      const SummaryLayout lay = census_layout(C, N);
      check_layout(lay, cen_grid(C, N), cen_grid(C, N), "census", C, N);
      expect(lay.F * 8 == sizeof(raft_census_t), "F", "census", C, N);
      // a chunk: four waves, sixteen rounds, floor(64 / N) clusters a wave
      expect((uint64_t)lay.chunks * (4 * 16 * (64 / N)) >= C, "chunks cover", "census", C, N);
    }
    const SummaryLayout lay = audit_layout(C);
    check_layout(lay, aud_grid(C, 16), aud_grid(C, 64), "audit", C, 0);
    expect(lay.F * 8 == sizeof(raft_audit_t), "F", "audit", C, 0);
    // a chunk: four records for each of 256 lanes
    expect((uint64_t)lay.chunks * 1024 >= C, "chunks cover", "audit", C, 0);
    // a group: 64 / width clusters; four waves a workgroup; at most 2,048 workgroups
    for (uint32_t G : {16u, 64u}) {
      const uint64_t groups = ((uint64_t)C + 64 / G - 1) / (64 / G);
      expect(aud_grid(C, G) == std::min<uint64_t>((groups + 3) / 4, 2048), "grid", "audit", C, G);
    }
  }
}

// ---- algebra ------------------------------------------------------------------------------------
struct Field {
  const char* name;
  uint32_t n;                                // u64 words
  int op;                                    // 0 sum, 1 minimum, 2 maximum: from the name
};
static uint64_t direct(int op, uint64_t a, uint64_t b) {
  return op == 1 ? std::min(a, b) : op == 2 ? std::max(a, b) : a + b;
}

@TABLES@

template <class T>
static void algebra(const char* who, const Field* fields, size_t nf,
                    void (*put)(T&, const uint64_t*), void (*get)(const T&, uint64_t*)) {
  constexpr uint32_t F = summary_F<T>;
  std::vector<int> op;
  for (size_t i = 0; i < nf; ++i) op.insert(op.end(), fields[i].n, fields[i].op);
  expect(op.size() == F && F * 8 == sizeof(T), "field list", who, (long)op.size(), F);
  if (op.size() != F) return;
  for (uint32_t f = 0; f < F; ++f) {
    expect(summary_fields<T>::op(f) == op[f], "op of field", who, f, op[f]);
    const uint64_t u = summary_unit<T>(f);
    for (int rep = 0; rep < 300; ++rep) {
      const uint64_t a = value(), b = value(), c = value();
      expect(summary_fold<T>(f, u, a) == a && summary_fold<T>(f, a, u) == a, "unit", who, f, rep);
      expect(summary_fold<T>(f, a, b) == summary_fold<T>(f, b, a), "commutative", who, f, rep);
      expect(summary_fold<T>(f, summary_fold<T>(f, a, b), c) ==
                 summary_fold<T>(f, a, summary_fold<T>(f, b, c)), "associative", who, f, rep);
      expect(summary_fold<T>(f, a, b) == direct(op[f], a, b), "fold", who, f, rep);
    }
  }
  for (uint32_t k : {0u, 1u, 2u, 3u, 8u, 100u}) {
    T acc;
    memset(&acc, 0xAB, sizeof acc);
    summary_init(&acc);
    uint64_t want[F], in[F], got[F];
    for (uint32_t f = 0; f < F; ++f) want[f] = op[f] == 1 ? ~0ull : 0ull;
    for (uint32_t i = 0; i < k; ++i) {
      T x;
      for (uint32_t f = 0; f < F; ++f) {
        in[f] = value();
        want[f] = direct(op[f], want[f], in[f]);
      }
      put(x, in);
      summary_combine(&acc, &x);
    }
    get(acc, got);
    for (uint32_t f = 0; f < F; ++f) expect(got[f] == want[f], "init + combine", who, k, f);
  }
}

int main() {
  layouts();
  algebra<raft_census_t>("census", census_fields, sizeof census_fields / sizeof *census_fields,
                         put_census, get_census);
  algebra<raft_audit_t>("audit", audit_fields, sizeof audit_fields / sizeof *audit_fields,
                        put_audit, get_audit);
  printf("checks %ld bad %ld\n", checks, bad);
  return bad ? 1 : 0;
}
"""


def tables(who, struct):
    """The C++ field table of an _abi structure, and its put / get through the member names."""
    fields = [(f, 1 if t is ctypes.c_uint64 else ctypes.sizeof(t) // 8) for f, t in struct._fields_]
    names = [f for f, _ in fields]
    assert set(MINIMA[who]) | set(MAXIMA[who]) <= set(names)
    rows = ", ".join('{"%s", %d, %d}' % (f, n, 1 if f in MINIMA[who] else 2 if f in MAXIMA[who] else 0)
                     for f, n in fields)
    put, get, i = [], [], 0
    for f, n in fields:
        for j in range(n):
            member = f if n == 1 and dict(struct._fields_)[f] is ctypes.c_uint64 else f"{f}[{j}]"
            put.append(f"  s.{member} = v[{i}];")
            get.append(f"  v[{i}] = s.{member};")
            i += 1
    return "\n".join([f"static const Field {who}_fields[] = {{{rows}}};",
                      f"static void put_{who}(raft_{who}_t& s, const uint64_t* v) {{", *put, "}",
                      f"static void get_{who}(const raft_{who}_t& s, uint64_t* v) {{", *get, "}"])


def test_layout_regions_are_disjoint_and_the_algebra_folds_by_name(tmp_path):
    program = PROGRAM.replace("@TABLES@", tables("census", _abi.Census) + "\n" +
                              tables("audit", _abi.Audit))
    assert hostprog.checks(hostprog.run_cpp(tmp_path, "summary_check", program)) > 100000
