// summary_host.hpp — what the summarising queries (state census, log audit) share that plain C++
// can state: how the u64 fields of a summary struct combine, the grids of the two passes, and
// where a shard's scratch array holds what. Compiles under hipcc (host and device) and under plain
// g++ with include/raftsim.h alone: tests/test_summary_host.py holds it to the structs' field lists
// and checks that no two regions of a scratch array overlap. The device side is summary.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/raftsim.h"

#if defined(__HIPCC__)
#define SUM_FN __host__ __device__ inline
#else
#define SUM_FN inline
#endif

namespace rs {

constexpr uint32_t SUMMARY_BLOCK = 256;              // four waves: both passes' workgroup
constexpr uint32_t SUMMARY_WAVES = SUMMARY_BLOCK / 64;

// ---- The field algebra. A summary T (raft_census_t, raft_audit_t) is summary_F<T> u64 fields,
// each an integer sum, minimum or maximum. summary_fields<T>::op(f) says which for field f: 0 sum,
// 1 minimum, 2 maximum.
template <class T> struct summary_fields;
template <class T> constexpr uint32_t summary_F = sizeof(T) / 8;

#define SUMMARY_IDX(T, field) ((uint32_t)(offsetof(T, field) / 8))
template <> struct summary_fields<raft_census_t> {
  static SUM_FN constexpr int op(uint32_t f) {
#define IS(field) (f == SUMMARY_IDX(raft_census_t, field))
    if (IS(term_min)) return 1;
    if (IS(term_max) || IS(commit_max) || IS(len_max) || IS(hwm_max)) return 2;
    return 0;
#undef IS
  }
};
template <> struct summary_fields<raft_audit_t> {
  static SUM_FN constexpr int op(uint32_t f) {
#define IS(field) (f == SUMMARY_IDX(raft_audit_t, field))
    if (IS(agree_min) || IS(diverge_index_min) || IS(commit_diverge_index_min)) return 1;
    return IS(agree_max) ? 2 : 0;
#undef IS
  }
};
#undef SUMMARY_IDX

template <class T> SUM_FN uint64_t summary_unit(uint32_t f) {
  return summary_fields<T>::op(f) == 1 ? ~0ull : 0ull;
}
template <class T> SUM_FN uint64_t summary_fold(uint32_t f, uint64_t a, uint64_t b) {
  static_assert(sizeof(T) % 8 == 0 && summary_F<T> <= 64, "a summary is at most 64 u64 fields");
  const int op = summary_fields<T>::op(f);
  return op == 0 ? a + b : op == 1 ? (a < b ? a : b) : (a > b ? a : b);
}
// Fields 0 .. n are sums: a pass may hold them as 32-bit counts (summary.hpp).
template <class T> constexpr bool summary_sums(uint32_t n) {
  for (uint32_t f = 0; f < n; ++f)
    if (summary_fields<T>::op(f) != 0) return false;
  return true;
}
// acc <- acc folded with x, field by field (the host's reduction over shards).
template <class T> SUM_FN void summary_init(T* acc) {
  uint64_t* a = reinterpret_cast<uint64_t*>(acc);
  for (uint32_t f = 0; f < summary_F<T>; ++f) a[f] = summary_unit<T>(f);
}
template <class T> SUM_FN void summary_combine(T* acc, const T* x) {
  uint64_t* a = reinterpret_cast<uint64_t*>(acc);
  const uint64_t* b = reinterpret_cast<const uint64_t*>(x);
  for (uint32_t f = 0; f < summary_F<T>; ++f) a[f] = summary_fold<T>(f, a[f], b[f]);
}

// ---- The scratch array of a shard's queries, in u64 words: `parts` partial records of F fields
// (a pass's workgroup b writes partial b), the folded record, then (as u32) the chunks + 1 counts
// of the selection's compaction (compact.hpp: a count per chunk, then the total). Whoever sizes the
// array and whoever writes it ask the same struct; a pass may use fewer partials than `parts`,
// never more (summary.hpp's launch_summary refuses it).
struct SummaryLayout {
  uint32_t parts, F, chunks;
  SUM_FN size_t part(uint32_t p) const { return (size_t)p * F; }
  SUM_FN size_t result() const { return part(parts); }
  SUM_FN size_t counts() const { return part(parts) + F; }
  SUM_FN size_t words() const { return counts() + ((size_t)chunks + 2) / 2; }
  SUM_FN uint32_t* counts_ptr(unsigned long long* scratch) const {
    return reinterpret_cast<uint32_t*>(scratch + counts());
  }
  SUM_FN const uint32_t* total_ptr(unsigned long long* scratch) const {
    return counts_ptr(scratch) + chunks;
  }
};

// ---- The census (census_kernel.hip): wave-sized groups of CPW = floor(64 / N) clusters; the pass
// strides over them on a capped grid; the selection's chunks are CEN_ROUNDS groups per wave.
constexpr uint32_t CEN_MAX_GRID = 1024;              // census workgroups (= partial records) at most
constexpr uint32_t CEN_ROUNDS = 16;                  // selection: wave-groups per wave and chunk
SUM_FN uint32_t cen_groups(uint32_t C, uint32_t N) {
  const uint32_t CPW = 64 / N;
  return (C + CPW - 1) / CPW;
}
SUM_FN uint32_t cen_grid(uint32_t C, uint32_t N) {
  const uint32_t wg = (cen_groups(C, N) + SUMMARY_WAVES - 1) / SUMMARY_WAVES;
  return wg < CEN_MAX_GRID ? wg : CEN_MAX_GRID;
}
SUM_FN uint32_t cen_chunks(uint32_t C, uint32_t N) {
  const uint32_t cc = SUMMARY_WAVES * CEN_ROUNDS * (64 / N);
  return (C + cc - 1) / cc;
}
SUM_FN SummaryLayout census_layout(uint32_t C, uint32_t N) {
  return {cen_grid(C, N), summary_F<raft_census_t>, cen_chunks(C, N)};
}

// ---- The audit (audit_kernel.hip): groups of 64 / G clusters, G the pass's lanes per cluster; the
// selection's chunks are AUD_ROUNDS records per lane.
constexpr uint32_t AUD_MAX_GRID = 2048;              // workgroups (= partial summaries) at most
constexpr uint32_t AUD_NARROW = 16, AUD_WIDE = 64;   // the two group widths
constexpr uint32_t AUD_ROUNDS = 4;
SUM_FN uint32_t aud_groups(uint32_t C, uint32_t G) {
  const uint32_t CPW = 64 / G;
  return (C + CPW - 1) / CPW;
}
SUM_FN uint32_t aud_grid(uint32_t C, uint32_t G) {
  const uint32_t wg = (aud_groups(C, G) + SUMMARY_WAVES - 1) / SUMMARY_WAVES;
  return wg < AUD_MAX_GRID ? wg : AUD_MAX_GRID;
}
SUM_FN uint32_t aud_chunks(uint32_t C) {
  return (C + AUD_ROUNDS * SUMMARY_BLOCK - 1) / (AUD_ROUNDS * SUMMARY_BLOCK);
}
// Partial summaries a shard's scratch holds: a handle may be queried at either width, so the
// larger of the two grids. The wide groups put one cluster on a wave, the narrow ones four, so the
// wide grid is the larger, up to four times.
SUM_FN uint32_t aud_parts(uint32_t C) {
  const uint32_t a = aud_grid(C, AUD_NARROW), b = aud_grid(C, AUD_WIDE);
  return a > b ? a : b;
}
SUM_FN SummaryLayout audit_layout(uint32_t C) {
  return {aud_parts(C), summary_F<raft_audit_t>, aud_chunks(C)};
}

}  // namespace rs
