// audit_kernel.hip — the log audit (gfx950): do the nodes' logs of a cluster agree as they stand,
// and is a disagreement below the commit indices (include/raftsim.h, "Log audit"; the classes:
// SIM_SPEC.md, "Derived, not state"). The first query that reads the arenas: bandwidth-bound.
//
// Mapping: a group of G lanes per cluster, 64 / G clusters per wave, adjacent lanes on adjacent log
// positions of one node. A step covers G positions: for every node one dwordx2 load per lane, G
// consecutive 8-byte entries of that node's arena, whole 128-B lines (G = 16: one line per node
// and step; an arena's end splits a run in two, per node). A lane then holds the N entries of its
// position and compares the N (N - 1) / 2 pairs in registers; nothing of a log passes through LDS.
// Positions at or past a node's len are not loaded and take no part in any comparison. G is 64 (the
// default: faster on handles whose logs are long, where the pass takes milliseconds) or 16 (faster
// by a sixth where the logs are empty; RAFTSIM_AUDIT_WIDTH=16, raftsim.hip; DESIGN.md has both
// widths' figures); the waves of a workgroup stride over the groups of clusters on a fixed grid.
//
// What needs more than a lane's own position:
//   - bits 1 and 2, the indices and the node masks do not: a differing position is a hit wherever
//     it lies, the smallest over lanes and steps is the index, the pairs that differ anywhere are
//     the masks. Per-lane minima and pair masks, reduced over the group once per cluster.
//   - bit 4 needs, per pair, "a difference at or before this position": the pairs that differed in
//     earlier steps (one pair mask, the same on every lane of the group) OR an inclusive prefix-OR
//     of this step's differing-pair masks over the group's lanes. Waves in which no pair has
//     differed yet skip it.
//   - bit 8 needs the previous position's term: the left neighbour's, and for a group's first lane
//     the last lane's of the step before (one rotation per node and step gives both).
//
// The pass writes one 32-byte record per cluster and, like the census, one partial summary per
// workgroup that a second one-workgroup kernel folds (summary.hpp: no atomics, the result depends
// on no arrival order). The selection is the compaction of compact.hpp over the record buffer.
#include <type_traits>

#include "summary.hpp"

namespace rs {

constexpr uint32_t AUD_BLOCK = SUMMARY_BLOCK;        // four waves
constexpr uint32_t AUD_WAVES = SUMMARY_WAVES;
constexpr uint32_t AUD_F = summary_F<raft_audit_t>;  // u64 fields of a summary
static_assert(sizeof(raft_audit_record_t) == 32, "raft_audit_record_t is eight words");

#define AUD_IDX(field) ((uint32_t)(offsetof(raft_audit_t, field) / 8))

// Shuffles of a pair mask inside a group of G lanes (32 bits hold the pairs up to N = 8).
template <uint32_t G>
__device__ __forceinline__ uint32_t aud_shfl(uint32_t x, int src) {
  return (uint32_t)__shfl((int)x, src, (int)G);
}
template <uint32_t G>
__device__ __forceinline__ uint64_t aud_shfl(uint64_t x, int src) {
  return (uint64_t)aud_shfl<G>((uint32_t)(x >> 32), src) << 32 | aud_shfl<G>((uint32_t)x, src);
}
template <uint32_t G>
__device__ __forceinline__ uint32_t aud_shfl_up(uint32_t x, int d) {
  return (uint32_t)__shfl_up((int)x, d, (int)G);
}
template <uint32_t G>
__device__ __forceinline__ uint64_t aud_shfl_up(uint64_t x, int d) {
  return (uint64_t)aud_shfl_up<G>((uint32_t)(x >> 32), d) << 32 | aud_shfl_up<G>((uint32_t)x, d);
}
template <uint32_t G>
__device__ __forceinline__ uint32_t aud_shfl_xor(uint32_t x, int d) {
  return (uint32_t)__shfl_xor((int)x, d, (int)G);
}
template <uint32_t G>
__device__ __forceinline__ uint64_t aud_shfl_xor(uint64_t x, int d) {
  return (uint64_t)aud_shfl_xor<G>((uint32_t)(x >> 32), d) << 32 | aud_shfl_xor<G>((uint32_t)x, d);
}

// The audit pass: rec[c] = cluster c's record (two uint4), part[blockIdx.x] = the summary of the
// clusters this workgroup strode over (AUD_F u64 fields). arena: [C * N][A] entries (term, val).
template <uint32_t N, uint32_t G>
__global__ void __launch_bounds__(AUD_BLOCK)
audit_kernel(const uint32_t* __restrict__ hot, uint32_t HB, const uint2* __restrict__ arena,
             uint32_t A, uint32_t C, uint4* __restrict__ rec,
             unsigned long long* __restrict__ part) {
  constexpr uint32_t CPW = 64 / G, NP = N * (N - 1) / 2;
  using PM = typename std::conditional<(NP <= 32), uint32_t, uint64_t>::type;   // one bit per pair
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t gl = lane & (G - 1), slot = lane / G, gbase = lane - gl;
  const uint32_t groups = aud_groups(C, G);
  // the summary's accumulators: a group's first lane counts its cluster. A lane's counts stay
  // below 2^32 (the node masks' popcounts sum to at most C * N < 2^31).
  uint32_t n_cl = 0, n_cls[5] = {}, n_div = 0, n_cdiv = 0;
  uint64_t entries = 0, agree_sum = 0;
  uint32_t agree_min = INF, agree_max = 0, div_min = INF, cdiv_min = INF;
  for (uint32_t g = blockIdx.x * AUD_WAVES + wv; g < groups; g += gridDim.x * AUD_WAVES) {
    const uint32_t c = g * CPW + slot;               // g < ceil(C / CPW): far below 2^32
    const bool act = c < C;
    // len, commit and arena_base of the N nodes, the same words on every lane of the group. No
    // deadline is read, so an owed draw (FL_DRAW) does not matter.
    uint32_t len[N], cm[N], off[N];
    uint32_t lmax = 0, lmin = INF, nonempty = 0, lsum = 0;
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
      len[k] = cm[k] = off[k] = 0;
      if (act) {
        const uint32_t* p = hot + (size_t)c * HB + HOT_CW + k;   // field f at p[f * N]
        // a log never exceeds log_cap <= A / 2; the clamp keeps a corrupt word inside the arena
        len[k] = min(p[HF_LEN * N], A);
        cm[k] = p[HF_COMMIT * N];
        off[k] = p[hf_abase(N) * N] % A;
      }
      lmax = max(lmax, len[k]);
      lmin = min(lmin, len[k]);
      lsum += len[k];
      nonempty += len[k] != 0;
    }
    // Nothing to compare and no adjacent pair of entries anywhere: no arena load (an empty handle
    // is read from its hot words alone).
    const bool walk = act && (lmax >= 2 || nonempty >= 2);
    const uint32_t end = walk ? lmax : 0;
    const uint2* const ar = arena + (walk ? (size_t)c * N * A : 0);
    PM carry = 0, cpm = 0;         // pairs that differed in earlier steps (group-uniform) / below
                                   // both commits (the lane's own)
    uint32_t dmin = INF, cmin = INF, omin = INF;
    bool broken = false;
    uint32_t last[N];              // on a group's first lane: the last term of the step before
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) last[k] = 0;
    for (uint32_t p0 = 0; __ballot(p0 < end) != 0; p0 += G) {     // wave-uniform trip count
      const uint32_t p = p0 + gl;
      uint32_t t[N], v[N];
      bool ok[N];
#pragma unroll
      for (uint32_t k = 0; k < N; ++k) {
        ok[k] = walk && p < len[k];
        t[k] = v[k] = 0;
        if (ok[k]) {
          uint32_t s = off[k] + p;                   // < 2 A
          s = s >= A ? s - A : s;
          const uint2 e = ar[(size_t)k * A + s];
          t[k] = e.x;
          v[k] = e.y;
        }
      }
      // bit 8: position p - 1 against p (p < len implies p - 1 < len)
#pragma unroll
      for (uint32_t k = 0; k < N; ++k) {
        const uint32_t r = aud_shfl<G>(t[k], (int)((gl + G - 1) & (G - 1)));
        const uint32_t prev = gl == 0 ? last[k] : r;
        last[k] = r;
        if (ok[k] && p >= 1 && prev > t[k]) omin = min(omin, p - 1);
      }
      PM dm = 0, cd = 0, em = 0;   // pairs that differ here / below both commits / share the term
      {
        uint32_t b = 0;
#pragma unroll
        for (uint32_t i = 0; i < N; ++i)
#pragma unroll
          for (uint32_t j = i + 1; j < N; ++j, ++b) {
            const bool both = ok[i] && ok[j];
            const bool ne = t[i] != t[j] || v[i] != v[j];
            if (both && ne) dm |= (PM)1 << b;
            if (both && ne && p < min(cm[i], cm[j])) cd |= (PM)1 << b;
            if (both && t[i] == t[j]) em |= (PM)1 << b;
          }
      }
      if (dm) dmin = min(dmin, p);
      if (cd) cmin = min(cmin, p);
      cpm |= cd;
      if (__ballot(dm != 0 || carry != 0)) {         // wave-uniform
        PM pre = dm;               // inclusive prefix-OR over the group's lanes (a lane below the
#pragma unroll                     // shift gets its own value back: OR-ing it changes nothing)
        for (uint32_t d = 1; d < G; d <<= 1) pre |= aud_shfl_up<G>(pre, (int)d);
        broken = broken || ((pre | carry) & em) != 0;
        carry |= aud_shfl<G>(pre, (int)(G - 1));
      }
    }
    // the group's facts: carry is the pairs that differ anywhere already
#pragma unroll
    for (uint32_t d = 1; d < G; d <<= 1) {
      cpm |= aud_shfl_xor<G>(cpm, (int)d);
      dmin = min(dmin, aud_shfl_xor<G>(dmin, (int)d));
      cmin = min(cmin, aud_shfl_xor<G>(cmin, (int)d));
      omin = min(omin, aud_shfl_xor<G>(omin, (int)d));
    }
    const uint64_t gmask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1) << gbase;
    broken = (__ballot(broken) & gmask) != 0;
    uint32_t dn = 0, cn = 0;       // bit i: id i is in such a pair (as votes)
    {
      uint32_t b = 0;
#pragma unroll
      for (uint32_t i = 0; i < N; ++i)
#pragma unroll
        for (uint32_t j = i + 1; j < N; ++j, ++b) {
          if ((carry >> b) & 1) dn |= 2u << i | 2u << j;
          if ((cpm >> b) & 1) cn |= 2u << i | 2u << j;
        }
    }
    uint32_t cls = 0;
    if (carry) cls |= RAFT_AUD_DIVERGED;
    if (cpm) cls |= RAFT_AUD_COMMIT_DIVERGED;
    if (broken) cls |= RAFT_AUD_MATCH_BROKEN;
    if (omin != INF) cls |= RAFT_AUD_TERM_ORDER;
    if (!carry && lmax == lmin) cls |= RAFT_AUD_IDENTICAL;
    const uint32_t agree = min(lmin, dmin);
    if (act && gl == 0) {
      uint4* const o = rec + (size_t)c * 2;
      o[0] = make_uint4(c, cls, agree, dmin);
      o[1] = make_uint4(cmin, omin, dn | cn << 16, lmin);
      ++n_cl;
#pragma unroll
      for (uint32_t i = 0; i < 5; ++i) n_cls[i] += (cls >> i) & 1;
      entries += lsum;
      agree_sum += agree;
      agree_min = min(agree_min, agree);
      agree_max = max(agree_max, agree);
      n_div += (uint32_t)__popc(dn);
      n_cdiv += (uint32_t)__popc(cn);
      div_min = min(div_min, dmin);
      cdiv_min = min(cdiv_min, cmin);
    }
  }
  // the lane's summary: a 32-bit "none" (INF) widens to the summary's UINT64_MAX
  auto wide = [](uint32_t x) { return x == INF ? ~0ull : (uint64_t)x; };
  uint64_t x[AUD_F];
#pragma unroll
  for (uint32_t f = 0; f < AUD_F; ++f) x[f] = 0;
  x[AUD_IDX(clusters)] = n_cl;
#pragma unroll
  for (uint32_t i = 0; i < 5; ++i) x[AUD_IDX(by_class) + i] = n_cls[i];
  x[AUD_IDX(entries)] = entries;
  x[AUD_IDX(agree_sum)] = agree_sum;
  x[AUD_IDX(agree_min)] = wide(agree_min);
  x[AUD_IDX(agree_max)] = agree_max;
  x[AUD_IDX(diverged_nodes)] = n_div;
  x[AUD_IDX(commit_diverged_nodes)] = n_cdiv;
  x[AUD_IDX(diverge_index_min)] = wide(div_min);
  x[AUD_IDX(commit_diverge_index_min)] = wide(cdiv_min);
  summary_block_store<raft_audit_t, 0>(nullptr, x, part);
}

// The selection's source for the compaction (compact.hpp): one record per lane, so the clusters
// rise with (chunk, round, wave, lane). The counting pass uses the class word alone.
struct aud_select {
  static constexpr uint32_t ROUNDS = AUD_ROUNDS;
  struct Item {
    uint4 a, b;
    bool act;
  };
  const uint4* __restrict__ rec;
  uint32_t C, any, all, none;
  uint4* __restrict__ out;

  __host__ __device__ uint32_t chunks() const { return aud_chunks(C); }
  __device__ __forceinline__ Item load(uint32_t b, uint32_t i) const {
    const uint32_t c = (b * ROUNDS + i) * COMPACT_BLOCK + threadIdx.x;   // < C + a chunk
    Item it;
    it.act = c < C;
    it.a = it.b = make_uint4(0, 0, 0, 0);
    if (it.act) {
      it.a = rec[(size_t)c * 2];
      it.b = rec[(size_t)c * 2 + 1];
    }
    return it;
  }
  __device__ __forceinline__ bool match(const Item& it) const {
    return it.act && class_match(it.a.y, any, all, none);
  }
  __device__ __forceinline__ void gather(Item&) const {}
  __device__ __forceinline__ void store(const Item& it, uint32_t o) const {
    out[(size_t)o * 2] = it.a;
    out[(size_t)o * 2 + 1] = it.b;
  }
};

template <uint32_t G>
static void aud_pass(const DevSim& S, uint4* rec, dim3 grid, unsigned long long* part,
                     hipStream_t st) {
  const dim3 block(AUD_BLOCK);
  const uint32_t* hot = S.hot;
  const uint2* arena = reinterpret_cast<const uint2*>(S.arena);
#define AUD_CASE(n)                                                                            \
  case n:                                                                                      \
    hipLaunchKernelGGL((audit_kernel<n, G>), grid, block, 0, st, hot, S.HB, arena, S.A, S.C,  \
                       rec, part);                                                             \
    break;
  switch (S.N) {
    AUD_CASE(2) AUD_CASE(3) AUD_CASE(4) AUD_CASE(5) AUD_CASE(6) AUD_CASE(7) AUD_CASE(8)
    AUD_CASE(9)
  }
#undef AUD_CASE
}

// The audit pass over shard S with groups of `width` lanes (64, or 16): rec (S.C records) receives
// every cluster's record with shard-local cluster indices, scratch[audit_layout(C).result() ...]
// the shard's raft_audit_t.
hipError_t launch_audit(const DevSim& S, uint32_t width, void* rec, unsigned long long* scratch,
                        hipStream_t st) {
  const bool wide = width == AUD_WIDE;
  uint4* const r = static_cast<uint4*>(rec);
  return launch_summary<raft_audit_t>(
      audit_layout(S.C), scratch, aud_grid(S.C, wide ? AUD_WIDE : AUD_NARROW), st,
      [&](dim3 grid, unsigned long long* part) {
        if (wide) aud_pass<AUD_WIDE>(S, r, grid, part, st);
        else aud_pass<AUD_NARROW>(S, r, grid, part, st);
      });
}

// The selection over the C records of rec: *audit_layout(C).total_ptr(scratch) receives the total,
// out (cap records; may be null when cap is 0) the first min(total, cap) matches.
hipError_t launch_audit_select(uint32_t C, uint32_t any, uint32_t all, uint32_t none,
                               const void* rec, unsigned long long* scratch, void* out,
                               uint32_t cap, hipStream_t st) {
  const aud_select src = {static_cast<const uint4*>(rec), C, any, all, none,
                          static_cast<uint4*>(out)};
  return launch_compact(src, audit_layout(C).counts_ptr(scratch), cap, st);
}

}  // namespace rs
