// census_kernel.hip — the state census and the selection of clusters by state class (gfx950):
// read-only queries over the hot blocks as they stand between launches (include/raftsim.h,
// "State census"; the classes: SIM_SPEC.md, "Derived, not state").
//
// Mapping: the tick kernel's. One lane per node, floor(64 / N) whole clusters per wave, so every
// field load of a wave is one contiguous N-word run per cluster (word HOT_CW + f * N + k of the
// block, device.hpp) and a cluster's facts are wave-native: the ballot of "live leader" shifted
// down to the cluster's lanes is the record's `leaders` mask, its popcount the leader count. Five
// fields are read per node (flags, term, commit, len, qmeta) and, by the census, cluster word 0
// (the checker's hwm index): at N = 5 words 0, 23-27, 48-52 and 58-72 of the block, three of its
// five 128-B lines. No deadline is read, so a deferred draw (FL_DRAW) only needs masking off, and
// a block under a steady certificate holds true words in every line.
//
// Census: a fixed grid of workgroups strides over the wave-sized groups of clusters. Counts are
// popcounts of ballots kept in scalar registers, sums and extrema one accumulator per lane; at the
// end every workgroup reduces to one raft_census_t in scratch and a second, one-workgroup kernel
// folds those (summary.hpp: no atomics, the result depends on no arrival or dispatch order).
//
// Selection: the compaction of compact.hpp (count / scan / scatter over chunks of consecutive
// clusters, the one the violation query runs over its records) over the source at the end of this
// file. The class word is recomputed in both passes: storing it would cost a write and a read of
// 4 B per cluster to save the second read of lines the first pass has just pulled through L2. The
// cluster's first lane stands for it in the ballot that ranks the matches; the record's
// per-cluster extrema are taken by shuffles over the cluster's lanes, in waves that hold a match
// only.
#include "summary.hpp"

namespace rs {

constexpr uint32_t CEN_BLOCK = SUMMARY_BLOCK;        // four waves, also for the census proper
constexpr uint32_t CEN_WAVES = SUMMARY_WAVES;
constexpr uint32_t CEN_F = summary_F<raft_census_t>; // u64 fields of a census
static_assert(sizeof(raft_cluster_state_t) == 32, "raft_cluster_state_t is eight words");

#define CEN_IDX(field) ((uint32_t)(offsetof(raft_census_t, field) / 8))

// A lane's node and its cluster's facts (the facts are the same on every lane of the cluster).
struct CenLane {
  bool act;                      // the lane holds a node: its slot is a whole cluster below C
  bool head;                     // ... and it is the cluster's first lane
  uint32_t c, k, sh;             // cluster, node index (id - 1), the cluster's first lane
  uint32_t role, lid, fault, term, commit, len, rq, rs;
  uint32_t classes, leaders, live, halted;   // class bits; lane-local masks (bit k = node k)
};

__device__ __forceinline__ uint32_t cen_seg(uint64_t ballot, uint32_t sh, uint32_t seg) {
  return (uint32_t)(ballot >> sh) & seg;
}

// Load the lane's node of group g0 (clusters g0 * CPW ...) and classify its cluster. Every lane of
// the wave must call it (ballots and shuffles). block: the cluster's block, for the caller's own
// loads (valid when act).
__device__ __forceinline__ CenLane cen_load(const uint32_t* __restrict__ hot, uint32_t HB,
                                            uint32_t N, uint32_t C, uint32_t L, uint32_t quorum,
                                            uint32_t group, uint32_t slot, uint32_t k,
                                            const uint32_t** block) {
  const uint32_t CPW = 64 / N, seg = (1u << N) - 1;
  CenLane n;
  // group < ceil(C / CPW), so group * CPW + slot stays far below 2^32 (C * N < 2^31)
  n.c = group * CPW + slot;
  n.k = k;
  n.sh = slot * N;                                   // <= 63, also on the wave's spare lanes
  n.act = slot < CPW && n.c < C;
  n.head = n.act && k == 0;
  uint32_t fl = 0, qm = 0;
  n.term = n.commit = n.len = 0;
  const uint32_t* b = hot;
  if (n.act) {
    b = hot + (size_t)n.c * HB;
    const uint32_t* p = b + HOT_CW + k;              // field f at p[f * N]
    fl = p[HF_FLAGS * N];
    n.term = p[HF_TERM * N];
    n.commit = p[HF_COMMIT * N];
    n.len = p[HF_LEN * N];
    qm = p[HF_QMETA * N];
  }
  *block = b;
  n.role = fl_role(fl);                              // bit 15, FL_DRAW, is not state
  n.lid = fl_lid(fl);
  n.fault = fl_fault(fl);
  n.rq = qm_req_cnt(qm);
  n.rs = qm_res_cnt(qm);
  const bool live = n.act && n.fault == 0;
  const bool lead = live && n.role == RAFT_LEADER;
  n.live = cen_seg(__ballot(live), n.sh, seg);
  n.leaders = cen_seg(__ballot(lead), n.sh, seg);
  n.halted = cen_seg(__ballot(n.act && n.fault != 0), n.sh, seg);
  const uint32_t cand = cen_seg(__ballot(live && n.role == RAFT_CANDIDATE), n.sh, seg);
  const uint32_t full = cen_seg(__ballot(n.act && n.len == L), n.sh, seg);
  const uint32_t nl = (uint32_t)__popc(n.leaders), nlive = (uint32_t)__popc(n.live);
  // settled: the one leader's id and term on every live node (its own lane included)
  const uint32_t lk = n.leaders ? (uint32_t)__ffs(n.leaders) - 1 : 0u;
  const uint32_t lterm = (uint32_t)__shfl((int)n.term, (int)min(n.sh + lk, 63u));
  const bool off = live && !(n.lid == lk + 1 && n.term == lterm);
  const uint32_t offs = cen_seg(__ballot(off), n.sh, seg);
  // two leaders in one term: only waves that hold a cluster with two leaders look
  uint32_t same = 0;
  if (__ballot(n.act && nl >= 2)) {                  // wave-uniform
    bool eq = false;
    for (uint32_t j = 0; j < N; ++j) {
      const uint32_t tj = (uint32_t)__shfl((int)n.term, (int)min(n.sh + j, 63u));
      eq = eq || (lead && j != k && ((n.leaders >> j) & 1) && tj == n.term);
    }
    same = cen_seg(__ballot(eq), n.sh, seg);
  }
  uint32_t cls = nl == 0 ? RAFT_CLS_NO_LEADER : nl == 1 ? RAFT_CLS_ONE_LEADER : RAFT_CLS_MULTI_LEADER;
  if (n.halted) cls |= RAFT_CLS_HALTED;
  if (nlive < quorum) cls |= RAFT_CLS_NO_QUORUM;
  if (same) cls |= RAFT_CLS_SAME_TERM_LEADERS;
  if (full) cls |= RAFT_CLS_LOG_FULL;
  if (cand) cls |= RAFT_CLS_CANDIDATE;
  if (nl == 1 && !offs) cls |= RAFT_CLS_SETTLED;
  n.classes = n.act ? cls : 0u;
  return n;
}

// The census of the groups this workgroup strides over: part[blockIdx.x] (CEN_F u64 fields).
__global__ void __launch_bounds__(CEN_BLOCK)
census_kernel(const uint32_t* __restrict__ hot, uint32_t HB, uint32_t N, uint32_t C, uint32_t L,
              uint32_t quorum, unsigned long long* __restrict__ part) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t slot = lane / N, k = lane - slot * N;
  const uint32_t groups = cen_groups(C, N);
  // per-lane counts, in the order of the census's leading fields (clusters, nodes, by_class,
  // leaders_hist, live_hist, role_nodes, fault_nodes): a lane counts its own node, the cluster's
  // first lane the cluster; constant indices only, so the array lives in registers
  constexpr uint32_t NCNT = CEN_IDX(term_min);
  static_assert(NCNT == 2 + 16 + 2 * (RAFT_MAX_NODES + 1) + 4 + 5 &&
                    CEN_IDX(hwm_sum) + 1 == CEN_F && CEN_F == NCNT + 11,
                "the counts, then eleven sums and extrema: every field is stored below");
  uint32_t cnt[NCNT] = {};
  // per-lane sums and extrema
  uint64_t tsum = 0, csum = 0, lsum = 0, rqs = 0, rss = 0, hsum = 0, tmin = ~0ull;
  uint32_t tmax = 0, cmax = 0, lmax = 0, hmax = 0;
  for (uint32_t g = blockIdx.x * CEN_WAVES + wv; g < groups; g += gridDim.x * CEN_WAVES) {
    const uint32_t* b;
    const CenLane n = cen_load(hot, HB, N, C, L, quorum, g, slot, k, &b);
    const bool live = n.act && n.fault == 0;
    cnt[CEN_IDX(clusters)] += n.head;
    cnt[CEN_IDX(nodes)] += n.act;
#pragma unroll
    for (uint32_t i = 0; i < 9; ++i) cnt[CEN_IDX(by_class) + i] += n.head && ((n.classes >> i) & 1);
    const uint32_t nl = (uint32_t)__popc(n.leaders), nv = (uint32_t)__popc(n.live);
#pragma unroll
    for (uint32_t i = 0; i <= RAFT_MAX_NODES; ++i) {
      cnt[CEN_IDX(leaders_hist) + i] += n.head && nl == i;
      cnt[CEN_IDX(live_hist) + i] += n.head && nv == i;
    }
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) cnt[CEN_IDX(role_nodes) + i] += live && n.role == i;
#pragma unroll
    for (uint32_t i = 0; i < 5; ++i) cnt[CEN_IDX(fault_nodes) + i] += n.act && n.fault == i;
    if (n.act) {
      tsum += n.term; csum += n.commit; lsum += n.len; rqs += n.rq; rss += n.rs;
      tmin = min(tmin, (uint64_t)n.term); tmax = max(tmax, n.term);
      cmax = max(cmax, n.commit); lmax = max(lmax, n.len);
    }
    if (n.head) {
      const uint32_t hwm = b[CL_HWM_IDX];
      hsum += hwm;
      hmax = max(hmax, hwm);
    }
  }
  // the eleven fields after the counts, widened. A wave's counts stay below 2^32 (64 lanes, at
  // most 2^18 groups per wave: C * N < 2^31 over 4,096 waves).
  uint64_t x[CEN_F - NCNT];
  x[CEN_IDX(term_min) - NCNT] = tmin; x[CEN_IDX(term_max) - NCNT] = tmax;
  x[CEN_IDX(term_sum) - NCNT] = tsum;
  x[CEN_IDX(commit_max) - NCNT] = cmax; x[CEN_IDX(commit_sum) - NCNT] = csum;
  x[CEN_IDX(len_max) - NCNT] = lmax; x[CEN_IDX(len_sum) - NCNT] = lsum;
  x[CEN_IDX(req_queued) - NCNT] = rqs; x[CEN_IDX(res_queued) - NCNT] = rss;
  x[CEN_IDX(hwm_max) - NCNT] = hmax; x[CEN_IDX(hwm_sum) - NCNT] = hsum;
  summary_block_store<raft_census_t, NCNT>(cnt, x, part);
}

// The selection's source for the compaction (compact.hpp): group (round * CEN_WAVES + wave) of the
// chunk in round `round`, so the clusters rise with (round, wave, lane); the cluster's first lane
// holds its item. out is [cap] raft_cluster_state_t, written as two 16-byte stores.
struct cen_select {
  static constexpr uint32_t ROUNDS = CEN_ROUNDS;
  struct Item {
    CenLane n;
    uint32_t tmax, tmin, cmax, lmax, queued;         // the lane's own, after gather the cluster's
  };
  const uint32_t* __restrict__ hot;
  uint32_t HB, N, C, L, quorum, any, all, none;
  uint4* __restrict__ out;

  __host__ __device__ uint32_t chunks() const { return cen_chunks(C, N); }
  __device__ __forceinline__ Item load(uint32_t b, uint32_t i) const {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t slot = lane / N, k = lane - slot * N;
    const uint32_t* blk;
    Item it;
    it.n = cen_load(hot, HB, N, C, L, quorum, (b * ROUNDS + i) * CEN_WAVES + wv, slot, k, &blk);
    const CenLane& n = it.n;
    it.tmax = it.tmin = n.term; it.cmax = n.commit; it.lmax = n.len; it.queued = n.rq + n.rs;
    return it;
  }
  __device__ __forceinline__ bool match(const Item& it) const {
    return it.n.head && class_match(it.n.classes, any, all, none);
  }
  // the record's extrema and sum over the cluster's N lanes, gathered by its first lane
  __device__ __forceinline__ void gather(Item& it) const {
    const CenLane& n = it.n;
    for (uint32_t j = 1; j < N; ++j) {
      const int src = (int)min(n.sh + j, 63u);
      const uint32_t t = (uint32_t)__shfl((int)n.term, src);
      const uint32_t c = (uint32_t)__shfl((int)n.commit, src);
      const uint32_t l = (uint32_t)__shfl((int)n.len, src);
      const uint32_t q = (uint32_t)__shfl((int)(n.rq + n.rs), src);
      it.tmax = max(it.tmax, t); it.tmin = min(it.tmin, t);
      it.cmax = max(it.cmax, c); it.lmax = max(it.lmax, l);
      it.queued += q;
    }
  }
  __device__ __forceinline__ void store(const Item& it, uint32_t o) const {
    const CenLane& n = it.n;
    uint4* const p = out + (size_t)o * 2;
    // cluster, classes, leaders | halted << 16 (bit i: id i, as votes), term_max
    p[0] = make_uint4(n.c, n.classes, (n.leaders << 1) | (n.halted << 17), it.tmax);
    p[1] = make_uint4(it.tmin, it.cmax, it.lmax, it.queued);
  }
};

uint32_t census_quorum(uint32_t N, uint32_t variant) {
  return variant & RAFT_VARIANT_SPEC ? N / 2 + 1 : (N + 1) >> 1;
}

// The census of shard S: scratch[census_layout(C, N).result() ...] receives its raft_census_t.
hipError_t launch_census(const DevSim& S, unsigned long long* scratch, hipStream_t st) {
  return launch_summary<raft_census_t>(
      census_layout(S.C, S.N), scratch, cen_grid(S.C, S.N), st,
      [&](dim3 grid, unsigned long long* part) {
        hipLaunchKernelGGL(census_kernel, grid, dim3(CEN_BLOCK), 0, st, (const uint32_t*)S.hot,
                           S.HB, S.N, S.C, S.L, census_quorum(S.N, S.variant), part);
      });
}

// The selection over shard S: *census_layout(C, N).total_ptr(scratch) receives the total, out (cap
// records; may be null when cap is 0) the first min(total, cap) matches with shard-local cluster
// indices.
hipError_t launch_census_select(const DevSim& S, uint32_t any, uint32_t all, uint32_t none,
                                unsigned long long* scratch, void* out, uint32_t cap,
                                hipStream_t st) {
  const cen_select src = {S.hot, S.HB, S.N, S.C, S.L, census_quorum(S.N, S.variant),
                          any, all, none, static_cast<uint4*>(out)};
  return launch_compact(src, census_layout(S.C, S.N).counts_ptr(scratch), cap, st);
}

}  // namespace rs
