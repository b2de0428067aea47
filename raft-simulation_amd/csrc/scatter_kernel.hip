// scatter_kernel.hip — cluster packs written back (gfx950): the inverse of gather_kernel.hip. Pack
// records (include/raftsim.h, "Cluster packs"; the layout: raft_gather_layout_t) become the state of
// arbitrary clusters of the shard; one record may become many clusters. Writes state only: the hot
// block, the queue rings, the arenas, commit_count and the commit-stream rings of every target --
// neither violation records nor counters nor trace rings (SIM_SPEC §6: none of them is pack state).
//
// Mapping: gather_kernel's turned round. `splits` workgroups of four waves per (record, target)
// pair, the groups of workgroups striding over the list of (target cluster, record slot) pairs;
// inside a pair every part is a flat array whose elements the lanes of the pair's workgroups take
// in order, adjacent lanes on adjacent bytes of the record:
//   - the hot block is encoded a word per lane (HB words), as raft_sim_write_nodes and
//     raft_sim_write_queue leave it: the cluster's five words, the reserved ones zero (which
//     clears the steady certificate, as every state writer does), the node fields from the node
//     records (FL_DRAW clear: a pack's deadline is the exact draw), the queue words from the
//     counts and the first and last message of each ring in the record, head 0, the pad zero;
//   - queues and arenas move 16 bytes per lane: message p of a ring goes to ring slot p, slots at
//     and past the count are written as zero; two arena entries are one uint4 store where the
//     cluster's first arena slot is even and both exist, and two uint2 stores otherwise (an odd
//     arena_cap puts every other cluster's arenas on an odd slot; the last entry of an odd total
//     is alone). Every load is one uint4 (parts start on 16 bytes and are padded to them);
//   - the commit-stream rings are rotated back a word per lane: ring slot s holds value p =
//     (s - (commit_count - kept)) mod SC of the record when p < kept = min(commit_count, SC).
// The counts a pair's parts need of its node records (req_count, res_count, commit_count) are read
// once per pair into LDS. The host has checked every record (scatter_host.hpp); the clamps here
// only keep a record it somehow let through inside its part.
#include <stddef.h>

#include <algorithm>

#include "device.hpp"

namespace rs {

constexpr uint32_t SCATTER_BLOCK = 256;
constexpr uint32_t SCATTER_MAX_GRID = 4096;       // pairs in flight
constexpr uint32_t SCATTER_SPLIT_BYTES = 32768;   // a workgroup's share of a record, at least
constexpr uint32_t SCATTER_MAX_SPLITS = 64;
constexpr uint32_t SC_NODE_WORDS = sizeof(raft_node_t) / 4;
static_assert(sizeof(raft_node_t) == 136 && sizeof(raft_msg_t) == 32 && sizeof(raft_entry_t) == 8 &&
                  sizeof(raft_cluster_t) == 32,
              "the record sizes the pack's layout is made of");
static_assert(offsetof(raft_node_t, role) == 0 && offsetof(raft_node_t, entries_is_seq) == 4 &&
                  offsetof(raft_node_t, votes) == 6 && offsetof(raft_node_t, ls_keys) == 8 &&
                  offsetof(raft_node_t, current_term) == 12 && offsetof(raft_node_t, deadline) == 24 &&
                  offsetof(raft_node_t, next_index) == 28 && offsetof(raft_node_t, match_index) == 64 &&
                  offsetof(raft_node_t, last_led_term) == 100 &&
                  offsetof(raft_node_t, arena_base) == 104 &&
                  offsetof(raft_node_t, req_count) == 112 &&
                  offsetof(raft_node_t, commit_count) == 120 &&
                  offsetof(raft_node_t, trace_hash) == 128 && offsetof(raft_msg_t, arrival) == 0,
              "scatter_hot_word's word numbers");

// Field f of node k's part of a hot block, from the node's record nw (34 words), its queue counts
// and the arrivals of the first and last message of its two rings (q: the node's REQ ring, then its
// RES ring, Q messages of 8 words each).
__device__ __forceinline__ uint32_t scatter_hot_word(uint32_t f, uint32_t N, uint32_t Q,
                                                     const uint32_t* __restrict__ nw,
                                                     const uint32_t* __restrict__ q, uint32_t rqc,
                                                     uint32_t rsc) {
  if (f >= HF_NEXT && f < HF_NEXT + 2 * N) {            // next_index, then match_index
    const uint32_t row = f >= HF_NEXT + N, p = f - HF_NEXT - row * N;
    return nw[7 + row * RAFT_MAX_NODES + p];
  }
  if (f == hf_abase(N)) return nw[26];
  if (f == hf_afront(N)) return nw[27];
  if (f == hf_led(N)) return nw[25];
  switch (f) {
    case HF_DEADLINE: return nw[6];
    case HF_TRACE_LO: return nw[32];
    case HF_TRACE_HI: return nw[33];
    case HF_QMETA: return pack_qmeta(0, rqc, 0, rsc);
    case HF_REQ_ARR: return rqc ? q[0] : INF;
    case HF_RES_ARR: return rsc ? q[(size_t)Q * 8] : INF;
    case HF_REQ_TAIL: return rqc ? q[(size_t)(rqc - 1) * 8] : 0u;
    case HF_RES_TAIL: return rsc ? q[(size_t)(Q + rsc - 1) * 8] : 0u;
    case HF_FLAGS: {                  // bytes role, voted_for, leader_id, fault | is_seq, ls_present
      const uint32_t a = nw[0], b = nw[1];
      return pack_flags(a & 3, (a >> 8) & 15, (a >> 16) & 15, (a >> 24) & 7, b & 1, (b >> 8) & 1);
    }
    case HF_MASKS: return nw[1] >> 16 | nw[2] << 16;    // votes | ls_keys << 16
    case HF_TERM: return nw[3];
    case HF_COMMIT: return nw[4];
    case HF_LEN: return nw[5];
    default: return 0u;                                 // the block's trailing pad
  }
}

// Y.off[b]: byte offset of part bit b in a record (the host refuses a pack without parts 0, 1, 2, 4,
// and without part 5 when SC > 0; part 3, the logs, is not read: the arenas are the log).
__global__ void __launch_bounds__(SCATTER_BLOCK)
scatter_kernel(const DevSim S, const uint2* __restrict__ pairs, uint32_t n, uint32_t splits,
               const raft_gather_layout_t Y, const uint8_t* __restrict__ in) {
  __shared__ uint32_t s_rq[RAFT_MAX_NODES], s_rs[RAFT_MAX_NODES], s_cc[RAFT_MAX_NODES];
  const uint32_t N = S.N, Q = S.Q, A = S.A, SC = S.SC, HB = S.HB, tid = threadIdx.x;
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  // this workgroup's lanes' first element of every part, and their step
  const uint32_t sp = blockIdx.x % splits, first = sp * SCATTER_BLOCK + tid;
  const uint32_t step = splits * SCATTER_BLOCK;
  for (uint32_t r = blockIdx.x / splits; r < n; r += gridDim.x / splits) {
    const uint32_t c = pairs[r].x;
    if (c >= S.C) continue;                              // (the host refuses such a list)
    const uint8_t* const rec = in + (size_t)pairs[r].y * Y.stride;
    const uint32_t* const nodes = reinterpret_cast<const uint32_t*>(rec + Y.off[1]);
    const uint32_t* const qwords = reinterpret_cast<const uint32_t*>(rec + Y.off[2]);
    __syncthreads();                                     // the pair before is done with the LDS
    if (tid < N) {
      const uint32_t* const nw = nodes + tid * SC_NODE_WORDS;
      // a queue never exceeds inbox_cap; the clamp keeps a corrupt count inside the ring
      s_rq[tid] = min(nw[28], Q);
      s_rs[tid] = min(nw[29], Q);
      s_cc[tid] = nw[30];
      if (sp == 0) S.ccount[(size_t)c * N + tid] = nw[30];
    }
    __syncthreads();

    {                                                    // the hot block, a word per lane
      uint32_t* const hb = hot_cl(S, c);
      const uint32_t* const cl = reinterpret_cast<const uint32_t*>(rec + Y.off[0]);
      const uint32_t fields = hf_led(N) + 1;
      for (uint32_t w = first; w < HB; w += step) {
        uint32_t v = 0;                                  // words 5-7 (CL_CTERM, CL_CERT) and the pad
        if (w <= CL_CLIENT_COUNT) {
          v = cl[w];
        } else if (w >= HOT_CW) {
          const uint32_t f = (w - HOT_CW) / N, k = (w - HOT_CW) - f * N;
          if (f < fields)
            v = scatter_hot_word(f, N, Q, nodes + k * SC_NODE_WORDS, qwords + (size_t)k * 2 * Q * 8,
                                 s_rq[k], s_rs[k]);
        }
        hb[w] = v;
      }
    }

    {                                                    // per node REQ then RES, message p to slot p
      const uint4* const src = reinterpret_cast<const uint4*>(rec + Y.off[2]);
      const uint32_t total = N * 2 * Q * 2;              // halves of messages
      for (uint32_t i = first; i < total; i += step) {
        const uint32_t half = i & 1, m = i >> 1, ring = m / Q, p = m - ring * Q;
        const uint32_t k = ring >> 1, which = ring & 1;
        const uint32_t cnt = which ? s_rs[k] : s_rq[k];
        uint4 v = zero4;
        if (p < cnt) v = src[i];
        reinterpret_cast<uint4*>(qslots(S, c * N + k, (int)which) +
                                 p * qstride(S, (int)which))[half] = v;
      }
    }

    {                                                    // per node the raw arena
      const uint4* const src = reinterpret_cast<const uint4*>(rec + Y.off[4]);
      const uint32_t entries = N * A, chunks = (entries + 1) >> 1;
      uint2* const ar = arena_of(S, c * N);
      const bool dst16 = (((size_t)c * N * A) & 1) == 0; // the cluster's first slot is even
      for (uint32_t i = first; i < chunks; i += step) {
        const uint4 v = src[i];                          // (the part is padded to 16 bytes)
        const bool both = 2 * i + 1 < entries;
        if (dst16 && both) {
          *reinterpret_cast<uint4*>(ar + 2 * i) = v;
        } else {
          ar[2 * i] = make_uint2(v.x, v.y);
          if (both) ar[2 * i + 1] = make_uint2(v.z, v.w);
        }
      }
    }

    if (SC) {                                            // per node the ring, rotated back
      const uint32_t* const src = reinterpret_cast<const uint32_t*>(rec + Y.off[5]);
      const uint32_t words = N * SC;
      for (uint32_t i = first; i < words; i += step) {
        const uint32_t k = i / SC, s = i - k * SC, cc = s_cc[k], kept = min(cc, SC);
        const uint32_t p = (s + SC - (cc - kept) % SC) % SC;
        S.stream[((size_t)c * N + k) * SC + s] = p < kept ? src[k * SC + p] : 0u;
      }
    }
  }
}

// Make the n clusters of `pairs` (device: x = shard-local cluster, y = record slot) the records of
// layout Y at in + slot * Y.stride.
hipError_t launch_scatter(const DevSim& S, const void* pairs, uint32_t n,
                          const raft_gather_layout_t& Y, const void* in, hipStream_t st) {
  if (!n) return hipSuccess;
  const uint32_t splits = (uint32_t)std::min<uint64_t>(
      std::max<uint64_t>(Y.stride / SCATTER_SPLIT_BYTES, 1), SCATTER_MAX_SPLITS);
  hipLaunchKernelGGL(scatter_kernel, dim3(std::min(n, SCATTER_MAX_GRID) * splits),
                     dim3(SCATTER_BLOCK), 0, st, S, static_cast<const uint2*>(pairs), n, splits, Y,
                     static_cast<const uint8_t*>(in));
  return hipGetLastError();
}

}  // namespace rs
