// scatter_kernel.hip — cluster packs written back (gfx950): the inverse of gather_kernel.hip. Pack
// records (include/raftsim.h, "Cluster packs"; the layout: raft_gather_layout_t) become the state of
// arbitrary clusters of the shard; one record may become many clusters. Writes state only: the hot
// block, the queue rings, the arenas, commit_count and the commit-stream rings of every target --
// neither violation records nor counters nor trace rings (SIM_SPEC §6: none of them is pack state).
//
// Mapping: gather_kernel's turned round, with its launch shape and a workgroup's share (pack.hpp).
// `splits` workgroups of four waves per (record, target) pair, the groups of workgroups striding
// over the list of (target cluster, record slot) pairs; inside a pair every part is a flat array
// whose elements the lanes of the pair's workgroups take in order, adjacent lanes on adjacent bytes
// of the record:
//   - the hot block is encoded a word per lane (HB words), as raft_sim_write_nodes and
//     raft_sim_write_queue leave it, by the functions they use (node_codec.hpp): the cluster's five
//     words, the reserved ones zero (which clears the steady certificate, as every state writer
//     does), the node fields from the node records (hot_field; FL_DRAW clear: a pack's deadline is
//     the exact draw), the queue words from the counts and the first and last message of each ring
//     in the record (queue_field; head 0), the pad zero;
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
#include "pack.hpp"

namespace rs {

// Y.off[b]: byte offset of part bit b in a record (the host refuses a pack without parts 0, 1, 2, 4,
// and without part 5 when SC > 0; part 3, the logs, is not read: the arenas are the log).
__global__ void __launch_bounds__(PACK_BLOCK)
scatter_kernel(const DevSim S, const uint2* __restrict__ pairs, uint32_t n, uint32_t splits,
               const raft_gather_layout_t Y, const uint8_t* __restrict__ in) {
  __shared__ uint32_t s_rq[RAFT_MAX_NODES], s_rs[RAFT_MAX_NODES], s_cc[RAFT_MAX_NODES];
  const uint32_t N = S.N, Q = S.Q, A = S.A, SC = S.SC, HB = S.HB, tid = threadIdx.x;
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  const PackLanes ln(splits);
  const uint32_t first = ln.first, step = ln.step;
  for (uint32_t r = ln.r0; r < n; r += ln.rstep) {
    const uint32_t c = pairs[r].x;
    if (c >= S.C) continue;                              // (the host refuses such a list)
    const uint8_t* const rec = in + (size_t)pairs[r].y * Y.stride;
    const uint32_t* const nodes = reinterpret_cast<const uint32_t*>(rec + Y.off[1]);
    const uint32_t* const qwords = reinterpret_cast<const uint32_t*>(rec + Y.off[2]);
    __syncthreads();                                     // the pair before is done with the LDS
    if (tid < N) {
      const uint32_t* const nw = nodes + tid * NODE_WORDS;
      // a queue never exceeds inbox_cap; the clamp keeps a corrupt count inside the ring
      s_rq[tid] = min(nw[NW_REQ_COUNT], Q);
      s_rs[tid] = min(nw[NW_RES_COUNT], Q);
      s_cc[tid] = nw[NW_COMMIT_COUNT];
      if (ln.sp == 0) S.ccount[(size_t)c * N + tid] = nw[NW_COMMIT_COUNT];
    }
    __syncthreads();

    {                                                    // the hot block, a word per lane
      uint32_t* const hb = hot_cl(S, c);
      const uint32_t* const cl = reinterpret_cast<const uint32_t*>(rec + Y.off[0]);
      for (uint32_t w = first; w < HB; w += step) {
        uint32_t v = 0;                                  // words 5-7 (CL_CTERM, CL_CERT) and the pad
        if (w <= CL_CLIENT_COUNT) {
          v = cl[w];
        } else if (w >= HOT_CW) {
          const uint32_t f = (w - HOT_CW) / N, k = (w - HOT_CW) - f * N;
          // the node's REQ ring in the record, then its RES ring, Q messages each
          const uint32_t* const rq = qwords + (size_t)k * 2 * Q * MSG_WORDS;
          if (hf_is_queue(f)) v = queue_field(f, s_rq[k], rq, s_rs[k], rq + Q * MSG_WORDS);
          else if (f < hot_fields(N)) v = hot_field(nodes + k * NODE_WORDS, N, f);
        }
        hb[w] = v;
      }
    }

    {                                                    // per node REQ then RES, message p to slot p
      const uint4* const src = reinterpret_cast<const uint4*>(rec + Y.off[2]);
      const uint32_t total = N * 2 * Q * 2;              // halves of messages
      for (uint32_t i = first; i < total; i += step) {
        const QueueElem e = queue_elem(i, Q);
        const uint32_t cnt = e.which ? s_rs[e.k] : s_rq[e.k];
        uint4 v = zero4;
        if (e.p < cnt) v = src[i];
        reinterpret_cast<uint4*>(qslots(S, c * N + e.k, (int)e.which) +
                                 e.p * qstride(S, (int)e.which))[e.half] = v;
      }
    }

    {                                                    // per node the raw arena
      const uint4* const src = reinterpret_cast<const uint4*>(rec + Y.off[4]);
      const uint32_t entries = N * A, chunks = (entries + 1) >> 1;
      uint2* const ar = arena_of(S, c * N);
      const bool dst16 = arena_even(S, c, 0);
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
  const uint32_t splits = pack_splits(Y.stride);
  hipLaunchKernelGGL(scatter_kernel, pack_grid(n, splits), dim3(PACK_BLOCK), 0, st, S,
                     static_cast<const uint2*>(pairs), n, splits, Y,
                     static_cast<const uint8_t*>(in));
  return hipGetLastError();
}

}  // namespace rs
