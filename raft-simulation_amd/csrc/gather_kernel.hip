// gather_kernel.hip — cluster packs (gfx950): the full canonical state of an arbitrary list of
// clusters, packed into one contiguous buffer of fixed-size records (include/raftsim.h, "Cluster
// packs"; the layout: raft_gather_layout_t). Reads state only.
//
// Mapping: `splits` workgroups of four waves per record, the groups of workgroups striding over the
// list of (cluster, output slot) pairs (pack.hpp: the launch shape and a workgroup's share, which
// scatter_kernel.hip uses too). The clusters come from anywhere in the shard, so nothing is shared
// between records; inside a record every part is a flat array whose elements the lanes of the
// record's workgroups take in order, adjacent lanes on adjacent bytes of the record:
//   - the node records are decoded word by word (34 words each, one dword per lane) by
//     node_codec.hpp's node_word, which raft_sim_read_nodes uses too; an owed timer draw is
//     resolved as every reader of the state resolves it;
//   - queues, logs and arenas move 16 bytes per lane: a message is two uint4 of a ring slot (rings
//     are 32-byte aligned), a log or arena chunk is two 8-byte entries. Two entries are one uint4
//     load where they are neighbours in the arena at an even slot, and two uint2 loads where the
//     log crosses the arena's end between them, where one of them lies past the log's end, or where
//     the source is only 8-byte aligned (an odd arena slot). Every store is one uint4;
//   - the commit-stream rings are linearised a word per lane.
// What a node's parts need of its hot words (counts, ring heads, the arena offset) is read once per
// record into LDS. A record's padding is written as zeros with the part before it, so the kernel
// writes every byte of a record and the scratch needs no clearing.
#include "pack.hpp"

namespace rs {

// Y.off[b]: byte offset of part bit b in a record, UINT64_MAX where the part is not asked for.
__global__ void __launch_bounds__(PACK_BLOCK)
gather_kernel(const DevSim S, const uint2* __restrict__ pairs, uint32_t n, uint32_t splits,
              const raft_gather_layout_t Y, uint8_t* __restrict__ out) {
  __shared__ uint32_t s_qm[RAFT_MAX_NODES], s_len[RAFT_MAX_NODES], s_off[RAFT_MAX_NODES],
      s_cc[RAFT_MAX_NODES];
  const uint32_t N = S.N, Q = S.Q, L = S.L, A = S.A, SC = S.SC, tid = threadIdx.x;
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  const DrawKeys dk = {S.el_base, S.el_span, S.key0, S.key1};
  const PackLanes ln(splits);
  const uint32_t first = ln.first, step = ln.step;
  for (uint32_t r = ln.r0; r < n; r += ln.rstep) {
    const uint32_t c = pairs[r].x;
    if (c >= S.C) continue;                              // (the host refuses such a list)
    uint8_t* const rec = out + (size_t)pairs[r].y * Y.stride;
    __syncthreads();                                     // the record before is done with the LDS
    if (tid < N) {
      const uint32_t* const h = hot_node(S, c, tid);
      s_qm[tid] = h[HF_QMETA * N];
      // a log never exceeds log_cap; the clamp keeps a corrupt word inside the part
      s_len[tid] = min(h[HF_LEN * N], L);
      s_off[tid] = h[hf_abase(N) * N] % A;
      s_cc[tid] = S.ccount[(size_t)c * N + tid];
    }
    __syncthreads();

    if (Y.off[0] != UINT64_MAX && first < 2) {             // raft_cluster_t, reserved words zero
      uint4 v = reinterpret_cast<const uint4*>(hot_cl(S, c))[first];
      if (first == 1) v.y = v.z = v.w = 0;               // word 4 is client_count
      reinterpret_cast<uint4*>(rec + Y.off[0])[first] = v;
    }

    if (Y.off[1] != UINT64_MAX) {                        // N raft_node_t, padded to 16 bytes
      uint32_t* const o = reinterpret_cast<uint32_t*>(rec + Y.off[1]);
      const uint32_t words = N * NODE_WORDS, padded = (words + 3) & ~3u;
      for (uint32_t i = first; i < padded; i += step) {
        const uint32_t k = i / NODE_WORDS, w = i - k * NODE_WORDS;
        o[i] = i < words ? node_word(hot_node(S, c, k), N, w, s_cc[k], S.goff + c, k, dk) : 0u;
      }
    }

    if (Y.off[2] != UINT64_MAX) {                        // per node REQ then RES, head first
      uint4* const o = reinterpret_cast<uint4*>(rec + Y.off[2]);
      const uint32_t total = N * 2 * Q * 2;              // halves of messages
      for (uint32_t i = first; i < total; i += step) {
        const QueueElem e = queue_elem(i, Q);
        const uint32_t qm = s_qm[e.k];
        const uint32_t head = e.which ? qm_res_head(qm) : qm_req_head(qm);
        const uint32_t cnt = min(e.which ? qm_res_cnt(qm) : qm_req_cnt(qm), Q);
        uint4 v = zero4;
        if (e.p < cnt) {
          const uint32_t slot = (head + e.p) % Q;
          v = reinterpret_cast<const uint4*>(qslots(S, c * N + e.k, (int)e.which) +
                                             slot * qstride(S, (int)e.which))[e.half];
        }
        o[i] = v;
      }
    }

    if (Y.off[3] != UINT64_MAX) {                        // per node log_cap entries, linearised
      uint4* const o = reinterpret_cast<uint4*>(rec + Y.off[3]);
      const uint32_t entries = N * L, chunks = (entries + 1) >> 1;
      const uint2* const ar = arena_of(S, c * N);
      for (uint32_t i = first; i < chunks; i += step) {
        uint2 e[2];
        uint32_t s[2];
        bool ok[2];
#pragma unroll
        for (uint32_t j = 0; j < 2; ++j) {
          const uint32_t x = 2 * i + j, k = min(x / L, N - 1), p = x - k * L;
          ok[j] = x < entries && p < s_len[k];
          uint32_t t = s_off[k] + p;                     // < 2 A
          t = t >= A ? t - A : t;
          s[j] = k * A + t;                              // < N A <= 9 * 2^24
          e[j] = make_uint2(0, 0);
        }
        if (ok[0] && ok[1] && s[1] == s[0] + 1 && arena_even(S, c, s[0])) {
          const uint4 v = *reinterpret_cast<const uint4*>(ar + s[0]);
          e[0] = make_uint2(v.x, v.y);
          e[1] = make_uint2(v.z, v.w);
        } else {
          if (ok[0]) e[0] = ar[s[0]];
          if (ok[1]) e[1] = ar[s[1]];
        }
        o[i] = make_uint4(e[0].x, e[0].y, e[1].x, e[1].y);
      }
    }

    if (Y.off[4] != UINT64_MAX) {                        // per node the raw arena
      uint4* const o = reinterpret_cast<uint4*>(rec + Y.off[4]);
      const uint32_t entries = N * A, chunks = (entries + 1) >> 1;
      const uint2* const ar = arena_of(S, c * N);
      const bool src16 = arena_even(S, c, 0);
      for (uint32_t i = first; i < chunks; i += step) {
        uint4 v;
        if (src16 && 2 * i + 1 < entries) {
          v = *reinterpret_cast<const uint4*>(ar + 2 * i);
        } else {
          const uint2 a = ar[2 * i];
          const uint2 b = 2 * i + 1 < entries ? ar[2 * i + 1] : make_uint2(0, 0);
          v = make_uint4(a.x, a.y, b.x, b.y);
        }
        o[i] = v;
      }
    }

    if (Y.off[5] != UINT64_MAX && SC) {                  // per node the newest values, oldest first
      uint32_t* const o = reinterpret_cast<uint32_t*>(rec + Y.off[5]);
      const uint32_t words = N * SC, padded = (words + 3) & ~3u;
      for (uint32_t i = first; i < padded; i += step) {
        uint32_t v = 0;
        if (i < words) {
          const uint32_t k = i / SC, p = i - k * SC, cc = s_cc[k], kept = min(cc, SC);
          if (p < kept) v = S.stream[((size_t)c * N + k) * SC + (cc - kept + p) % SC];
        }
        o[i] = v;
      }
    }
  }
}

// Pack the n clusters of `pairs` (device: x = shard-local cluster, y = output slot) into out, one
// record of layout Y at out + slot * Y.stride each.
hipError_t launch_gather(const DevSim& S, const void* pairs, uint32_t n,
                         const raft_gather_layout_t& Y, void* out, hipStream_t st) {
  if (!n) return hipSuccess;
  const uint32_t splits = pack_splits(Y.stride);
  hipLaunchKernelGGL(gather_kernel, pack_grid(n, splits), dim3(PACK_BLOCK), 0, st, S,
                     static_cast<const uint2*>(pairs), n, splits, Y, static_cast<uint8_t*>(out));
  return hipGetLastError();
}

}  // namespace rs
