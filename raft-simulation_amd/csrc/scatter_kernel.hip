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
//
// The unit's second state writer, clone_kernel (below), is this kernel fed by gather_kernel's reads
// instead of a record: cluster to cluster on the device ("Cluster clones").
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

// clone_kernel — cluster state copied on the device (include/raftsim.h, "Cluster clones"): cluster
// pairs[r].y of the shard Src becomes cluster pairs[r].x of the shard T, and the target is left bit
// for bit as scatter_kernel leaves it from the record gather_kernel packs of the source, without
// that record: one read and one write of the state. Src and T may be one shard; the host refuses a
// cluster that is both read and written, so no pair's source is any pair's target. The launch shape
// and a workgroup's share of a pair are the two kernels' (pack.hpp), the stride that of the record
// with every part a scatter needs. Per pair:
//   - the hot block a word per lane: the cluster's five words, words 5-7 and the pad zero; a node
//     field through hot_clone (node_codec.hpp: hot_field of node_word, so an owed draw is resolved
//     with the source's global id and Src's keys, and FL_DRAW is clear); a queue word through
//     queue_field from the source rings' counts and the arrivals of their first and last messages,
//     read from the rings;
//   - the queues 16 bytes per lane: message p from source slot (head + p) mod Q to target slot p,
//     zero at and past the count;
//   - the arenas two entries per lane, each side with 16-byte accesses where it can and 8-byte ones
//     where it cannot (arena_access_bytes; an odd arena_cap gives all four combinations);
//   - commit_count and the commit-stream rings a word per lane: slot s from slot s where it holds
//     a kept value, else zero (stream_slot_kept has the derivation).
// What a pair's parts need per node (QMETA, the rings' end arrivals, commit_count) is read once
// per pair into LDS.
__global__ void __launch_bounds__(PACK_BLOCK)
clone_kernel(const DevSim T, const DevSim Src, const uint2* __restrict__ pairs, uint32_t n,
             uint32_t splits) {
  __shared__ uint32_t s_qm[RAFT_MAX_NODES], s_cc[RAFT_MAX_NODES], s_arr[2][RAFT_MAX_NODES],
      s_tail[2][RAFT_MAX_NODES];
  const uint32_t N = T.N, Q = T.Q, A = T.A, SC = T.SC, HB = T.HB, tid = threadIdx.x;
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  const DrawKeys dk = {Src.el_base, Src.el_span, Src.key0, Src.key1};
  const PackLanes ln(splits);
  const uint32_t first = ln.first, step = ln.step;
  for (uint32_t r = ln.r0; r < n; r += ln.rstep) {
    const uint32_t ct = pairs[r].x, cs = pairs[r].y;
    if (ct >= T.C || cs >= Src.C) continue;              // (the host refuses such a list)
    __syncthreads();                                     // the pair before is done with the LDS
    if (tid < N) {
      const uint32_t qm = hot_node(Src, cs, tid)[HF_QMETA * N], cc = Src.ccount[(size_t)cs * N + tid];
      s_qm[tid] = qm;
      s_cc[tid] = cc;
      if (ln.sp == 0) T.ccount[(size_t)ct * N + tid] = cc;
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        // a queue never exceeds inbox_cap; the clamp keeps a corrupt word inside the ring
        const uint32_t head = which ? qm_res_head(qm) : qm_req_head(qm);
        const uint32_t cnt = min(which ? qm_res_cnt(qm) : qm_req_cnt(qm), Q);
        const uint32_t* const ring = qslots(Src, cs * N + tid, which);
        const size_t qs = qstride(Src, which);
        s_arr[which][tid] = cnt ? ring[(head % Q) * qs] : 0u;
        s_tail[which][tid] = cnt ? ring[((head + cnt - 1) % Q) * qs] : 0u;
      }
    }
    __syncthreads();

    {                                                    // the hot block, a word per lane
      uint32_t* const hb = hot_cl(T, ct);
      const uint32_t* const cl = hot_cl(Src, cs);
      for (uint32_t w = first; w < HB; w += step) {
        uint32_t v = 0;                                  // words 5-7 (CL_CTERM, CL_CERT) and the pad
        if (w <= CL_CLIENT_COUNT) {
          v = cl[w];
        } else if (w >= HOT_CW) {
          const uint32_t f = (w - HOT_CW) / N, k = (w - HOT_CW) - f * N;
          if (hf_is_queue(f)) {
            const uint32_t qm = s_qm[k];
            v = queue_field(f, ring_words(0, min(qm_req_cnt(qm), Q), s_arr[0][k], s_tail[0][k]),
                            ring_words(1, min(qm_res_cnt(qm), Q), s_arr[1][k], s_tail[1][k]));
          } else if (f < hot_fields(N)) {
            v = hot_clone(hot_node(Src, cs, k), N, f, Src.goff + cs, k, dk);
          }
        }
        hb[w] = v;
      }
    }

    {                                                    // per node REQ then RES, head first
      const uint32_t total = N * 2 * Q * 2;              // halves of messages
      for (uint32_t i = first; i < total; i += step) {
        const QueueElem e = queue_elem(i, Q);
        const uint32_t qm = s_qm[e.k];
        const uint32_t head = e.which ? qm_res_head(qm) : qm_req_head(qm);
        const uint32_t cnt = min(e.which ? qm_res_cnt(qm) : qm_req_cnt(qm), Q);
        uint4 v = zero4;
        if (e.p < cnt) {
          const uint32_t slot = (head + e.p) % Q;
          v = reinterpret_cast<const uint4*>(qslots(Src, cs * N + e.k, (int)e.which) +
                                             slot * qstride(Src, (int)e.which))[e.half];
        }
        reinterpret_cast<uint4*>(qslots(T, ct * N + e.k, (int)e.which) +
                                 e.p * qstride(T, (int)e.which))[e.half] = v;
      }
    }

    {                                                    // per node the raw arena
      const uint32_t entries = N * A, chunks = (entries + 1) >> 1;
      const uint2* const sa = arena_of(Src, cs * N);
      uint2* const ta = arena_of(T, ct * N);
      const uint64_t s0 = (uint64_t)cs * N * A, t0 = (uint64_t)ct * N * A;
      for (uint32_t i = first; i < chunks; i += step) {
        const uint32_t e = 2 * i;
        const bool both = e + 1 < entries;
        uint4 v;
        if (arena_access_bytes(s0, e, entries) == 16) {
          v = *reinterpret_cast<const uint4*>(sa + e);
        } else {
          const uint2 a = sa[e];
          const uint2 b = both ? sa[e + 1] : make_uint2(0, 0);
          v = make_uint4(a.x, a.y, b.x, b.y);
        }
        if (arena_access_bytes(t0, e, entries) == 16) {
          *reinterpret_cast<uint4*>(ta + e) = v;
        } else {
          ta[e] = make_uint2(v.x, v.y);
          if (both) ta[e + 1] = make_uint2(v.z, v.w);
        }
      }
    }

    if (SC) {                                            // per node the ring, slot to slot
      const uint32_t words = N * SC;
      for (uint32_t i = first; i < words; i += step) {
        const uint32_t k = i / SC, s = i - k * SC;
        T.stream[((size_t)ct * N + k) * SC + s] =
            stream_slot_kept(s, s_cc[k], SC) ? Src.stream[((size_t)cs * N + k) * SC + s] : 0u;
      }
    }
  }
}

// Make cluster pairs[i].x of T the state of cluster pairs[i].y of Src (device list, shard-local
// ids), n pairs. stride: that of the record a scatter needs (it sizes a pair's workgroups).
hipError_t launch_clone(const DevSim& T, const DevSim& Src, const void* pairs, uint32_t n,
                        uint64_t stride, hipStream_t st) {
  if (!n) return hipSuccess;
  const uint32_t splits = pack_splits(stride);
  hipLaunchKernelGGL(clone_kernel, pack_grid(n, splits), dim3(PACK_BLOCK), 0, st, T, Src,
                     static_cast<const uint2*>(pairs), n, splits);
  return hipGetLastError();
}

// Node restarts (include/raftsim.h, "Node restarts"; SIM_SPEC §4a): the unit's third state writer.
// A restart writes hot words only -- no queue slot, arena slot or stream slot moves -- so both
// kernels take the tick kernel's mapping instead of the packs': one lane per node, floor(64 / N)
// whole clusters per wave, and a store of field f is one run of N adjacent words per cluster (word
// HOT_CW + f * N + k), of which the lanes of the restarted nodes take part. Every word is
// hot_restart's (node_codec.hpp) of the node's words before it: a lane reads and writes its own
// node's words alone, field after field, and the one word it reads after writing another (the
// frontier, for the base) is one a restart keeps. The cluster's first lane zeroes words 5-7 (the
// unused word and the steady certificate, as scatter and clone leave them) of a cluster with a
// restarted node; words 0-4 (hwm, client cursor) stay.
__device__ __forceinline__ void restart_lane(const DevSim& S, uint32_t c, uint32_t k, bool node,
                                             bool head, uint32_t mode, uint32_t T) {
  const uint32_t N = S.N;
  if (node) {
    const DrawKeys dk = {S.el_base, S.el_span, S.key0, S.key1};
    uint32_t* const h = hot_node(S, c, k);
    const uint32_t F = hot_fields(N);
    for (uint32_t f = 0; f < F; ++f) h[f * N] = hot_restart(h, N, f, mode, T, S.goff + c, k, dk);
  }
  if (head) {
    uint32_t* const cl = hot_cl(S, c);
    cl[CL_CLIENT_COUNT + 1] = 0;
    cl[CL_CTERM] = 0;
    cl[CL_CERT] = 0;
  }
}

constexpr uint32_t RESTART_WAVES = PACK_BLOCK / 64;

// restart_kernel — the list form: node id j of cluster pairs[r].x of shard S is restarted where bit
// j of pairs[r].y is set. The waves stride over the list, floor(64 / N) pairs at a time.
__global__ void __launch_bounds__(PACK_BLOCK)
restart_kernel(const DevSim S, const uint2* __restrict__ pairs, uint32_t n, uint32_t mode,
               uint32_t T) {
  const uint32_t N = S.N, CPW = 64 / N, lane = threadIdx.x & 63;
  const uint32_t slot = lane / N, k = lane - slot * N;
  const uint32_t wave = blockIdx.x * RESTART_WAVES + (threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * RESTART_WAVES;
  if (slot >= CPW) return;                               // the wave's spare lanes
  for (uint64_t r = (uint64_t)wave * CPW + slot; r < n; r += (uint64_t)waves * CPW) {
    const uint2 p = pairs[r];
    if (p.x >= S.C) continue;                            // (the host refuses such a list)
    const uint32_t ids = p.y & ((2u << N) - 2);          // (... and a bit outside ids 1..N)
    restart_lane(S, p.x, k, (ids >> (k + 1)) & 1, k == 0 && ids, mode, T);
  }
}

// restart_where_kernel — the supervisor form: one pass over the hot blocks of shard S restarts every
// node whose fault code f has bit f set in fault_mask (bit 0: the running nodes). A wave reads the
// flags words of its clusters, a word per lane; only clusters with a matching node are written. The
// matches are counted per wave (the popcount of the ballot, a scalar) and added once per wave into
// the shard's counter *count, which the host zeroes before the launch and reads once after it.
__global__ void __launch_bounds__(PACK_BLOCK)
restart_where_kernel(const DevSim S, uint32_t fault_mask, uint32_t mode, uint32_t T,
                     uint32_t* __restrict__ count) {
  const uint32_t N = S.N, CPW = 64 / N, lane = threadIdx.x & 63;
  const uint32_t slot = lane / N, k = lane - slot * N, seg = (1u << N) - 1;
  const uint32_t wave = blockIdx.x * RESTART_WAVES + (threadIdx.x >> 6);
  const uint32_t waves = gridDim.x * RESTART_WAVES;
  const uint32_t groups = (S.C + CPW - 1) / CPW;         // C * N < 2^31: no overflow
  uint32_t total = 0;                                    // wave-uniform
  for (uint32_t g = wave; g < groups; g += waves) {
    const uint32_t c = g * CPW + slot;
    const bool act = slot < CPW && c < S.C;
    bool hit = false;
    if (act) hit = (fault_mask >> fl_fault(hot_node(S, c, k)[HF_FLAGS * N])) & 1;
    const uint64_t b = __ballot(hit);
    total += (uint32_t)__popcll(b);
    // slot * N <= 63, also on the wave's spare lanes
    restart_lane(S, c, k, hit, act && k == 0 && ((uint32_t)(b >> (slot * N)) & seg), mode, T);
  }
  if (lane == 0 && total) atomicAdd(count, total);
}

inline dim3 restart_grid(uint32_t clusters, uint32_t N) {
  const uint32_t CPW = 64 / N, waves = (clusters + CPW - 1) / CPW;
  return dim3(std::min((waves + RESTART_WAVES - 1) / RESTART_WAVES, PACK_MAX_GRID));
}

// Restart the nodes pairs[i].y (bit j: id j) of cluster pairs[i].x of S (device list, shard-local
// ids), n pairs, at tick T in mode `mode` (raft_restart_mode).
hipError_t launch_restart(const DevSim& S, const void* pairs, uint32_t n, uint32_t mode, uint32_t T,
                          hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(restart_kernel, restart_grid(n, S.N), dim3(PACK_BLOCK), 0, st, S,
                     static_cast<const uint2*>(pairs), n, mode, T);
  return hipGetLastError();
}

// Restart every node of S whose fault code is in fault_mask; *count (device, zeroed by the caller
// on the same stream) receives their number.
hipError_t launch_restart_where(const DevSim& S, uint32_t fault_mask, uint32_t mode, uint32_t T,
                                uint32_t* count, hipStream_t st) {
  hipLaunchKernelGGL(restart_where_kernel, restart_grid(S.C, S.N), dim3(PACK_BLOCK), 0, st, S,
                     fault_mask, mode, T, count);
  return hipGetLastError();
}

}  // namespace rs
