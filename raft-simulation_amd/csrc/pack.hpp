// pack.hpp — what gather_kernel.hip and scatter_kernel.hip share (cluster packs, include/raftsim.h):
// the launch shape, a workgroup's share of the list and of a record, and how the elements of the
// queue and arena parts are numbered. A record is a pack record, and for the scatter one (record,
// target) pair. clone_kernel (scatter_kernel.hip), which copies cluster to cluster without a record,
// takes the same shape over its (target, source) pairs, and from here the two decisions it shares
// with the host tests: the width of an arena access and which commit-stream slots a pack keeps.
#pragma once
#include <algorithm>

#include "node_codec.hpp"

namespace rs {

// `splits` workgroups of four waves per record, the groups of workgroups striding over the list. A
// record of a few KB has one workgroup; a 1.5-MB record (N = 9, 16,384-slot arenas), of which a
// 64-MiB scratch holds 45, has 46, since 45 workgroups would leave most of the chip idle.
constexpr uint32_t PACK_BLOCK = 256;
constexpr uint32_t PACK_MAX_GRID = 4096;       // records in flight
constexpr uint32_t PACK_SPLIT_BYTES = 32768;   // a workgroup's share of a record, at least
constexpr uint32_t PACK_MAX_SPLITS = 64;
inline uint32_t pack_splits(uint64_t stride) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(stride / PACK_SPLIT_BYTES, 1),
                                      PACK_MAX_SPLITS);
}
inline dim3 pack_grid(uint32_t n, uint32_t splits) {
  return dim3(std::min(n, PACK_MAX_GRID) * splits);
}

// A workgroup's place in that grid: the records r0, r0 + rstep, ... of the list, and of every part
// of a record, a flat array, its lanes' elements first, first + step, ... (workgroup sp of a record
// the sp-th PACK_BLOCK of every step), adjacent lanes on adjacent bytes of the record.
struct PackLanes {
  uint32_t sp, first, step, r0, rstep;
  __device__ explicit PackLanes(uint32_t splits)
      : sp(blockIdx.x % splits), first(sp * PACK_BLOCK + threadIdx.x), step(splits * PACK_BLOCK),
        r0(blockIdx.x / splits), rstep(gridDim.x / splits) {}
};

// Element i of a record's queues, 16 bytes: half `half` of message p of node k's ring `which` (per
// node REQ then RES, Q messages each).
struct QueueElem {
  uint32_t half, p, k, which;
};
__device__ __forceinline__ QueueElem queue_elem(uint32_t i, uint32_t Q) {
  const uint32_t m = i >> 1, ring = m / Q;
  return {i & 1, m - ring * Q, ring >> 1, ring & 1};
}

// Two neighbouring arena entries move as one 16-byte access where both exist and the first lies on
// an even slot of the shard's arenas (an odd arena_cap puts every other cluster's arenas on an odd
// one), else as 8-byte accesses. s: a slot counted from cluster c's first.
__device__ __forceinline__ bool arena_even(const DevSim& S, uint32_t c, uint32_t s) {
  return (((size_t)c * S.N * S.A + s) & 1) == 0;
}

// The same decision for a copy from arena to arena (clone_kernel), where either side may stand on
// an odd slot, taken for each side alone: the bytes of the access that moves entry e and, where it
// exists, entry e + 1 (e even) of the `entries` of a cluster whose first arena slot is slot0 of its
// shard's arenas (c * N * A; the arenas start on 16 bytes). 16 only where that side's entry e lies
// on an even slot, i.e. on 16 bytes, and entry e + 1 exists.
__host__ __device__ constexpr uint32_t arena_access_bytes(uint64_t slot0, uint32_t e,
                                                          uint32_t entries) {
  return ((slot0 + e) & 1) == 0 && e + 1 < entries ? 16u : 8u;
}

// Whether slot s of a node's commit-stream ring (SC slots, commit_count cc) holds one of the values
// a pack keeps, the newest kept = min(cc, SC). gather_kernel writes value p < kept of a record from
// slot (cc - kept + p) mod SC, and scatter_kernel writes into slot s the record's value
// p = (s - (cc - kept)) mod SC when p < kept, else 0. For that p the gather's slot is
// (cc - kept + p) mod SC = s: a scatter of a gather leaves slot s of the target with slot s of the
// source where p < kept, and with 0 elsewhere -- the ring is not rotated, only cleared outside the
// kept window.
__host__ __device__ constexpr bool stream_slot_kept(uint32_t s, uint32_t cc, uint32_t SC) {
  const uint32_t kept = cc < SC ? cc : SC;
  return (s + SC - (cc - kept) % SC) % SC < kept;
}

}  // namespace rs
