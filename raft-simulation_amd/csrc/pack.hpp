// pack.hpp — what gather_kernel.hip and scatter_kernel.hip share (cluster packs, include/raftsim.h):
// the launch shape, a workgroup's share of the list and of a record, and how the elements of the
// queue and arena parts are numbered. A record is a pack record, and for the scatter one (record,
// target) pair.
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

}  // namespace rs
