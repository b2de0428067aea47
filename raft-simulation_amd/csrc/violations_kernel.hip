// violations_kernel.hip — the query over a shard's violation records (DevSim::viol, device.hpp) and
// the kernel that clears the records.
//
// A record matches when one of the kinds asked for has a nonzero count and its first tick lies in
// [t_lo, t_hi). The matching clusters leave as raft_violation_t in ascending cluster order, and
// their number is reported whatever the caller's capacity: the compaction of compact.hpp over the
// source below, one record (16 B) per lane and round.
#include "compact.hpp"

namespace rs {

constexpr uint32_t VIOL_BLOCK = 256;

// The kinds (raft_viol_kind bits) with a nonzero count in record r = (first_tick, counts).
__device__ __forceinline__ uint32_t viol_kinds(const uint4& r) {
  return (r.y ? 1u : 0u) | (r.z ? 2u : 0u) | (r.w ? 4u : 0u);
}
__device__ __forceinline__ bool viol_match(const uint4& r, uint32_t kinds, uint64_t t_lo,
                                           uint64_t t_hi) {
  return (viol_kinds(r) & kinds) != 0 && t_lo <= r.x && r.x < t_hi;
}

__global__ void __launch_bounds__(VIOL_BLOCK)
viol_clear_kernel(uint4* rec, uint32_t C) {
  const uint32_t c = blockIdx.x * VIOL_BLOCK + threadIdx.x;
  if (c < C) rec[c] = make_uint4(INF, 0, 0, 0);
}

// The compaction's source (compact.hpp): chunks of COMPACT_BLOCK * ROUNDS consecutive clusters, a
// lane's item the record of cluster chunk base + round * COMPACT_BLOCK + thread. out is [cap]
// records of six words (raft_violation_t), written as three 8-byte stores.
struct viol {
  static constexpr uint32_t ROUNDS = 8;
  struct Item {
    uint32_t c;
    uint4 r;
  };
  const uint4* __restrict__ rec;
  uint32_t C, kinds;
  uint64_t t_lo, t_hi;
  uint2* __restrict__ out;

  __host__ __device__ uint32_t chunks() const {
    return (C + COMPACT_BLOCK * ROUNDS - 1) / (COMPACT_BLOCK * ROUNDS);
  }
  __device__ __forceinline__ Item load(uint32_t b, uint32_t i) const {
    const uint32_t c = (b * ROUNDS + i) * COMPACT_BLOCK + threadIdx.x;
    return {c, c < C ? rec[c] : make_uint4(INF, 0, 0, 0)};
  }
  __device__ __forceinline__ bool match(const Item& it) const {
    return it.c < C && viol_match(it.r, kinds, t_lo, t_hi);
  }
  __device__ __forceinline__ void gather(Item&) const {}
  __device__ __forceinline__ void store(const Item& it, uint32_t o) const {
    static_assert(sizeof(raft_violation_t) == 24, "raft_violation_t is six words");
    uint2* const p = out + (size_t)o * 3;
    p[0] = make_uint2(it.c, it.r.x);
    p[1] = make_uint2(it.r.y, it.r.z);
    p[2] = make_uint2(it.r.w, viol_kinds(it.r));
  }
};

hipError_t launch_viol_clear(const DevSim& S, hipStream_t st) {
  hipLaunchKernelGGL(viol_clear_kernel, dim3((S.C + VIOL_BLOCK - 1) / VIOL_BLOCK),
                     dim3(VIOL_BLOCK), 0, st, reinterpret_cast<uint4*>(S.viol), S.C);
  return hipGetLastError();
}

// Words of the scratch array launch_viol_query needs for a shard of C clusters, and where in it the
// total stands.
size_t viol_scratch_words(uint32_t C) { return compact_scratch_words(viol{nullptr, C}.chunks()); }
const uint32_t* viol_total_ptr(const uint32_t* scratch, uint32_t C) {
  return compact_total_ptr(scratch, viol{nullptr, C}.chunks());
}

// The query over shard S: *viol_total_ptr receives the total, out (cap records; may be null when
// cap is 0) the first min(total, cap) matches with shard-local cluster indices.
hipError_t launch_viol_query(const DevSim& S, uint32_t kinds, uint64_t t_lo, uint64_t t_hi,
                             uint32_t* scratch, void* out, uint32_t cap, hipStream_t st) {
  const viol src = {reinterpret_cast<const uint4*>(S.viol), S.C, kinds, t_lo, t_hi,
                    static_cast<uint2*>(out)};
  return launch_compact(src, scratch, cap, st);
}

}  // namespace rs
