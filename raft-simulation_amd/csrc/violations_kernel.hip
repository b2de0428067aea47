// violations_kernel.hip — the query over a shard's violation records (DevSim::viol, device.hpp):
// an order-preserving stream compaction for gfx950, and the kernel that clears the records.
//
// A record matches when one of the kinds asked for has a nonzero count and its first tick lies in
// [t_lo, t_hi). The matching clusters leave as raft_violation_t in ascending cluster order, and
// their number is reported whatever the caller's capacity: a search over a million clusters copies
// the few dozen records it asks for to the host, not 16 B per cluster.
//
// Three launches on the shard's stream: every workgroup counts the matches of its own chunk of
// VIOL_CHUNK consecutive clusters (ballot + popcount per wave, the waves' sums through LDS), one
// workgroup turns the chunk counts into exclusive offsets and the total, and the workgroups pass
// over their chunks again and scatter (the lane's rank in its wave from mbcnt of the ballot, the
// waves' offsets from an LDS scan). A single pass with decoupled look-back would read the records
// once instead of twice, but its workgroups spin on their predecessors' flags, which rests on the
// order in which workgroups are dispatched; here a launch boundary is the only synchronisation
// between workgroups, the records are 16 B per cluster (16 MB at a million clusters, a few
// microseconds of HBM time per pass), and the output depends on no arrival order: no atomics at
// all, plain vector loads and stores, bitwise reproducible.
#include "device.hpp"

namespace rs {

constexpr uint32_t VIOL_BLOCK = 256;                 // four waves
constexpr uint32_t VIOL_WAVES = VIOL_BLOCK / 64;
constexpr uint32_t VIOL_ROUNDS = 8;                  // records per thread
constexpr uint32_t VIOL_CHUNK = VIOL_BLOCK * VIOL_ROUNDS;

__host__ __device__ inline uint32_t viol_chunks(uint32_t C) {
  return (C + VIOL_CHUNK - 1) / VIOL_CHUNK;
}

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

// Pass 1: cnt[b] = matches among clusters [b * VIOL_CHUNK, (b + 1) * VIOL_CHUNK) below C.
__global__ void __launch_bounds__(VIOL_BLOCK)
viol_count_kernel(const uint4* __restrict__ rec, uint32_t C, uint32_t kinds, uint64_t t_lo,
                  uint64_t t_hi, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t wsum[VIOL_WAVES];
  const uint32_t base = blockIdx.x * VIOL_CHUNK;
  uint32_t n = 0;                                    // the wave's matches (uniform)
#pragma unroll
  for (uint32_t i = 0; i < VIOL_ROUNDS; ++i) {
    const uint32_t c = base + i * VIOL_BLOCK + threadIdx.x;
    const bool m = c < C && viol_match(rec[c], kinds, t_lo, t_hi);
    n += (uint32_t)__popcll(__ballot(m));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t w = 0; w < VIOL_WAVES; ++w) s += wsum[w];
    cnt[blockIdx.x] = s;
  }
}

// Pass 2 (one workgroup): cnt[0 .. nb) becomes its exclusive prefix sum, cnt[nb] the total.
__global__ void __launch_bounds__(VIOL_BLOCK)
viol_scan_kernel(uint32_t* cnt, uint32_t nb) {
  __shared__ uint32_t wsum[VIOL_WAVES];
  __shared__ uint32_t carry_s;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < nb; b0 += VIOL_BLOCK) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nb ? cnt[i] : 0u;
    uint32_t x = v;                                  // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)x, d);
      if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint32_t off = carry_s, tile = 0;
#pragma unroll
    for (uint32_t w = 0; w < VIOL_WAVES; ++w) {
      off += w < wv ? wsum[w] : 0u;
      tile += wsum[w];
    }
    if (i < nb) cnt[i] = off + x - v;
    __syncthreads();                                 // every thread has read carry_s and wsum
    if (threadIdx.x == 0) carry_s += tile;
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[nb] = carry_s;
}

// Pass 3: the matches of chunk b go to out[off[b] ...] in cluster order, as far as cap reaches.
// out is [cap] records of six words (raft_violation_t), written as three 8-byte stores.
__global__ void __launch_bounds__(VIOL_BLOCK)
viol_scatter_kernel(const uint4* __restrict__ rec, uint32_t C, uint32_t kinds, uint64_t t_lo,
                    uint64_t t_hi, const uint32_t* __restrict__ off, uint2* __restrict__ out,
                    uint32_t cap) {
  static_assert(sizeof(raft_violation_t) == 24, "raft_violation_t is six words");
  __shared__ uint32_t wsum[2][VIOL_WAVES];           // alternate: one barrier per round
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * VIOL_CHUNK;
  uint32_t pos = off[blockIdx.x];                    // the round's first output slot (uniform)
  if (pos >= cap) return;                            // the whole chunk lies past the capacity
  for (uint32_t i = 0; i < VIOL_ROUNDS; ++i) {
    const uint32_t c = base + i * VIOL_BLOCK + threadIdx.x;
    uint4 r = make_uint4(INF, 0, 0, 0);
    if (c < C) r = rec[c];
    const bool m = c < C && viol_match(r, kinds, t_lo, t_hi);
    const uint64_t b = __ballot(m);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 0) wsum[i & 1][wv] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t woff = 0, tile = 0;
#pragma unroll
    for (uint32_t w = 0; w < VIOL_WAVES; ++w) {
      const uint32_t s = wsum[i & 1][w];
      woff += w < wv ? s : 0u;
      tile += s;
    }
    const uint32_t o = pos + woff + rank;
    if (m && o < cap) {
      uint2* const p = out + (size_t)o * 3;
      p[0] = make_uint2(c, r.x);
      p[1] = make_uint2(r.y, r.z);
      p[2] = make_uint2(r.w, viol_kinds(r));
    }
    pos += tile;
  }
}

hipError_t launch_viol_clear(const DevSim& S, hipStream_t st) {
  hipLaunchKernelGGL(viol_clear_kernel, dim3((S.C + VIOL_BLOCK - 1) / VIOL_BLOCK),
                     dim3(VIOL_BLOCK), 0, st, reinterpret_cast<uint4*>(S.viol), S.C);
  return hipGetLastError();
}

// Words of the scratch array launch_viol_query needs for a shard of C clusters.
size_t viol_scratch_words(uint32_t C) { return (size_t)viol_chunks(C) + 1; }

// The query over shard S: scratch[viol_chunks(C)] receives the total, out (cap records; may be
// null when cap is 0) the first min(total, cap) matches with shard-local cluster indices.
hipError_t launch_viol_query(const DevSim& S, uint32_t kinds, uint64_t t_lo, uint64_t t_hi,
                             uint32_t* scratch, void* out, uint32_t cap, hipStream_t st) {
  const uint32_t nb = viol_chunks(S.C);
  const uint4* rec = reinterpret_cast<const uint4*>(S.viol);
  hipLaunchKernelGGL(viol_count_kernel, dim3(nb), dim3(VIOL_BLOCK), 0, st, rec, S.C, kinds, t_lo,
                     t_hi, scratch);
  hipLaunchKernelGGL(viol_scan_kernel, dim3(1), dim3(VIOL_BLOCK), 0, st, scratch, nb);
  if (cap)
    hipLaunchKernelGGL(viol_scatter_kernel, dim3(nb), dim3(VIOL_BLOCK), 0, st, rec, S.C, kinds,
                       t_lo, t_hi, (const uint32_t*)scratch, static_cast<uint2*>(out), cap);
  return hipGetLastError();
}

}  // namespace rs
