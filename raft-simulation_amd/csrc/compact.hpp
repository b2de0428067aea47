// compact.hpp — the order-preserving stream compaction behind the device-side queries (gfx950):
// the matching items of a shard leave as records in ascending cluster order, and their number is
// reported whatever the caller's capacity. A query over a million clusters copies the few dozen
// records it asks for to the host, not every cluster's.
//
// Three launches on the shard's stream: every workgroup counts the matches of its own chunk of
// consecutive clusters (ballot + popcount per wave, the waves' sums through LDS), one workgroup
// turns the chunk counts into exclusive offsets and the total, and the workgroups pass over their
// chunks again and scatter (the lane's rank in its wave from mbcnt of the ballot, the waves'
// offsets from an LDS scan). A single pass with decoupled look-back would read the items once
// instead of twice, but its workgroups spin on their predecessors' flags, which rests on the
// order in which workgroups are dispatched; here a launch boundary is the only synchronisation
// between workgroups, the items are small (16 B per cluster of violation records: 16 MB at a
// million clusters, a few microseconds of HBM time per pass), and the output depends on no arrival
// order: no atomics at all, plain vector loads and stores, bitwise reproducible.
//
// What is compacted is a "source", passed to the kernels by value:
//   static constexpr uint32_t ROUNDS      items per lane and chunk
//   uint32_t chunks() const               chunks of the shard (host)
//   Item load(chunk, round) const         the lane's item; every lane of the workgroup calls it, so
//                                         it may ballot and shuffle. Items rise with (chunk, round,
//                                         wave, lane).
//   bool match(const Item&) const         the lane's item is selected (at most one record per lane)
//   void gather(Item&) const              called by every lane of a wave in which some lane
//                                         matched, before the store: what a record needs from
//                                         other lanes
//   void store(const Item&, slot) const   write the record of a matching item at output slot `slot`
#pragma once
#include "device.hpp"

namespace rs {

constexpr uint32_t COMPACT_BLOCK = 256;              // four waves
constexpr uint32_t COMPACT_WAVES = COMPACT_BLOCK / 64;

// The scratch array of a compaction over nb chunks: the chunk counts (then offsets), then the total.
inline size_t compact_scratch_words(uint32_t nb) { return (size_t)nb + 1; }
inline const uint32_t* compact_total_ptr(const uint32_t* cnt, uint32_t nb) { return cnt + nb; }

// Pass 1: cnt[b] = matches of chunk b.
template <class Src>
__global__ void __launch_bounds__(COMPACT_BLOCK)
compact_count(const Src src, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t wsum[COMPACT_WAVES];
  uint32_t n = 0;                                    // the wave's matches (uniform)
  for (uint32_t i = 0; i < Src::ROUNDS; ++i) {
    const typename Src::Item it = src.load(blockIdx.x, i);
    n += (uint32_t)__popcll(__ballot(src.match(it)));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t w = 0; w < COMPACT_WAVES; ++w) s += wsum[w];
    cnt[blockIdx.x] = s;
  }
}

// Pass 2 (one workgroup): cnt[0 .. nb) becomes its exclusive prefix sum, cnt[nb] the total.
// static: the header is included by more than one file, each with its own copy of the kernel.
static __global__ void __launch_bounds__(COMPACT_BLOCK)
compact_scan(uint32_t* cnt, uint32_t nb) {
  __shared__ uint32_t wsum[COMPACT_WAVES];
  __shared__ uint32_t carry_s;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < nb; b0 += COMPACT_BLOCK) {
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
    for (uint32_t w = 0; w < COMPACT_WAVES; ++w) {
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

// Pass 3: the matches of chunk b go to output slots off[b] ... in item order, as far as cap reaches.
template <class Src>
__global__ void __launch_bounds__(COMPACT_BLOCK)
compact_scatter(const Src src, const uint32_t* __restrict__ off, uint32_t cap) {
  __shared__ uint32_t wsum[2][COMPACT_WAVES];        // alternate: one barrier per round
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t pos = off[blockIdx.x];                    // the round's first output slot (uniform)
  if (pos >= cap) return;                            // the whole chunk lies past the capacity
  for (uint32_t i = 0; i < Src::ROUNDS; ++i) {
    typename Src::Item it = src.load(blockIdx.x, i);
    const bool m = src.match(it);
    const uint64_t b = __ballot(m);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (b) src.gather(it);                           // wave-uniform
    if (lane == 0) wsum[i & 1][wv] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t woff = 0, tile = 0;
#pragma unroll
    for (uint32_t w = 0; w < COMPACT_WAVES; ++w) {
      const uint32_t s = wsum[i & 1][w];
      woff += w < wv ? s : 0u;
      tile += s;
    }
    const uint32_t o = pos + woff + rank;
    if (m && o < cap) src.store(it, o);
    pos += tile;
  }
}

// The compaction of src on stream st: *compact_total_ptr(cnt, src.chunks()) receives the total,
// the source's output (cap records; unused when cap is 0) the first min(total, cap) matches.
template <class Src>
hipError_t launch_compact(const Src& src, uint32_t* cnt, uint32_t cap, hipStream_t st) {
  const uint32_t nb = src.chunks();
  hipLaunchKernelGGL(compact_count<Src>, dim3(nb), dim3(COMPACT_BLOCK), 0, st, src, cnt);
  hipLaunchKernelGGL(compact_scan, dim3(1), dim3(COMPACT_BLOCK), 0, st, cnt, nb);
  if (cap)
    hipLaunchKernelGGL(compact_scatter<Src>, dim3(nb), dim3(COMPACT_BLOCK), 0, st, src,
                       (const uint32_t*)cnt, cap);
  return hipGetLastError();
}

}  // namespace rs
