// summary.hpp — from per-lane accumulators to one summary struct (gfx950), the part the state
// census and the log audit share on the device. A pass's waves reduce their lanes, the workgroup
// its waves through LDS, and workgroup b leaves partial record b in the shard's scratch array; a
// second, one-workgroup kernel folds the partials. Every field is an integer sum, minimum or
// maximum (summary_host.hpp), the only synchronisation between workgroups is the launch boundary
// and there is no atomic anywhere: the result depends on no arrival or dispatch order. A further
// summarising query brings its struct's summary_fields, its pass and a SummaryLayout.
#pragma once
#include "compact.hpp"
#include "summary_host.hpp"

namespace rs {

static_assert(SUMMARY_BLOCK == COMPACT_BLOCK, "the selections' chunks are counted in these blocks");
constexpr uint32_t SUMMARY_FOLD_BLOCK = 1024;        // the folding workgroup: 16 waves

// The selections' predicate over a cluster's class word.
__device__ __forceinline__ bool class_match(uint32_t cls, uint32_t any, uint32_t all, uint32_t none) {
  return (any == 0 || (cls & any) != 0) && (cls & all) == all && (cls & none) == 0;
}

// Wave reduction of a lane's value of field f (all 64 lanes active), uniform result.
template <class T>
__device__ __forceinline__ uint64_t wave_fold(uint32_t f, uint64_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d);
    x = summary_fold<T>(f, x, (uint64_t)hi << 32 | lo);
  }
  return x;
}

// The end of a pass: part[blockIdx.x] = the workgroup's record. Fields 0 .. NC are sums a lane
// holds as 32-bit counts (cnt; a wave's sum must stay below 2^32), field NC + i is x[i]. Every
// thread of the workgroup calls it; constant indices only, so both arrays live in registers.
template <class T, uint32_t NC>
__device__ __forceinline__ void summary_block_store(const uint32_t* cnt, const uint64_t* x,
                                                    unsigned long long* __restrict__ part) {
  constexpr uint32_t F = summary_F<T>;
  static_assert(NC <= F && summary_sums<T>(NC), "the 32-bit counts are sums");
  __shared__ unsigned long long rec[SUMMARY_WAVES][F];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t f = 0; f < NC; ++f) {
    const uint32_t s = wave_sum(cnt[f]);
    if (lane == 0) rec[wv][f] = s;
  }
  uint64_t folded[F - NC];
#pragma unroll
  for (uint32_t f = NC; f < F; ++f) folded[f - NC] = wave_fold<T>(f, x[f - NC]);
  if (lane == 0) {                                   // one test for all of them
#pragma unroll
    for (uint32_t f = NC; f < F; ++f) rec[wv][f] = folded[f - NC];
  }
  __syncthreads();
  if (threadIdx.x < F) {
    const uint32_t f = threadIdx.x;
    uint64_t y = rec[0][f];
#pragma unroll
    for (uint32_t w = 1; w < SUMMARY_WAVES; ++w) y = summary_fold<T>(f, y, rec[w][f]);
    part[(size_t)blockIdx.x * F + f] = y;
  }
}

// One workgroup: out[0 .. F) = the np partial records folded field by field.
template <class T>
__global__ void __launch_bounds__(SUMMARY_FOLD_BLOCK)
summary_fold_kernel(const unsigned long long* __restrict__ part, uint32_t np,
                    unsigned long long* __restrict__ out) {
  constexpr uint32_t F = summary_F<T>, ROWS = SUMMARY_FOLD_BLOCK / 64;
  __shared__ unsigned long long acc[ROWS][64];
  const uint32_t f = threadIdx.x & 63, row = threadIdx.x >> 6;
  uint64_t x = summary_unit<T>(f);
  if (f < F)
    for (uint32_t p = row; p < np; p += ROWS) x = summary_fold<T>(f, x, part[(size_t)p * F + f]);
  acc[row][f] = x;
  __syncthreads();
  if (threadIdx.x < F) {
    for (uint32_t r = 1; r < ROWS; ++r) x = summary_fold<T>(f, x, acc[r][f]);
    out[f] = x;
  }
}

// A pass of `grid` workgroups and the fold of its partials into the layout's result record.
// pass(grid, part): enqueue the pass; its workgroup b writes part[b] through summary_block_store.
// A grid the layout has no room for is refused before anything is enqueued.
template <class T, class Pass>
hipError_t launch_summary(const SummaryLayout& lay, unsigned long long* scratch, uint32_t grid,
                          hipStream_t st, Pass pass) {
  if (grid > lay.parts || lay.F != summary_F<T>) return hipErrorInvalidValue;
  pass(dim3(grid), scratch + lay.part(0));
  hipLaunchKernelGGL(summary_fold_kernel<T>, dim3(1), dim3(SUMMARY_FOLD_BLOCK), 0, st,
                     (const unsigned long long*)scratch, grid, scratch + lay.result());
  return hipGetLastError();
}

}  // namespace rs
