// fsmc_pair_minima.h -- per site, the smallest posterior mean / MAP over the pairs and the first pair that has it
// (fsmc_decode_pair_minima).
//
// DecodePairsReturnStruct::finaliseCalculations (DecodePairsReturnStruct.hpp:105-118) walks the [pairs][sites] mean and
// MAP matrices column by column: pair 0 seeds (best, arg), a later pair replaces them only when `v < best`.  So ties keep
// the earlier pair, -0.f does not beat +0.f, and a NaN never replaces anything (a NaN seed stays).  The per-pair
// consumers of the decode kernels leave a slice of the work list as rows, stage[pair of slice][site]; two kernels
// reduce them to the same result without the rows ever leaving the device:
//   - pair_minima_kernel: lane = site, a wave = 64 consecutive sites, so a row read is 256 contiguous bytes.  The
//     slice's pairs are cut into contiguous ranges; a wave walks one range in ascending pair order with (best, arg) of
//     the mean and of the MAP in registers and the compare above, and writes one partial per range and site.  The range
//     that holds the chain's seed (pair 0 of a chain that starts in this call) starts from that pair's value whatever
//     it is; every other range starts from "nothing yet" (+inf / INT32_MAX, index -1), which no value it can meet is
//     smaller than in a way that would differ from the sequential loop: a value that is not `<` +inf is +inf or NaN,
//     and neither replaces anything in the loop either.
//   - pair_minima_combine_kernel: lane = site walks the ranges in ascending order, starting from the carried state
//     (or, for the chain's first slice, from the seed range's partial, taken as it is), and lets a partial replace the
//     state only when it is strictly smaller: the first of equal minima wins across ranges, slices and calls.
// No atomics, no value-and-index keys (an integer key orders +-0 and NaN differently from `<`).  Rows are indexed by
// pair of the slice, sites beyond S are never read or written: what a ragged group would leave beyond its pairs does
// not exist in the staging buffer and is not looked for.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "fsmc_kernels.h"

namespace fsmc
{

struct PairMinimaParams {
  const float* mean; // [n][S]: the slice's posterior means, or null
  const int* map;    // [n][S]: the slice's MAP states, or null
  int n;             // pairs of the slice
  int S;
  int rangeLen;      // pairs a range; ranges = ceil(n / rangeLen)
  int nRanges;
  int seeded;        // range 0 starts with the chain's seed (first slice of a call with pair_base == 0)
  int firstIndex;    // index reported for pair 0 of the slice: pair_base + the slice's first pair
  // partials, [nRanges][S] each
  float* partMinMean;
  int* partArgMean;
  int* partMinMap;
  int* partArgMap;
  // the carried state, [S] each (device copies of the caller's arrays)
  float* minMean;
  int* argMean;
  int* minMap;
  int* argMap;
};

constexpr int kPairMinimaBlock = 8; // rows in flight together, per output

// One output's walk over rows [lo, hi) of `rows` for site `site`: T = float (mean) or int (MAP).
template <typename T>
__device__ __forceinline__ void pairMinimaWalk(const T* __restrict__ rows, size_t S, int site, int lo, int hi,
                                               int firstIndex, T& best, int& arg)
{
  const T* src = rows + (size_t)lo * S + site;
  int i = lo;
  for (; i + kPairMinimaBlock <= hi; i += kPairMinimaBlock, src += (size_t)kPairMinimaBlock * S) {
    T v[kPairMinimaBlock];
#pragma unroll
    for (int j = 0; j < kPairMinimaBlock; ++j) {
      v[j] = src[(size_t)j * S];
    }
#pragma unroll
    for (int j = 0; j < kPairMinimaBlock; ++j) {
      if (v[j] < best) {
        best = v[j];
        arg = firstIndex + i + j;
      }
    }
  }
  for (; i < hi; ++i, src += S) {
    const T v = *src;
    if (v < best) {
      best = v;
      arg = firstIndex + i;
    }
  }
}

// grid: nRanges * ceil(S / 64) workgroups of one wave; workgroup b: range b / siteBlocks, sites 64 * (b % siteBlocks) ...
__global__ __launch_bounds__(kWave) void pair_minima_kernel(const PairMinimaParams p)
{
  const int siteBlocks = (p.S + kWave - 1) / kWave;
  const int r = (int)(blockIdx.x / (unsigned)siteBlocks);
  const int site = (int)(blockIdx.x % (unsigned)siteBlocks) * kWave + (int)threadIdx.x;
  if (site >= p.S || r >= p.nRanges) {
    return;
  }
  int lo = r * p.rangeLen;
  const int hi = p.n - lo < p.rangeLen ? p.n : lo + p.rangeLen;
  const bool seed = p.seeded && r == 0;
  const size_t cell = (size_t)r * p.S + site;
  if (p.mean) {
    float best = seed ? p.mean[site] : __builtin_inff();
    int arg = seed ? p.firstIndex : -1;
    pairMinimaWalk<float>(p.mean, (size_t)p.S, site, seed ? 1 : lo, hi, p.firstIndex, best, arg);
    p.partMinMean[cell] = best;
    p.partArgMean[cell] = arg;
  }
  if (p.map) {
    int best = seed ? p.map[site] : INT_MAX;
    int arg = seed ? p.firstIndex : -1;
    pairMinimaWalk<int>(p.map, (size_t)p.S, site, seed ? 1 : lo, hi, p.firstIndex, best, arg);
    p.partMinMap[cell] = best;
    p.partArgMap[cell] = arg;
  }
}

template <typename T>
__device__ __forceinline__ void pairMinimaCombine(const T* __restrict__ partMin, const int* __restrict__ partArg, int S,
                                                  int site, int nRanges, bool seeded, T* stateMin, int* stateArg)
{
  T best = seeded ? partMin[site] : stateMin[site];
  int arg = seeded ? partArg[site] : stateArg[site];
  for (int r = seeded ? 1 : 0; r < nRanges; ++r) {
    const T v = partMin[(size_t)r * S + site];
    const int a = partArg[(size_t)r * S + site];
    if (a >= 0 && v < best) { // (a range that met nothing it could take has index -1 and never wins)
      best = v;
      arg = a;
    }
  }
  stateMin[site] = best;
  stateArg[site] = arg;
}

// grid: ceil(S / blockDim.x) workgroups; thread = site
__global__ void pair_minima_combine_kernel(const PairMinimaParams p)
{
  const int site = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (site >= p.S) {
    return;
  }
  if (p.mean) {
    pairMinimaCombine<float>(p.partMinMean, p.partArgMean, p.S, site, p.nRanges, p.seeded != 0, p.minMean, p.argMean);
  }
  if (p.map) {
    pairMinimaCombine<int>(p.partMinMap, p.partArgMap, p.S, site, p.nRanges, p.seeded != 0, p.minMap, p.argMap);
  }
}

} // namespace fsmc
