// fsmc_pair_bins.h -- per pair, summaries of the posterior mean / MAP rows over bins of sites (fsmc_decode_pair_bins):
// the counterpart of fsmc_pair_minima.h, which reduces over pairs per site.
//
// Bin b of the edges e[0] < e[1] < ... < e[B] is sites [e[b], e[b+1]), n = e[b+1] - e[b] of them.  The per-pair
// consumers of the decode kernels leave a slice of the work list as rows, stage[pair of slice][site];
// pair_bins_kernel reduces them to [pair of slice][B] per output:
//   - bin_mean: a mean in a DEFINED fp64 order.  Slot j (0 <= j < 64) starts at +0.0 and adds (double)mean[t] for
//     t = e[b] + j, e[b] + j + 64, ... below e[b+1], ascending; then for stride = 32, 16, 8, 4, 2, 1:
//     a[j] = a[j] + a[j + stride] for j < stride; the result is (float)(a[0] / (double)n), one fp64 divide and one
//     round-to-nearest conversion.  A slot beyond a narrow bin holds +0.0, an exact identity of these sums (no slot is
//     ever -0.0: it starts at +0.0), so the order does not depend on how bins are mapped to waves.
//   - bin_min_mean / bin_argmin_mean, bin_min_map / bin_argmin_map: the smallest value of the bin under `<` and the
//     LOWEST absolute site index that has it: numpy's argmin on the slice.  Lane-strided partials are no contiguous
//     ranges, so the compare carries the site: `v < best`, or `v == best` and `site < arg`.  A NaN in the bin wins,
//     lowest site first, as in numpy (the decode writes no NaN: this rule is stated, no test reaches it).
// One wave per (pair, bin) cell, lane = slot, the waves of the launch stride over the slice's n * B cells.  Lane j walks
// sites e[b] + j + 64 r with kPairBinsBlock loads in flight (a row read is 256 contiguous bytes, unaligned when e[b] is
// no multiple of 64); the tree runs through __shfl_down (a double is two 32-bit moves), no LDS memory, no atomics, no
// value-and-index keys packed into integers (an integer key orders +-0 and NaN differently from `<`).  Lanes beyond a
// bin read nothing, sites beyond e[B] <= S and rows beyond the slice's pairs are never read.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "fsmc_kernels.h"

namespace fsmc
{

struct PairBinsParams {
  const float* mean; // [n][S]: the slice's posterior means, or null
  const int* map;    // [n][S]: the slice's MAP states, or null
  const int* edges;  // [B + 1], strictly ascending, 0 <= edges[0], edges[B] <= S
  int n;             // pairs of the slice
  int S;
  int B;
  // outputs, [n][B] each, or null
  float* binMean;
  float* binMinMean;
  int* binArgMean;
  int* binMinMap;
  int* binArgMap;
};

constexpr int kPairBinsBlock = 4;   // strides of 64 sites in flight together, per output
constexpr int kPairBinsThreads = 256; // four waves a workgroup, each on cells of its own

// Does (v, t) come before (best, arg)?  The order of the header: smaller first, of equal values the lower site, a NaN
// before everything that is not one.  `arg` == INT_MAX with +inf / INT_MAX is "nothing yet": any real site precedes it.
__device__ __forceinline__ bool pairBinsBefore(float v, int t, float best, int arg)
{
  const bool vNan = v != v, bestNan = best != best;
  if (vNan || bestNan) {
    return vNan && (!bestNan || t < arg);
  }
  return v < best || (v == best && t < arg);
}

__device__ __forceinline__ bool pairBinsBefore(int v, int t, int best, int arg)
{
  return v < best || (v == best && t < arg);
}

// Lane's walk over its sites of [lo, hi) of `row` and the tree over the 64 lanes: (best, arg) of the bin in lane 0.
template <typename T>
__device__ __forceinline__ void pairBinsMin(const T* __restrict__ row, int lo, int hi, int lane, T nothing, T& best,
                                            int& arg)
{
  best = nothing;
  arg = INT_MAX;
  for (int t0 = lo + lane; t0 < hi; t0 += kPairBinsBlock * kWave) {
    T v[kPairBinsBlock];
#pragma unroll
    for (int j = 0; j < kPairBinsBlock; ++j) {
      const int t = t0 + j * kWave;
      v[j] = t < hi ? row[t] : nothing;
    }
#pragma unroll
    for (int j = 0; j < kPairBinsBlock; ++j) {
      const int t = t0 + j * kWave;
      if (t < hi && pairBinsBefore(v[j], t, best, arg)) {
        best = v[j];
        arg = t;
      }
    }
  }
#pragma unroll
  for (int stride = kWave / 2; stride >= 1; stride >>= 1) {
    const T ov = __shfl_down(best, stride, kWave);
    const int oa = __shfl_down(arg, stride, kWave);
    if (pairBinsBefore(ov, oa, best, arg)) {
      best = ov;
      arg = oa;
    }
  }
}

// The defined fp64 sum of row[lo, hi) (see the header): a[0] in lane 0.
__device__ __forceinline__ double pairBinsSum(const float* __restrict__ row, int lo, int hi, int lane)
{
  double a = 0.0;
  for (int t0 = lo + lane; t0 < hi; t0 += kPairBinsBlock * kWave) {
    float v[kPairBinsBlock];
#pragma unroll
    for (int j = 0; j < kPairBinsBlock; ++j) {
      const int t = t0 + j * kWave;
      v[j] = t < hi ? row[t] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kPairBinsBlock; ++j) {
      if (t0 + j * kWave < hi) {
        a = a + (double)v[j];
      }
    }
  }
#pragma unroll
  for (int stride = kWave / 2; stride >= 1; stride >>= 1) {
    // (lanes j >= stride add what they get back, their own value included: nothing reads them again)
    a = a + __shfl_down(a, stride, kWave);
  }
  return a;
}

// grid: any number of workgroups of kPairBinsThreads; wave w of the launch's W waves takes cells w, w + W, ... of the
// slice's n * B, cell = pair * B + bin.  (pair, bin) advance by (W / B, W % B) with a carry: no division in the loop, no
// cell index beyond 32 bits.
__global__ __launch_bounds__(kPairBinsThreads) void pair_bins_kernel(const PairBinsParams p)
{
  const int lane = (int)threadIdx.x & (kWave - 1);
  const unsigned wavesPerBlock = kPairBinsThreads / kWave;
  const unsigned w = __builtin_amdgcn_readfirstlane(blockIdx.x * wavesPerBlock + threadIdx.x / kWave);
  const unsigned W = gridDim.x * wavesPerBlock;
  const unsigned B = (unsigned)p.B;
  const int stepPair = (int)(W / B), stepBin = (int)(W % B);
  int pair = (int)(w / B), bin = (int)(w % B);
  while (pair < p.n) {
    const int lo = p.edges[bin], hi = p.edges[bin + 1];
    const size_t cell = (size_t)pair * B + (size_t)bin;
    if (p.mean) {
      const float* row = p.mean + (size_t)pair * (size_t)p.S;
      if (p.binMean) {
        const double a = pairBinsSum(row, lo, hi, lane);
        if (lane == 0) {
          p.binMean[cell] = (float)(a / (double)(hi - lo));
        }
      }
      if (p.binMinMean) {
        float best;
        int arg;
        pairBinsMin<float>(row, lo, hi, lane, __builtin_inff(), best, arg);
        if (lane == 0) {
          p.binMinMean[cell] = best;
          p.binArgMean[cell] = arg;
        }
      }
    }
    if (p.map) {
      int best, arg;
      pairBinsMin<int>(p.map + (size_t)pair * (size_t)p.S, lo, hi, lane, INT_MAX, best, arg);
      if (lane == 0) {
        p.binMinMap[cell] = best;
        p.binArgMap[cell] = arg;
      }
    }
    // (n - pair can be smaller than stepPair: the sum below stays within int, n and W / B both do)
    if (p.n - pair <= stepPair) {
      break;
    }
    pair += stepPair;
    bin += stepBin;
    if (bin >= (int)B) {
      bin -= (int)B;
      ++pair;
    }
  }
}

} // namespace fsmc
