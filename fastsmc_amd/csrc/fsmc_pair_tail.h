// fsmc_pair_tail.h -- the tail probabilities of fsmc_pair_cdf.h reduced over pairs and over bins of sites
// (fsmc_decode_pair_tail_summaries), without the [pairs][S] tail rows leaving the device.
//
// tail[j][i][t] is what pair_cdf_kernel writes for the cut c = tail_states[j]: the fp32 running sum cdf[c-1] of pair i's
// normalised posterior at site t (fsmc_pair_cdf.h).  Per slice of groups pair_cdf_kernel leaves these as rows,
// rows[cut][pair of slice][S]; the two kernels here reduce them:
//   - tail_sum[j][t], fp64: acc = acc + (double)tail[j][i][t] for i = 0, 1, ... in work-list order, one fp64 add a pair,
//     starting from the accumulator and going back to it, so slices, calls and flushes continue one chain
//     (pair_tail_sum_kernel).  The rows hold the slice's pairs only: a lane beyond a group's n_pairs has no row and adds
//     nothing.  One wave owns a cut and a block of 64 sites, lane = site; it walks the rows in pair order with
//     kPairTailBlock row loads (256 contiguous bytes each) in flight, the adds stay in pair order.
//   - bin_tail_mean[j][i][b], fp32: the mean of tail[j][i][t] over bin b = [e[b], e[b+1]) in the defined fp64 order of
//     bin_mean (fsmc_pair_bins.h): 64 slots starting at +0.0, slot s adds (double)tail for t = e[b] + s, + 64, ...
//     ascending, then the tree a[s] = a[s] + a[s + stride] for stride = 32 ... 1, then (float)(a[0] / (double)n).
//     pairBinsSum of fsmc_pair_bins.h is that sum, called as it is.
//   - bin_tail_length[j][i][b], fp32: the same slots and the same tree over (double)tail[j][i][t] * (double)w[t], the
//     result (float)a[0], no divide.  The fp64 product of two floats is exact (24 + 24 significant bits, and the exponent
//     range of a double holds every product of two finite floats, subnormal ones included), so whether the compiler fuses
//     the multiply into the add or not cannot change a bit: an fma rounds the exact product plus the addend once, and
//     the unfused pair rounds the same exact product plus the addend once.
//   (pair_tail_bins_kernel: one wave per (cut, pair, bin) cell, lane = slot, the tree through __shfl_down.)
// No atomics, no LDS memory, no scratch.  Sites at or beyond S, sites outside [e[0], e[B]) and rows beyond the slice's
// pairs are never read.
#pragma once

#include <hip/hip_runtime.h>

#include "fsmc_kernels.h"
#include "fsmc_pair_bins.h"

namespace fsmc
{

struct PairTailParams {
  const float* rows;  // [nTail][rowsPerOut][S]: the slice's tail rows (pair_cdf_kernel's)
  size_t rowsPerOut;  // pairs of the largest slice
  int n;              // pairs of this slice
  int S;
  int nTail;
  double* sum;          // [nTail][S] accumulator, or null
  const int* edges;     // [B + 1], strictly ascending, 0 <= edges[0], edges[B] <= S; null without bin outputs
  const float* weights; // [S], or null
  int B;
  // outputs, [nTail][rowsPerOut][B] each, or null
  float* binMean;
  float* binLength;
};

constexpr int kPairTailBlock = 8; // rows in flight together, a wave

// grid: (ceil(S / 64), nTail) workgroups of one wave
__global__ __launch_bounds__(kWave) void pair_tail_sum_kernel(const PairTailParams p)
{
  const int lane = (int)threadIdx.x;
  const int j = (int)blockIdx.y;
  const int t = (int)blockIdx.x * kWave + lane;
  if (t >= p.S) {
    return;
  }
  const size_t S = (size_t)p.S;
  const float* row = p.rows + (size_t)j * p.rowsPerOut * S + (size_t)t;
  double* const cell = p.sum + (size_t)j * S + (size_t)t;
  double acc = *cell;
  int i0 = 0;
  for (; i0 + kPairTailBlock <= p.n; i0 += kPairTailBlock) {
    float v[kPairTailBlock];
#pragma unroll
    for (int i = 0; i < kPairTailBlock; ++i) {
      v[i] = row[(size_t)i * S];
    }
#pragma unroll
    for (int i = 0; i < kPairTailBlock; ++i) {
      acc = acc + (double)v[i];
    }
    row += (size_t)kPairTailBlock * S;
  }
  for (; i0 < p.n; ++i0) {
    acc = acc + (double)*row;
    row += S;
  }
  *cell = acc;
}

// The defined fp64 sum of row[t] * w[t] over [lo, hi): pairBinsSum's slots and tree over the products; a[0] in lane 0.
__device__ __forceinline__ double pairTailWeightedSum(const float* __restrict__ row, const float* __restrict__ w, int lo,
                                                      int hi, int lane)
{
  double a = 0.0;
  for (int t0 = lo + lane; t0 < hi; t0 += kPairBinsBlock * kWave) {
    float v[kPairBinsBlock], u[kPairBinsBlock];
#pragma unroll
    for (int j = 0; j < kPairBinsBlock; ++j) {
      const int t = t0 + j * kWave;
      v[j] = t < hi ? row[t] : 0.f;
      u[j] = t < hi ? w[t] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kPairBinsBlock; ++j) {
      if (t0 + j * kWave < hi) {
        a = a + (double)v[j] * (double)u[j];
      }
    }
  }
#pragma unroll
  for (int stride = kWave / 2; stride >= 1; stride >>= 1) {
    a = a + __shfl_down(a, stride, kWave);
  }
  return a;
}

// grid: (any number, nTail) workgroups of kPairBinsThreads; within a cut, wave w of the W waves of a grid row takes cells
// w, w + W, ... of the slice's n * B, cell = pair * B + bin, advanced as in pair_bins_kernel.
__global__ __launch_bounds__(kPairBinsThreads) void pair_tail_bins_kernel(const PairTailParams p)
{
  const int lane = (int)threadIdx.x & (kWave - 1);
  const unsigned wavesPerBlock = kPairBinsThreads / kWave;
  const unsigned w = __builtin_amdgcn_readfirstlane(blockIdx.x * wavesPerBlock + threadIdx.x / kWave);
  const unsigned W = gridDim.x * wavesPerBlock;
  const unsigned B = (unsigned)p.B;
  const size_t out0 = (size_t)blockIdx.y * p.rowsPerOut; // first row of the cut, in the rows and in the outputs
  const int stepPair = (int)(W / B), stepBin = (int)(W % B);
  int pair = (int)(w / B), bin = (int)(w % B);
  while (pair < p.n) {
    const int lo = p.edges[bin], hi = p.edges[bin + 1];
    const float* row = p.rows + (out0 + (size_t)pair) * (size_t)p.S;
    const size_t cell = (out0 + (size_t)pair) * B + (size_t)bin;
    if (p.binMean) {
      const double a = pairBinsSum(row, lo, hi, lane);
      if (lane == 0) {
        p.binMean[cell] = (float)(a / (double)(hi - lo));
      }
    }
    if (p.binLength) {
      const double a = pairTailWeightedSum(row, p.weights, lo, hi, lane);
      if (lane == 0) {
        p.binLength[cell] = (float)a;
      }
    }
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
