// fsmc_pair_posteriors.h -- the per-pair posterior tables and their sum over pairs (fsmc_decode_pair_posteriors).
//
// HMM::writePerPairOutput (HMM.cpp:1378-1392) hands out, per pair, a [K][S] table of posterior * expectedCoalTimes[k]
// and adds the same values onto one [K][S] table, pair after pair.  The dump consumers of the decode kernels leave a
// slice of groups in the reference's batch layout, stage[group][site][k][lane]; this kernel turns that into the two
// outputs.  One wave owns state k and a block of 64 sites and walks the slice's groups in order:
//   - the 64 sites x 64 lanes tile of the group is read row by row (a row is the 64 lanes of one site: 256 contiguous
//     bytes), multiplied by expCoal[k] and put into LDS with a row stride of 65 floats, so that the column walk below
//     (lane = site, address lane * 65 + pair) touches 64 different banks, as the row writes do;
//   - pair by pair, lane = site reads its value back, stores it into the pair's row (64 consecutive floats a wave) and
//     adds it onto its running sum -- ((sum + v_0) + v_1) + ..., across the groups of the slice, and across slices and
//     calls because the running sum starts from the accumulator and goes back to it.
// The product passes through LDS before it is added, and the library is built with -ffp-contract=off: one fp32
// multiply, one fp32 add a value, the reference's operations.  Lanes beyond a group's n_pairs are never loaded, sites
// beyond S are masked in loads and stores.
#pragma once

#include <hip/hip_runtime.h>

#include "fsmc_kernels.h"

namespace fsmc
{

struct PairPostParams {
  const float* stage;       // [nGroups][S][K][64]: the dump of the slice
  const fsmc_group* groups; // the slice's groups (a window of the resident work list)
  int nGroups;
  int K, S;
  const float* expCoal; // [K]
  float* rows;          // [pairs of the slice][K][S], or null
  unsigned firstPair;   // first pair of the slice: row 0 of `rows`
  float* sum;           // [K][S] accumulator, or null
};

constexpr int kPairPostStride = kWave + 1;

__global__ __launch_bounds__(kWave) void pair_posteriors_kernel(const PairPostParams p)
{
  __shared__ float tile[kWave * kPairPostStride];
  const int lane = (int)threadIdx.x;
  const int k = (int)blockIdx.y;
  const int s0 = (int)blockIdx.x * kWave;
  const int nS = p.S - s0 < kWave ? p.S - s0 : kWave; // sites of this block (the last one may be short)
  const bool mine = lane < nS;
  const float e = p.expCoal[k];
  const size_t cell = (size_t)k * p.S + s0 + (mine ? lane : 0);
  float run = (p.sum && mine) ? p.sum[cell] : 0.f;
  const size_t siteStride = (size_t)p.K * kWave;
  const size_t groupFloats = siteStride * p.S;
  constexpr int kBlock = 8; // loads / LDS reads in flight together
  for (int g = 0; g < p.nGroups; ++g) {
    const int n = (int)p.groups[g].n_pairs;
    const float* src = p.stage + (size_t)g * groupFloats + ((size_t)s0 * p.K + k) * kWave + lane;
    for (int sb = 0; sb < nS; sb += kBlock) {
      float v[kBlock];
#pragma unroll
      for (int i = 0; i < kBlock; ++i) {
        v[i] = (sb + i < nS && lane < n) ? src[(size_t)(sb + i) * siteStride] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kBlock; ++i) {
        if (sb + i < nS) {
          tile[(sb + i) * kPairPostStride + lane] = v[i] * e;
        }
      }
    }
    __syncthreads();
    float* dst = p.rows ? p.rows + ((size_t)(p.groups[g].first_pair - p.firstPair) * p.K + k) * p.S + s0 + lane : nullptr;
    const size_t rowStride = (size_t)p.K * p.S;
    const float* col = tile + (mine ? lane : 0) * kPairPostStride;
    int i0 = 0;
    for (; i0 + kBlock <= n; i0 += kBlock) {
      float v[kBlock];
#pragma unroll
      for (int i = 0; i < kBlock; ++i) {
        v[i] = col[i0 + i];
      }
#pragma unroll
      for (int i = 0; i < kBlock; ++i) {
        run = run + v[i];
        if (dst && mine) {
          dst[(size_t)(i0 + i) * rowStride] = v[i];
        }
      }
    }
    for (; i0 < n; ++i0) {
      const float v = col[i0];
      run = run + v;
      if (dst && mine) {
        dst[(size_t)i0 * rowStride] = v;
      }
    }
    __syncthreads(); // the tile is free for the next group
  }
  if (p.sum && mine) {
    p.sum[cell] = run;
  }
}

} // namespace fsmc
