// fsmc_pair_cdf.h -- per pair and site, where the posterior mass lies (fsmc_decode_pair_cdf): tail probabilities at
// state cuts and quantile states, reduced from the dump of a slice of groups without the [K][S] tables leaving the device.
//
// For pair i and site t, post[k] is the normalised fp32 posterior of the dump (the model's K states; ghost states of a
// padded member are not in the dump).  In fp32, ascending k only -- the IBD scan's order (HMM.cpp:1207-1224):
//   cdf[0] = 0.f + post[0];  cdf[k] = cdf[k-1] + post[k]      (one fp32 add a state; the library is built with
//                                                              -ffp-contract=off)
//   tail for a cut c, 1 <= c <= K:      cdf[c-1], float32
//   quantile state for q, 0 < q <= 1:   the smallest k with cdf[k] >= q under an fp32 compare, int32; K-1 if no state
//                                       reaches q (rounding can leave cdf[K-1] < 1).  A NaN never compares true, so a NaN
//                                       cdf gives K-1 (the decode writes no NaN: this rule is stated, no test reaches it).
// The dump is stage[group][site][k][lane].  A workgroup of four waves owns one group and a block of 64 sites:
//   phase 1: lane = the pair's lane, wave w takes sites w, w + 4, ... of the block.  Per site the wave walks k = 0 ... K-1
//     in blocks of kPairCdfBlock states: every load is one row of 64 lanes (256 contiguous bytes), a block's loads are in
//     flight together, the adds stay in k order.  The lane records cdf at the cuts and the first k at each quantile (both
//     wave-uniform, read from a small device array) and puts them into one LDS tile per output, [64 sites][65] cells: the
//     stride of 65 keeps these row writes and the column reads below on different banks, as kPairPostStride does;
//   phase 2: lane = site.  Wave w takes pairs w, w + 4, ... of every output of the pass: it reads the pair's column of
//     the output's tile and stores 64 consecutive 4-byte cells of the pair's output row -- always a whole 256-byte line
//     of ONE row.
// kPairCdfPass outputs are kept in LDS at a time (4 x 16 640 bytes: two workgroups, eight waves, a CU); a call with more
// outputs walks the dump again for the next kPairCdfPass (16 outputs: four walks).  Lanes at or beyond a group's n_pairs
// are neither loaded nor stored, sites at or beyond S are masked in loads and stores, states at or beyond K are not
// loaded.  Float and int32 cells share the row buffer.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "fsmc_kernels.h"

namespace fsmc
{

// one output of the call: a tail (cut >= 1, q unused) or a quantile state (cut == 0)
struct PairCdfSpec {
  int cut;
  float q;
};

struct PairCdfParams {
  const float* stage;       // [nGroups][S][K][64]: the dump of the slice
  const fsmc_group* groups; // the slice's groups (a window of the resident work list)
  int nGroups;
  int K, S;
  const PairCdfSpec* spec; // [nOut]
  int nOut;
  int* rows;          // [nOut][rowsPerOut][S]: float bits for a tail, int32 for a quantile state
  size_t rowsPerOut;  // pairs of the largest slice
  unsigned firstPair; // first pair of the slice: row 0 of every output
};

constexpr int kPairCdfStride = kWave + 1;
constexpr int kPairCdfPass = 4;    // outputs kept in LDS together
constexpr int kPairCdfBlock = 8;   // rows of the dump in flight together, a wave
constexpr int kPairCdfWaves = 4;   // waves a workgroup
constexpr int kPairCdfThreads = kPairCdfWaves * kWave;

// grid: nGroups * ceil(S / 64) workgroups of kPairCdfThreads, the site block fastest
__global__ __launch_bounds__(kPairCdfThreads) void pair_cdf_kernel(const PairCdfParams p)
{
  __shared__ int tile[kPairCdfPass][kWave * kPairCdfStride];
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const unsigned siteBlocks = ((unsigned)p.S + kWave - 1) / kWave;
  const int g = (int)(blockIdx.x / siteBlocks);
  const int s0 = (int)(blockIdx.x % siteBlocks) * kWave;
  const int nS = p.S - s0 < kWave ? p.S - s0 : kWave; // sites of this block (the last one may be short)
  const int K = p.K;
  const int n = (int)p.groups[g].n_pairs < kWave ? (int)p.groups[g].n_pairs : kWave;
  const bool live = lane < n;
  const size_t siteStride = (size_t)K * kWave;
  const float* const src0 = p.stage + ((size_t)g * p.S + s0) * siteStride + lane;
  const size_t row0 = (size_t)(p.groups[g].first_pair - p.firstPair);

  for (int o0 = 0; o0 < p.nOut; o0 += kPairCdfPass) {
    const int nO = p.nOut - o0 < kPairCdfPass ? p.nOut - o0 : kPairCdfPass;
    // Per output of the pass: the state whose cdf a tail records (-1: none) and the quantile (NaN: none, it never
    // compares true).  A slot beyond nO has neither and is not stored.
    int cutAt[kPairCdfPass];
    float q[kPairCdfPass];
#pragma unroll
    for (int o = 0; o < kPairCdfPass; ++o) {
      const PairCdfSpec sp = p.spec[o0 + (o < nO ? o : 0)];
      const bool tail = o < nO && sp.cut > 0, quantile = o < nO && sp.cut <= 0;
      cutAt[o] = tail ? sp.cut - 1 : -1;
      q[o] = quantile ? sp.q : __builtin_nanf("");
    }
    if (live) {
      for (int s = w; s < nS; s += kPairCdfWaves) {
        const float* const src = src0 + (size_t)s * siteStride;
        float cdf = 0.f;
        int res[kPairCdfPass];
#pragma unroll
        for (int o = 0; o < kPairCdfPass; ++o) {
          res[o] = INT_MAX; // a quantile: no state has reached q yet
        }
        // A block of states from k0 on, v[i] = post[k0 + i]: the adds in k order, c[i] = cdf[k0 + i]; a quantile keeps
        // the smallest k whose cdf reaches it (`>=` is false for a NaN cdf), a tail whose cut lies in the block picks
        // its cdf afterwards (a wave-uniform branch, taken once a site and tail).  States at or beyond K add +0.0f,
        // which changes no cdf, and record nothing: no cut lies there, and a quantile they reach was reached at K-1.
        auto block = [&](int k0, const float(&v)[kPairCdfBlock]) {
          float c[kPairCdfBlock];
#pragma unroll
          for (int i = 0; i < kPairCdfBlock; ++i) {
            cdf = cdf + v[i];
            c[i] = cdf;
          }
#pragma unroll
          for (int o = 0; o < kPairCdfPass; ++o) {
#pragma unroll
            for (int i = 0; i < kPairCdfBlock; ++i) {
              const int at = c[i] >= q[o] ? k0 + i : INT_MAX;
              res[o] = at < res[o] ? at : res[o];
            }
            unsigned d = (unsigned)(cutAt[o] - k0);
            // (d is compared below as it stands: without this the compiler keeps cutAt[o] - i for every o and i in
            // scalar registers across the loops, more than there are, and spills them)
            asm volatile("" : "+s"(d));
            if (d < (unsigned)kPairCdfBlock) {
              float t = c[0];
#pragma unroll
              for (int i = 1; i < kPairCdfBlock; ++i) {
                t = d == (unsigned)i ? c[i] : t;
              }
              res[o] = __float_as_int(t);
            }
          }
        };
        int k0 = 0;
        for (; k0 + kPairCdfBlock <= K; k0 += kPairCdfBlock) {
          float v[kPairCdfBlock];
#pragma unroll
          for (int i = 0; i < kPairCdfBlock; ++i) {
            v[i] = src[(size_t)(k0 + i) * kWave];
          }
          block(k0, v);
        }
        if (k0 < K) { // the last, short block: states at or beyond K are not loaded
          float v[kPairCdfBlock];
#pragma unroll
          for (int i = 0; i < kPairCdfBlock; ++i) {
            v[i] = k0 + i < K ? src[(size_t)(k0 + i) * kWave] : 0.f;
          }
          block(k0, v);
        }
#pragma unroll
        for (int o = 0; o < kPairCdfPass; ++o) {
          if (o < nO) {
            tile[o][s * kPairCdfStride + lane] = (cutAt[o] < 0 && res[o] > K - 1) ? K - 1 : res[o];
          }
        }
      }
    }
    __syncthreads();
    // lane = site: wave w stores the rows of pairs w, w + 4, ... of every output of the pass
    const int siteOfLane = lane < nS ? lane : 0;
    for (int o = 0; o < nO; ++o) {
      const int* const col = &tile[o][siteOfLane * kPairCdfStride];
      int* const dst = p.rows + ((size_t)(o0 + o) * p.rowsPerOut + row0) * (size_t)p.S + (size_t)(s0 + siteOfLane);
      for (int pair = w; pair < n; pair += kPairCdfWaves) {
        const int v = col[pair];
        if (lane < nS) {
          dst[(size_t)pair * (size_t)p.S] = v;
        }
      }
    }
    __syncthreads(); // the tiles are free for the next pass
  }
}

} // namespace fsmc
