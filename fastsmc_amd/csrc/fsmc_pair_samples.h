// fsmc_pair_samples.h -- per pair, n state sequences drawn from the JOINT posterior over sequences given the pair's
// observations (fsmc_decode_pair_samples): forward filtering with backward sampling.  The Viterbi path
// (fsmc_pair_viterbi.h) is one point without spread, the marginals have spread without dependence between sites; these
// are whole tracks with the right joint law.
//
// The transition is semiseparable: the forward step's term for state j is a sum over the states
// i of coefficient(i, j) * delta_t[i], and the coefficients of one column j cost O(K): B[j] above j, D[j] at j, U[i]
// times a running product of column ratios below j.  Those are the weights of the predecessor of j.
//
// The definition (the contract of the entry point; tests compare for equality).  A pair whose group is the whole
// sequence, array mode, K <= 128.  Every operation is one separately rounded IEEE fp32 operation.  delta_t is the scaled
// forward vector of site t, exactly what forward_kernel (fsmc_pair_loglik.h) holds after scale_pk.
//   uniform of (seed, pair, sample r, site t):
//     Philox4x32-10, key = (seed & 0xffffffff, seed >> 32),
//     counter = (t >> 2, r, hap_a, hap_b)          (the pair's two fields of the work list, as stored)
//     u = float(out[t & 3] >> 8) * 2^-24           (exact, in [0, 1))
//   pick(w[0..K-1], u):
//     c[-1] = 0.f;  c[i] = c[i-1] + w[i]   for i ascending
//     x = u * c[K-1]
//     state = min(K-1, #{ i in [0, K) : c[i] <= x })   (exactly this comparison; K the model's states)
//   site S-1:  w[i] = delta_{S-1}[i];   x[S-1] = pick(w, u(S-1))
//   site t = S-2 .. 0, with j = x[t+1] and D, B, U the table row stepRow[t+1], cR the column ratios:
//     i > j:   w[i] = B[j] * delta_t[i]
//     i = j:   w[j] = D[j] * delta_t[j]
//     i < j:   g = 1.f at i = j-1;   for i = j-2 .. 0:  g = g * cR[i+1]
//              w[i] = (U[i] * delta_t[i]) * g
//     x[t] = pick(w, u(t))
// states[(i * n + r) * S + t] = x[t] of sample r (uint8), i in work-list order.  A chosen state always has w > 0
// (c[i] > x >= c[i-1]), so every sampled path is one the model allows.  A sample depends on (seed, hap_a, hap_b, r, t)
// and the data only: not on list order, groups, slices, chunk length, workspace.  A pair with a zero scaling sum
// somewhere (NaN vectors) only has states in [0, K).
//
// Ghost states (a padded member: K < KT) have delta = 0 and zero table entries, so w = +0 and c stays at the total,
// which is > x: they are never counted and never chosen.  The clamp uses the model's K, not KT.
// The kernel forms every weight as (coefficient * delta_t[i]) * g with g = 1.f at i >= j - 1: a product with 1.f is the
// value itself.  c[0] is w[0] itself (0.f + w[0]).
//
// sample_kernel<KT>: lane = pair, one wave per group, the waves of the launch pull groups from an atomic queue.  The
// surroundings of the forward step are fsmc_pair_sweep.h's, the step is forward_kernel's (forwardStep, scale_pk).
// Workspace of a wave: [chunk sites][KT4][64 lanes] float4 of delta rows (KT4 = ceil(KT / 4), coalesced 1-KiB stores),
// then [chunks][KT4][64] float4 of checkpoints: the checkpointed replay of fsmc_pair_sweep.h, a row being delta of its
// site.  The walk is site-outer and sample-inner: a delta row is loaded once
// for all n samples.  A sample and site take three passes over the K registers: the weights descending with the
// predicated g chain (U and cR as scalar operand blocks like alpha_step's; D[j] and B[j] gathered per lane, the next
// sample's one sample ahead), the running sums ascending in place, the count.
// A lane's n samples each keep one dword in LDS: the bytes of the output dword under construction, among them the state
// of site t+1.  The states leave through packState (fsmc_pair_sweep.h); the dword stays in LDS beyond its store.
#pragma once

#include <hip/hip_runtime.h>

#include "fsmc_kernels.h"
#include "fsmc_pair_sweep.h"
#include "fsmc_philox.h"

namespace fsmc
{

constexpr int kMaxSamples = 64; // samples a pair and call

struct SmpParams {
  int S;       // sites
  int W;       // 64-bit words per haplotype row
  int nGroups; // groups of the slice
  int K;       // states of the model (<= KT)
  int chunk;   // sites a chunk
  int nChunks; // ceil(S / chunk)
  int nSamples; // samples a pair (1 .. kMaxSamples)
  unsigned pairBase; // first pair of the slice: the outputs are indexed by pair of the work list minus this
  unsigned seedLo, seedHi;
  const float* pi;      // [KP]
  const float* cR;      // [KP]
  const float* rowSets; // [rows][5][KP]
  const int* stepRow;   // [S] row of the step into site q
  const float4* emis3;  // [S][3][KP/4]
  const unsigned long long* haps; // [nHaps][W]
  const fsmc_pair* pairs;
  const fsmc_group* groups; // the slice's first group
  unsigned* counter;        // head of the group queue
  char* ws;                 // the waves' workspaces, slotBytes each
  size_t slotBytes;
  unsigned char* states;    // [pairs of the slice][nSamples][S]
};

// Operand loads: asynchronous and one block ahead where the compiled instantiation passes the in-flight check
// (tools/check_inflight_sgprs.py, tests/test_isa_hazards.py), synchronous where it does not.
template <int KT> constexpr bool kSmpSyncLoads = KT == 32;

// The weights of the predecessors of state j (this lane's), i descending: w[i] = (coefficient * a[i]) * g.
template <int KT, int KA, bool SY>
__device__ __forceinline__ void sample_weights(const float (&a)[KA], float (&w)[KA], cfloat_p rowSet, cfloat_p cR,
                                               const unsigned j, const float dj, const float bj, Diag& dg)
{
  constexpr int K = KT;
  constexpr int KPc = ((KT + kKPad - 1) / kKPad) * kKPad;
  typedef typename SV<kKBF>::T SVec;
  constexpr int NB = (K + kKBF - 1) / kKBF;
  SVec u = LD<kKBF, SY>::loadAt(rowSet, kRowU * KPc + (NB - 1) * kKBF), c = LD<kKBF, SY>::loadAt(cR, (NB - 1) * kKBF);
  SVec nu, nc; // (assigned behind a wait before they are read)
  __builtin_amdgcn_sched_barrier(0);
  float g = 1.f;
  float cAbove = 1.f; // cR of the state above the block's top one
#pragma unroll
  for (int blk = NB - 1; blk >= 0; --blk) {
    FSMC_WAIT_OPERANDS(dg.waitCycles);
    if (blk < NB - 1) {
      landed(nu, nc);
      u = nu;
      c = nc;
    } else {
      landed(u, c);
    }
    if (blk > 0) {
      nu = LD<kKBF, SY>::loadAt(rowSet, kRowU * KPc + (blk - 1) * kKBF);
      nc = LD<kKBF, SY>::loadAt(cR, (blk - 1) * kKBF);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = kKBF - 1; i >= 0; --i) {
      const int k = blk * kKBF + i;
      if (k < K) {
        if (k < K - 1) { // g of state k: 1.f down to j - 1, then the product of cR[k+1 .. j-1]
          const float gm = g * (i == kKBF - 1 ? cAbove : c[i + 1]);
          g = (unsigned)(k + 1) < j ? gm : 1.f;
        }
        const float coef = (unsigned)k < j ? u[i] : ((unsigned)k == j ? dj : bj);
        w[k] = (coef * a[k]) * g;
      }
    }
    cAbove = c[0];
  }
}

// pick(): the running sums ascending in place, x = u * total, the count of c[i] <= x.
template <int KT, int KA> __device__ __forceinline__ unsigned sample_pick(float (&w)[KA], const float u)
{
#pragma unroll
  for (int k = 1; k < KT; ++k) {
    w[k] = w[k - 1] + w[k];
  }
  const float x = u * w[KT - 1];
  unsigned cnt = 0u;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    cnt += w[k] <= x ? 1u : 0u;
  }
  return cnt;
}

// grid: any number of single-wave workgroups (one workspace slot each), no dynamic LDS.
template <int KT> __global__ __launch_bounds__(kWave, minWavesPerSimd(KT)) void sample_kernel(const SmpParams p)
{
  static_assert(KT >= 2 && KT <= 128, "a lane-per-pair member (fsmc_instances.h)");
  constexpr int KA = KT;
  using Sh = SweepShape<KT, 3>;
  constexpr bool SY = kSmpSyncLoads<KT>;

  __shared__ float4 ring[2][Sh::NC * Sh::E4];
  __shared__ unsigned accs[kMaxSamples][kWave]; // a sample's output dword under construction, per lane

  const int lane = threadIdx.x;
  const unsigned laneOff = threadIdx.x * (unsigned)sizeof(float4);
  const SweepParams sp = sweepParams(p);
  const cfloat_p tPi = (cfloat_p)sp.pi;
  const Tables tabs = {(cfloat_p)sp.rowSets, (cfloat_p)sp.cR, (cfloat_p) nullptr};
  const int S = sp.S;
  const int C = p.chunk;
  const int nChunks = p.nChunks;
  const int n = p.nSamples;
  char* const slot = p.ws + (size_t)blockIdx.x * p.slotBytes;
  char* const rowBuf = slot;
  char* const ckptBuf = slot + (size_t)C * Sh::kVecBytes;
  const int lastStart = (nChunks - 1) * C; // sweep 1 keeps the rows from this site on
  const unsigned kTop = (unsigned)(p.K - 1);
  unsigned char* const out = p.states;

  for (;;) {
    const unsigned g = pullGroup(sp.counter, lane);
    if (g >= (unsigned)sp.nGroups) {
      break;
    }
    const PairLane pl = pairLane(sp, g, lane);
    const fsmc_pair pr = sp.pairs[pl.pairIdx];
    ObsWords obs{pl.rowA, pl.rowB};
    RowIndexBlock stepRows;
    // site q's rows into ring slot (q & 1)
    auto stage = [&](const int q) {
      stageRows<Sh::NL>(sp.emis3 + (size_t)q * (Sh::NC * Sh::E4), ring[q & 1], Sh::NC * Sh::E4, lane, laneOff);
    };

    float a[KA], w[KA];
    Diag dg;

    // one site of a forward sweep: delta of site pos in a, stored as row `r` of the buffer
    auto forwardSite = [&](const int pos, const int r) {
      const int c = obs.classAt(pos);
      const float4* er = &ring[pos & 1][c * Sh::E4];
      const float sum = forwardStep<KT, KA, SY>(a, w, er, tPi, tabs, stepRows, sp.stepRow, S, lane, pos, dg);
      scale_pk<KT, KA>(a, a, sum);
      store_vec<KT, KA>(KT, (float4*)(rowBuf + (size_t)r * Sh::kVecBytes), laneOff, a);
    };

    // ---- sweep 1: the whole sequence
    stage(0);
    for (int pos = 0; pos < S; ++pos) {
      landedRows();
      if (pos + 1 < S) {
        stage(pos + 1); // into the slot of site pos - 1, whose step is over
      }
      if (pos > 0 && pos % C == 0) { // delta of the site before chunk pos / C
        store_vec<KT, KA>(KT, (float4*)(ckptBuf + (size_t)(pos / C) * Sh::kVecBytes), laneOff, a);
      }
      forwardSite(pos, pos >= lastStart ? pos - lastStart : 0);
    }
    for (int r = 0; r < n; ++r) {
      accs[r][lane] = 0u;
    }

    // ---- the walk, chunk by chunk descending; every chunk but the last is swept again from its checkpoint first
    const size_t pairRow = pl.outIdx * (size_t)n; // this pair's first row of the slice's state rows
    for (int ch = nChunks - 1; ch >= 0; --ch) {
      const int lo = ch * C;
      const int hi = (lo + C < S ? lo + C : S) - 1; // the chunk's last site
      if (ch != nChunks - 1) {
        obs.restart();
        waitVm0(); // (nothing of the walk before is in flight when the ring is restarted)
        stage(lo);
        if (lo > 0) {
          load_vec<KT, KA>(KT, (const float4*)(ckptBuf + (size_t)ch * Sh::kVecBytes), laneOff, a);
        }
        for (int pos = lo; pos <= hi; ++pos) {
          landedRows();
          if (pos < hi) {
            stage(pos + 1);
          }
          forwardSite(pos, pos - lo);
        }
      }
      waitVm0(); // the chunk's rows are written
      for (int t = hi; t >= lo; --t) {
        load_vec<KT, KA>(KT, (const float4*)(rowBuf + (size_t)(t - lo) * Sh::kVecBytes), laneOff, a);
        const bool top = t == S - 1;
        const int row = top ? 0 : stepRows.at(sp.stepRow, S, lane, t + 1);
        const cfloat_p rowSet = rowSetOf<KT>(tabs, row);
        const float* const rowD = p.rowSets + (size_t)row * (kRowSetParts * Sh::KPc) + kRowD * Sh::KPc;
        const float* const rowB = p.rowSets + (size_t)row * (kRowSetParts * Sh::KPc) + kRowB * Sh::KPc;
        // the state of site t + 1 of sample r and its two table entries, one sample ahead
        auto carried = [&](const int r, unsigned& acc, unsigned& j, float& dj, float& bj) {
          acc = accs[r][lane];
          const unsigned A1 = (unsigned)((pairRow + (size_t)r) * (size_t)S + (size_t)t + 1u);
          j = (acc >> (8u * (A1 & 3u))) & 0xffu;
          dj = rowD[j];
          bj = rowB[j];
        };
        unsigned accN = 0u, jN = 0u;
        float djN = 0.f, bjN = 0.f;
        if (!top) {
          carried(0, accN, jN, djN, bjN);
        }
        for (int r = 0; r < n; ++r) {
          unsigned acc = accN;
          if (top) {
#pragma unroll
            for (int k = 0; k < KT; ++k) {
              w[k] = a[k];
            }
          } else {
            const unsigned j = jN;
            const float dj = djN, bj = bjN;
            carried(r + 1 < n ? r + 1 : r, accN, jN, djN, bjN);
            sample_weights<KT, KA, SY>(a, w, rowSet, tabs.cR, j, dj, bj, dg);
          }
          const float u = sampleUniform(p.seedLo, p.seedHi, pr.hap_a, pr.hap_b, (unsigned)r, (unsigned)t);
          unsigned x = sample_pick<KT, KA>(w, u);
          x = x < kTop ? x : kTop;
          // (the dword stays in LDS beyond its store: the state of site t is the next site's j)
          (void)packState(acc, x, out, (pairRow + (size_t)r) * (size_t)S, t, S, pl.valid);
          accs[r][lane] = acc;
        }
      }
    }
  }
}

} // namespace fsmc
