// fsmc_pair_loglik.h -- per pair, the likelihood of the pair's observations under the model from the forward sweep
// alone (fsmc_decode_pair_loglik): one of the decode's three sweeps, no beta rows, no workspace, no checkpoints.
//
// The definition (the contract of the entry point).  For a pair whose group is the whole sequence let sum[t] (fp32) be
// the scaling sum of the forward vector at site t: the `sums` of calculateScalingBatch at HMM.cpp:745 and 776-779,
// accumulated from 0.f over k ascending in separately rounded adds (ghost states add +0).  Array mode: sum[0] comes
// from pi * emission and sum[t] from the step into site t.  Sequence mode: the un-normalised half-step across the gap
// contributes no sum of its own; sum[t] is the sum after the site step that follows it (HMM.cpp:760-779).  The product
// of the sums is P(observations of the pair | model); it is carried as a mantissa / exponent pair so that the result is
// bit-reproducible:
//     m = 1.0 (fp64); e = 0 (int32)
//     for t = 0 .. S-1, ascending:
//         m = m * (double)sum[t]                                       // one fp64 multiply, round to nearest
//         if (m != 0 && isfinite(m)) { m = frexp(m, &de); e += de; }   // exact
// mant[i] = m (in [0.5, 1), or 0 / inf / NaN), expo[i] = e, in work-list order; the log-likelihood is
// log(mant) + expo * ln 2, formed on the host in fp64 (a zero sum gives -inf, a NaN stays a NaN).
// With bin edges e[0] < ... < e[B] (the rules of fsmc_decode_pair_bins) bin_mant[i][b] / bin_expo[i][b] are the same
// recurrence started afresh at m = 1, e = 0 at site e[b] and taken at site e[b+1] - 1: the conditional likelihood of the
// bin's observations given everything before it.  Sites outside every bin count towards the total only; the total is a
// chain of its own over all sites, not a combination of the bins.
//
// forward_kernel<KT, SEQ>: lane = pair, one wave per group, the waves of the launch pull groups from an atomic queue.
// The arithmetic of a site is the decode's (fsmc_kernels.h): alpha_step<..., SCALE = false>, the ascending sum of what
// it leaves (the adds of the scaled step, in its order: the compiler folds the two chains into one), scale_pk; the first
// site is alpha_init with its sum handed back (forwardInit).  What surrounds the steps is fsmc_pair_sweep.h's, shared with
// viterbi_kernel (fsmc_pair_viterbi.h): the group queue, the observation classes from the packed haplotype words, a
// two-slot LDS ring of emission rows fed by LDS-DMA one site ahead (three rows a site, four in sequence mode), the table
// rows of 64 consecutive sites in one register.  This kernel's own are the fp64 recurrence over the sums, the bins and
// the sequence-mode half-step.  The site loop is wave-uniform, so the open bin is scalar state; a bin's two values leave
// with ordinary vector stores when it closes.  No workspace: the kernel's HBM traffic is the emission rows (12 or 16
// bytes a state and site for the WAVE, not the pair) and 12 bytes a pair and output.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "fsmc_kernels.h"
#include "fsmc_pair_sweep.h"

namespace fsmc
{

struct FwdParams {
  int S;       // sites
  int W;       // 64-bit words per haplotype row
  int nGroups; // groups of the slice
  int B;       // bins (0: none)
  unsigned pairBase; // first pair of the slice: the outputs are indexed by pair of the work list minus this
  const float* pi;      // [KP]
  const float* cR;      // [KP]
  const float* rowSets; // [rows][5][KP]
  const int* stepRow;   // [S] row of the (site) step into site q
  const int* rowGapF;   // [S] sequence mode: row of the half-step across the gap (q-1, q)
  const float4* emis3;  // [S][3 or 4][KP/4]
  const unsigned long long* haps; // [nHaps][W]
  const fsmc_pair* pairs;
  const fsmc_group* groups; // the slice's first group
  unsigned* counter;        // head of the group queue
  const int* edges;         // [B + 1], or null
  double* mant;             // [pairs of the slice], or null
  int* expo;
  double* binMant;          // [pairs of the slice][B], or null
  int* binExpo;
};

// Operand loads of the steps: asynchronous and one block ahead where the compiled instantiation passes the in-flight
// check (tools/check_inflight_sgprs.py, tests/test_isa_hazards.py), synchronous (LD<N, true>) where it does not: the
// 32-state member in both modes, whose allocation spills operand blocks behind their loads (v_writelane of
// registers in flight); every other instantiation of the default build is clean.
template <int KT, bool SEQ> constexpr bool kFwdSyncLoads = KT == 32;

// grid: any number of single-wave workgroups, no dynamic LDS.
template <int KT, bool SEQ>
__global__ __launch_bounds__(kWave, minWavesPerSimd(KT)) void forward_kernel(const FwdParams p)
{
  static_assert(KT >= 2 && KT <= 128, "a lane-per-pair member (fsmc_instances.h)");
  constexpr int KA = KT;
  using Sh = SweepShape<KT, SEQ ? 4 : 3>; // rows per site: the observation classes (+ the gap)
  constexpr int K = KT;
  constexpr bool SY = kFwdSyncLoads<KT, SEQ>;

  __shared__ float4 ring[2][Sh::NC * Sh::E4];

  const int lane = threadIdx.x;
  const unsigned laneOff = threadIdx.x * (unsigned)sizeof(float4);
  const SweepParams sp = sweepParams(p);
  const cfloat_p tPi = (cfloat_p)sp.pi;
  const Tables tabs = {(cfloat_p)sp.rowSets, (cfloat_p)sp.cR, (cfloat_p) nullptr};
  const cint_p tEdges = (cint_p)p.edges;
  const int S = sp.S;
  const int B = p.B;

  for (;;) {
    const unsigned g = pullGroup(sp.counter, lane);
    if (g >= (unsigned)sp.nGroups) {
      break;
    }
    const PairLane pl = pairLane(sp, g, lane);
    ObsWords obs{pl.rowA, pl.rowB};
    RowIndexBlock stepRows, gapRows;
    // site q's rows into ring slot (q & 1)
    auto stage = [&](const int q) {
      stageRows<Sh::NL>(sp.emis3 + (size_t)q * (Sh::NC * Sh::E4), ring[q & 1], Sh::NC * Sh::E4, lane, laneOff);
    };

    // the open bin: [lo, hi) = edges[bin], edges[bin + 1]; beyond the last bin lo = INT_MAX
    int bin = 0;
    int lo = INT_MAX, hi = INT_MAX;
    if (B > 0) {
      lo = tEdges[0];
      hi = tEdges[1];
    }
    double m = 1.0, bm = 1.0;
    int e = 0, be = 0;

    float a[KA], w[KA];
    Diag dg;
    stage(0);
    for (int pos = 0; pos < S; ++pos) {
      if (!SEQ || pos == 0) {
        landedRows(); // the rows of site pos (sequence mode: the half-step towards pos waited for them)
      }
      if (pos + 1 < S) {
        stage(pos + 1); // into the slot of site pos - 1, whose steps are over
      }
      const int c = obs.classAt(pos);
      const float4* er = &ring[pos & 1][c * Sh::E4];
      float sum;
      if (__builtin_expect(pos == 0, 0)) {
        sum = forwardInit<KT, KA>(a, tPi, er);
      } else {
        alpha_step<KT, KA, false, SY>(K, a, w, tabs, stepRows.at(sp.stepRow, S, lane, pos), er, dg);
        sum = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          sum = sum + a[k];
        }
      }
      scale_pk<KT, KA>(a, a, sum);

      const double sd = (double)sum;
      likelihoodTimes(m, e, sd);
      if (pos >= lo) { // inside the open bin (pos < hi: a bin is closed at its last site)
        if (pos == lo) {
          bm = 1.0;
          be = 0;
        }
        likelihoodTimes(bm, be, sd);
        if (pos == hi - 1) {
          if (pl.valid) {
            p.binMant[pl.outIdx * (size_t)B + (size_t)bin] = bm;
            p.binExpo[pl.outIdx * (size_t)B + (size_t)bin] = be;
          }
          ++bin;
          lo = bin < B ? hi : INT_MAX;
          hi = bin < B ? tEdges[bin + 1] : INT_MAX;
        }
      }

      if constexpr (SEQ) {
        // the un-normalised half-step across the gap to the next site (HMM.cpp:760-767): no sum of its own
        if (pos + 1 < S) {
          landedRows(); // the rows of site pos + 1: its fourth row is the homozygous emission of the gap before it
          alpha_step<KT, KA, false, SY>(K, a, w, tabs, gapRows.at(p.rowGapF, S, lane, pos + 1),
                                        &ring[(pos + 1) & 1][3 * Sh::E4], dg);
        }
      }
    }
    if (pl.valid && p.mant) {
      p.mant[pl.outIdx] = m;
      p.expo[pl.outIdx] = e;
    }
  }
}

} // namespace fsmc
