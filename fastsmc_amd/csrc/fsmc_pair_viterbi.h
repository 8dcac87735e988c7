// fsmc_pair_viterbi.h -- per pair, the single most probable JOINT state sequence of the pair under the model (the
// Viterbi path) and its probability (fsmc_decode_pair_viterbi): a max-product forward sweep with back-pointers and a
// traceback.  per_pair_MAPs is the per-site argmax of the marginals; this is the argmax over whole paths.
//
// The transition is semiseparable with non-negative entries, so `max` distributes over the
// recurrences of the forward step exactly as `+` does: AU becomes a running maximum (MU, with the state it came from),
// alphaC a suffix maximum (mC, with its state).  O(K) a site, like the decode.
//
// The definition (the contract of the entry point; tests compare for equality).  A pair whose group is the whole
// sequence, array mode, K <= 128.  Every operation is one separately rounded IEEE fp32 operation, every comparison
// exactly the one written:
//   site 0:   v[k] = pi[k] * em0[k]                                    (alpha_init's products)
//   site t>=1, from the scaled vector p of site t-1, table row stepRow[t]:
//     suffix maximum, k descending:  mC[K-1] = p[K-1], cI[K-1] = K-1;
//         for k = K-2 .. 0:  if (p[k] >= mC[k+1]) (mC[k], cI[k]) = (p[k], k) else = (mC[k+1], cI[k+1])
//     MU = 0.f, uI = 0
//     for k = 0 .. K-1 ascending:
//         d = D[k] * p[k]
//         if k >= 1:  cand = U[k-1] * p[k-1];  car = cR[k-1] * MU
//                     if (car >= cand) MU = car  (uI stays)  else (MU, uI) = (cand, k-1)
//                     (best, arg) = (MU, uI);  if (d > best) (best, arg) = (d, k)
//         else        (best, arg) = (d, 0)
//         if k < K-1: l = B[k] * mC[k+1];  if (l > best) (best, arg) = (l, cI[k+1])
//         v[k] = em_t[k] * best;   psi[t][k] = arg
//   every site: sum[t] = ((0.f + v[0]) + v[1]) + ...  (k ascending);  delta_t = v * (1.0f / sum[t])   (scale_pk)
//   end:      x[S-1] = the smallest k with delta_{S-1}[k] > every earlier one (strict >, k ascending)
//             x[t-1] = psi[t][x[t]]   for t = S-1 .. 1
//   probability of (path, observations): m = 1.0, e = 0; for t ascending: likelihoodTimes(m, e, (double)sum[t]);
//             then likelihoodTimes(m, e, (double)delta_{S-1}[x[S-1]])          (fsmc_pair_sweep.h's function)
// em_t is the emission row of the pair's observation class at site t (emis3, as the decode reads it).  On equal values
// the smaller predecessor index wins everywhere: that is what the comparisons above say.
// states[i * S + t] = x[t] (uint8), mant[i] = m, expo[i] = e, in work-list order.  A pair whose mantissa is 0 or not
// finite (a zero scaling sum somewhere) has mantissa and exponent as defined; its states are only clamped into [0, K).
//
// Ghost states (a padded member: K < KT) have p = 0 and zero table, emission and prior entries, and are never chosen:
// in the suffix maximum `>=` lets every real state k take over from the ghosts above it (p[k] >= 0), so cI[k + 1] of a
// real k < K-1 is a real state; at k = K-1 the ghost term l = B * mC = +0 is not `>` a best that is >= 0; MU of a real k
// comes from real states; a ghost's delta is +0, never `>` an earlier one at the end; and a ghost's own v is em * best
// = 0 * best = +0, which adds +0 to the sum.
//
// viterbi_kernel<KT>: lane = pair, one wave per group, the waves of the launch pull groups from an atomic queue.  The
// surroundings of the step -- the group queue, observation classes, the two-slot LDS-DMA emission ring one site ahead,
// the table rows of 64 consecutive sites in one register, the first site, the packing of the state rows -- are
// fsmc_pair_sweep.h's, shared with the other sweep kernels; the step and the traceback are this file's.  viterbi_step takes its
// operand blocks by scalar loads one block ahead like alpha_step.  Registers: p and the vector under construction (the
// suffix maxima one slot down, as alpha_step keeps alphaC: w[k] = mC[k+1] until state k is done, then v[k]), cI packed
// four bytes to a register, the back-pointers of four states packed to one dword and stored as they complete.
//
// Workspace of a wave: [chunk sites][KT4][64 lanes] u32 of back-pointers (KT4 = ceil(KT / 4): 256-byte coalesced rows, KT
// bytes a pair and site), then [chunks][KT4][64] float4 of checkpoints: the checkpointed replay of fsmc_pair_sweep.h.
// Sweep 1 also gives the sums, the mantissa chain and x[S-1]; sums and probabilities come from sweep 1 only.  With one
// chunk the traceback follows directly.  The traceback is one dependent dword load a site and lane (row x >> 2, byte
// x & 3); the states leave through packState, the dword under construction reset after each store.
#pragma once

#include <hip/hip_runtime.h>

#include "fsmc_kernels.h"
#include "fsmc_pair_sweep.h"

namespace fsmc
{

struct VitParams {
  int S;       // sites
  int W;       // 64-bit words per haplotype row
  int nGroups; // groups of the slice
  int K;       // states of the model (<= KT)
  int chunk;   // sites a chunk
  int nChunks; // ceil(S / chunk)
  unsigned pairBase; // first pair of the slice: the outputs are indexed by pair of the work list minus this
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
  unsigned char* states;    // [pairs of the slice][S], or null: the probabilities alone
  double* mant;             // [pairs of the slice], or null
  int* expo;
};

// Operand loads: asynchronous and one block ahead where the compiled instantiation passes the in-flight check
// (tools/check_inflight_sgprs.py, tests/test_isa_hazards.py), synchronous where it does not.
template <int KT> constexpr bool kVitSyncLoads = false;

typedef unsigned __attribute__((address_space(1))) * gu32_p;

// One max-product step: on entry a = delta of site t-1; on exit a = delta of site t, the return value sum[t], and this
// lane's back-pointers of site t at psiRow + lane (psiRow: the wave-uniform address of the site's row, laneOff4 = 4 * lane).
template <int KT, int KA, bool SY>
__device__ __forceinline__ float viterbi_step(float (&a)[KA], float (&w)[KA], cfloat_p rowSet, cfloat_p cR,
                                              const float4* e, const gchar_p psiRow, const unsigned laneOff4, Diag& dg)
{
  constexpr int K = KT;
  constexpr int KPc = ((KT + kKPad - 1) / kKPad) * kKPad;
  static_assert(K >= 2, "the step needs at least two states");
  typedef typename SV<kKBF>::T SVec;
  constexpr int NB = (K + kKBF - 1) / kKBF; // operand blocks (scalar loads + emission values, one block ahead)
  constexpr int NLINES = KPc / 16;
  constexpr int K4 = (KT + 3) / 4;
  SVec d = LD<kKBF, SY>::loadAt(rowSet, kRowD * KPc), bt = LD<kKBF, SY>::loadAt(rowSet, kRowB * KPc),
       u = LD<kKBF, SY>::loadAt(rowSet, kRowU * KPc), c4 = LD<kKBF, SY>::loadAt(cR, 0);
  Touched td, tbt, tu;
  if constexpr (kTouch && !SY) {
    touchRow<1, NLINES - 1>(td, rowSet, kRowD * KPc);
    touchRow<1, NLINES - 1>(tbt, rowSet, kRowB * KPc);
    touchRow<1, NLINES - 1>(tu, rowSet, kRowU * KPc);
  }
  SVec nd, nbt, nu, nc; // (assigned behind a wait before they are read)
  EmisBlk<kKBF> em = readEmis<kKBF>(e, 0), nem;
  __builtin_amdgcn_sched_barrier(0);
  // operand-free: the suffix maximum from the top, one slot down (w[k] = mC[k+1], byte k+1 of ci = cI[k+1])
  unsigned ci[K4];
#pragma unroll
  for (int j = 0; j < K4; ++j) {
    ci[j] = 0u;
  }
  {
    float mc = a[K - 1];
    unsigned cidx = (unsigned)(K - 1);
#pragma unroll
    for (int k = K - 2; k >= 0; --k) {
      w[k] = mc;
      ci[(k + 1) >> 2] |= cidx << (8 * ((k + 1) & 3));
      if (k >= 1) {
        const bool ge = a[k] >= mc;
        mc = ge ? a[k] : mc;
        cidx = ge ? (unsigned)k : cidx;
      }
    }
  }
  float MU = 0.f;
  unsigned uI = 0u;
  float sum = 0.f;
  unsigned pk = 0u;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    FSMC_WAIT_OPERANDS(dg.waitCycles);
    if (blk > 0) {
      landed(nd, nbt, nu, nc);
      d = nd;
      bt = nbt;
      u = nu;
      c4 = nc;
      em = nem;
    } else {
      landed(d, bt, u, c4);
      if constexpr (kTouch && !SY) {
        heldRow<NLINES - 1>(td);
        heldRow<NLINES - 1>(tbt);
        heldRow<NLINES - 1>(tu);
      }
    }
    if (blk + 1 < NB) {
      nd = LD<kKBF, SY>::loadAt(rowSet, kRowD * KPc + (blk + 1) * kKBF);
      nbt = LD<kKBF, SY>::loadAt(rowSet, kRowB * KPc + (blk + 1) * kKBF);
      nu = LD<kKBF, SY>::loadAt(rowSet, kRowU * KPc + (blk + 1) * kKBF);
      nc = LD<kKBF, SY>::loadAt(cR, (blk + 1) * kKBF);
      nem = readEmis<kKBF>(e, blk + 1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kKBF; ++i) {
      const int k = blk * kKBF + i;
      if (k < K) {
        const float dv = d[i] * a[k];
        float best;
        unsigned arg;
        if (k == 0) {
          best = dv;
          arg = 0u;
        } else {
          const bool gd = dv > MU;
          best = gd ? dv : MU;
          arg = gd ? (unsigned)k : uI;
        }
        if (k < K - 1) {
          const float l = bt[i] * w[k];
          const bool gl = l > best;
          best = gl ? l : best;
          arg = gl ? ((ci[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xffu) : arg;
        }
        w[k] = em.at(i) * best;
        sum = sum + w[k];
        pk |= arg << (8 * (k & 3));
        if ((k & 3) == 3 || k == K - 1) {
          *(gu32_p)(psiRow + (size_t)(k >> 2) * (kWave * sizeof(unsigned)) + laneOff4) = pk;
          pk = 0u;
        }
        if (k < K - 1) { // MU, uI of state k + 1
          const float cand = u[i] * a[k];
          const float car = c4[i] * MU;
          const bool ge = car >= cand;
          MU = ge ? car : cand;
          uI = ge ? uI : (unsigned)k;
        }
      }
    }
  }
  scale_pk<KT, KA>(a, w, sum);
  return sum;
}

// grid: any number of single-wave workgroups (one workspace slot each), no dynamic LDS.
template <int KT> __global__ __launch_bounds__(kWave, minWavesPerSimd(KT)) void viterbi_kernel(const VitParams p)
{
  static_assert(KT >= 2 && KT <= 128, "a lane-per-pair member (fsmc_instances.h)");
  constexpr int KA = KT;
  using Sh = SweepShape<KT, 3>;
  constexpr bool SY = kVitSyncLoads<KT>;
  constexpr size_t kPsiRow = (size_t)Sh::K4 * kWave * sizeof(unsigned);  // bytes of a site's back-pointers

  __shared__ float4 ring[2][Sh::NC * Sh::E4];

  const int lane = threadIdx.x;
  const unsigned laneOff = threadIdx.x * (unsigned)sizeof(float4);
  const unsigned laneOff4 = threadIdx.x * (unsigned)sizeof(unsigned);
  const SweepParams sp = sweepParams(p);
  const cfloat_p tPi = (cfloat_p)sp.pi;
  const Tables tabs = {(cfloat_p)sp.rowSets, (cfloat_p)sp.cR, (cfloat_p) nullptr};
  const int S = sp.S;
  const int C = p.chunk;
  const int nChunks = p.nChunks;
  const bool trace = p.states != nullptr;
  char* const slot = p.ws + (size_t)blockIdx.x * p.slotBytes;
  char* const psiBuf = slot;
  char* const ckptBuf = slot + (size_t)C * kPsiRow;
  const int lastStart = trace ? (nChunks - 1) * C : S; // sweep 1 keeps the back-pointers from this site on

  for (;;) {
    const unsigned g = pullGroup(sp.counter, lane);
    if (g >= (unsigned)sp.nGroups) {
      break;
    }
    const PairLane pl = pairLane(sp, g, lane);
    ObsWords obs{pl.rowA, pl.rowB};
    RowIndexBlock stepRows;
    // site q's rows into ring slot (q & 1)
    auto stage = [&](const int q) {
      stageRows<Sh::NL>(sp.emis3 + (size_t)q * (Sh::NC * Sh::E4), ring[q & 1], Sh::NC * Sh::E4, lane, laneOff);
    };

    float a[KA], w[KA];
    Diag dg;
    double m = 1.0;
    int e = 0;

    // ---- sweep 1: the whole sequence
    stage(0);
    for (int pos = 0; pos < S; ++pos) {
      landedRows();
      if (pos + 1 < S) {
        stage(pos + 1); // into the slot of site pos - 1, whose step is over
      }
      const int c = obs.classAt(pos);
      const float4* er = &ring[pos & 1][c * Sh::E4];
      float sum;
      if (__builtin_expect(pos == 0, 0)) {
        sum = firstSite<KT, KA>(a, tPi, er);
      } else {
        if (trace && pos % C == 0) { // delta of the site before chunk pos / C
          store_vec<KT, KA>(KT, (float4*)(ckptBuf + (size_t)(pos / C) * Sh::kVecBytes), laneOff, a);
        }
        const int r = pos >= lastStart ? pos - lastStart : 0;
        sum = viterbi_step<KT, KA, SY>(a, w, rowSetOf<KT>(tabs, stepRows.at(sp.stepRow, S, lane, pos)), tabs.cR, er,
                                       uniformPtr(psiBuf + (size_t)r * kPsiRow), laneOff4, dg);
      }
      likelihoodTimes(m, e, (double)sum);
    }
    // x[S-1]: the first maximum of the last delta
    unsigned x = 0u;
    {
      float best = a[0];
#pragma unroll
      for (int k = 1; k < KT; ++k) {
        const bool gt = a[k] > best;
        best = gt ? a[k] : best;
        x = gt ? (unsigned)k : x;
      }
      likelihoodTimes(m, e, (double)best);
    }
    if (pl.valid && p.mant) {
      p.mant[pl.outIdx] = m;
      p.expo[pl.outIdx] = e;
    }
    if (!trace) {
      continue;
    }

    // ---- the traceback, chunk by chunk descending; every chunk but the last is swept again from its checkpoint first
    const unsigned kTop = (unsigned)(p.K - 1);
    const size_t rowByte = pl.outIdx * (size_t)S; // this pair's row in the slice's state rows
    unsigned char* const out = p.states;
    unsigned acc = 0u; // the bytes of the output dword under construction
    for (int ch = nChunks - 1; ch >= 0; --ch) {
      const int lo = ch * C;
      const int hi = (lo + C < S ? lo + C : S) - 1; // the chunk's last site
      if (ch != nChunks - 1) {
        obs.restart();
        waitVm0(); // (nothing of the traceback before is in flight when the ring is restarted)
        stage(lo);
        if (lo > 0) {
          load_vec<KT, KA>(KT, (const float4*)(ckptBuf + (size_t)ch * Sh::kVecBytes), laneOff, a);
        }
        for (int pos = lo; pos <= hi; ++pos) {
          landedRows();
          if (pos < hi) {
            stage(pos + 1);
          }
          const int c = obs.classAt(pos);
          const float4* er = &ring[pos & 1][c * Sh::E4];
          if (__builtin_expect(pos == 0, 0)) {
            (void)firstSite<KT, KA>(a, tPi, er);
          } else {
            (void)viterbi_step<KT, KA, SY>(a, w, rowSetOf<KT>(tabs, stepRows.at(sp.stepRow, S, lane, pos)), tabs.cR, er,
                                           uniformPtr(psiBuf + (size_t)(pos - lo) * kPsiRow), laneOff4, dg);
          }
        }
      }
      const gchar_p psiBase = uniformPtr(psiBuf);
      for (int t = hi; t >= lo; --t) {
        x = x < kTop ? x : kTop; // (a no-op for every pair with a finite, non-zero probability)
        if (packState(acc, x, out, rowByte, t, S, pl.valid)) {
          acc = 0u;
        }
        if (t >= 1) {
          const unsigned dw = *(gu32_p)(psiBase + (size_t)(t - lo) * kPsiRow + (size_t)(x >> 2) * (kWave * sizeof(unsigned)) +
                                        laneOff4);
          x = (dw >> (8u * (x & 3u))) & 0xffu;
        }
      }
    }
  }
}

} // namespace fsmc
