// fsmc_pair_transitions.h -- per pair and site, the posterior probability that the state changes between site t-1 and
// site t, and in which direction (fsmc_decode_pair_transitions): the two-slice posterior summed below and above the
// diagonal.  The marginals carry no dependence between neighbouring sites, the Viterbi path (fsmc_pair_viterbi.h) has no
// uncertainty, and counting over sampled paths (fsmc_pair_samples.h) costs n samples for 1 / sqrt(n); this is exact and
// costs about one decode.
//
// The transition is semiseparable: the backward step forms, per state k of site t-1, the mass
// moving to lower states (BL[k]), staying (D[k] * vec[k]) and moving to higher states (BU[k]).  Three dot products with
// the scaled forward vector of site t-1 are the three two-slice probabilities, O(K) a site.
//
// The definition (the contract of the entry point; tests compare for equality).  A pair whose group is the whole
// sequence, array mode, K <= 128.  Every operation is one separately rounded IEEE fp32 operation.  delta_t is the scaled
// forward vector of site t, exactly what forward_kernel (fsmc_pair_loglik.h) holds after scale_pk.  b_t is the scaled
// backward vector of the decode kernels: b_{S-1}[k] = 1.f * (1.0f / sum) with sum over the model's K states; going down,
// one backward step in the order (BL + D * vec) + BU, then scale_pk.
//   site t = S-1 .. 1, with D, B, U, RR the table row stepRow[t] and e the emission of the pair's class at site t:
//     vec[k] = b_t[k] * e[k]
//     BU[K-1] = 0.f;  BU[k] = U[k] * vec[k+1] + RR[k] * BU[k+1]       (k descending)
//     BL[0]   = 0.f;  BL[k] = BL[k-1] + B[k-1] * vec[k-1]            (k ascending)
//     down = up = stay = 0.f;  for k ascending over the model's K states:
//       down = down + delta_{t-1}[k] * BL[k]
//       stay = stay + delta_{t-1}[k] * (D[k] * vec[k])
//       up   = up   + delta_{t-1}[k] * BU[k]
//     z = (down + stay) + up;   r = 1.0f / z
//     p_down[t] = down * r;     p_up[t] = up * r
//   p_down[0] = p_up[0] = 0.f.
// p_down[t] is the posterior probability that the state at site t is lower than the state at site t-1, p_up[t] that it
// is higher, 1 - p_down - p_up that it is the same.  down[i * S + t], up[i * S + t], i in work-list order.  A pair with a
// zero scaling sum somewhere gives whatever IEEE gives (NaN).  The results depend on the pair and the data only: not on
// list order, groups, slices, chunk length, workspace.
//
// Ghost states (a padded member: K < KT) have delta = 0 and zero table entries: they contribute +0.f products and change
// nothing.  The first scaling of b uses the model's K, not KT.
//
// transition_kernel<KT>: lane = pair, one wave per group, the waves of the launch pull groups from an atomic queue
// (fsmc_pair_sweep.h).  The workspace of a wave is sample_kernel's (planSamples): [chunk sites][KT4][64 lanes] float4
// of delta rows, then [chunks][KT4][64] float4 of checkpoints: the checkpointed replay of fsmc_pair_sweep.h with
// sample_kernel's site step (forwardStep, scale_pk, the row stored).  While a chunk is swept again b waits in
// checkpoint slot 0, which no chunk uses (a lane holds two K-vectors at any time); a chunk that holds site 0 alone is
// neither swept nor walked.  Then the chunk is walked down with b in registers.  A site of the walk is one
// backward step (transition_core_pk: beta_core_pk's recurrences with the three accumulators in the ascending pass, where
// BL, D * vec and BU are live); the row of t-1 is not held but read in blocks of sixteen states one block ahead of the
// ascending pass.  At a chunk's first site the row of t-1 is the chunk's checkpoint.
// A lane buffers four sites of each output and stores aligned float4, single floats at a row's unaligned ends (rows are
// S floats apart).  Vector stores only.
#pragma once

#include <hip/hip_runtime.h>

#include "fsmc_kernels.h"
#include "fsmc_pair_sweep.h"

namespace fsmc
{

struct TrnParams {
  int S;       // sites
  int W;       // 64-bit words per haplotype row
  int nGroups; // groups of the slice
  int K;       // states of the model (<= KT)
  int chunk;   // sites a chunk
  int nChunks; // ceil(S / chunk)
  unsigned pairBase; // first pair of the slice: the outputs are indexed by pair of the work list minus this
  const float* pi;        // [KP]
  const float* cR;        // [KP]
  const float* rowSets;   // [rows][5][KP]
  const float* ghostMask; // [KP]
  const int* stepRow;     // [S] row of the step into site q
  const float4* emis3;    // [S][3][KP/4]
  const unsigned long long* haps; // [nHaps][W]
  const fsmc_pair* pairs;
  const fsmc_group* groups; // the slice's first group
  unsigned* counter;        // head of the group queue
  char* ws;                 // the waves' workspaces, slotBytes each
  size_t slotBytes;
  float* down;              // [pairs of the slice][S], 16-byte aligned
  float* up;                // [pairs of the slice][S], 16-byte aligned
};

// Operand loads: asynchronous and one block ahead where the compiled instantiation passes the in-flight check
// (tools/check_inflight_sgprs.py, tests/test_isa_hazards.py), synchronous where it does not.
// (the 32-state member as in sample_kernel; in the 48- and 50-state members the allocator spills the walk's operand blocks
// right behind their loads)
template <int KT> constexpr bool kTrnSyncLoads = KT == 32 || KT == 48 || KT == 50;

// Sixteen states of this lane's column of a stored row (store_vec's layout), from float4 group k4 on; groups beyond the
// row are not read.
template <int KT> struct RowBlk {
  f32x4 v[kKB / 4];
  __device__ __forceinline__ float at(const int i) const { return v[i >> 2][i & 3]; }
  __device__ __forceinline__ f32x2 pair(const int i) const
  {
    const f32x2 r = {v[i >> 2][i & 3], v[i >> 2][(i & 3) + 1]};
    return r;
  }
};
template <int KT> __device__ __forceinline__ RowBlk<KT> readRowBlk(const gchar_p row, const int blk, const unsigned laneOff)
{
  constexpr int K4 = (KT + 3) / 4;
  RowBlk<KT> r;
#pragma unroll
  for (int j = 0; j < kKB / 4; ++j) {
    if (blk * (kKB / 4) + j < K4) {
      r.v[j] = __builtin_nontemporal_load(rowSlot(row, blk * (kKB / 4) + j, laneOff));
    } else {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      r.v[j] = z;
    }
  }
  return r;
}

// The recurrences of one backward step (beta_core_pk's, the same operations in the same order) and, in the ascending
// pass, the three sums over delta of site t-1 (`frow`: the stored row).  On entry b = beta of site t (scaled), on exit
// w = the un-normalised beta of site t-1 and the return value its sum; b is used up.
template <int KT, int KA, bool GHOST, bool SY>
__device__ __forceinline__ float transition_core_pk(float (&b)[KA], float (&w)[KA], BetaOps<KT>& ops, cfloat_p rowSet,
                                                    const float4* e, cfloat_p ghostMask, const gchar_p frow,
                                                    const unsigned laneOff, float& down, float& stay, float& up,
                                                    Diag& dg)
{
  constexpr int K = KT;
  constexpr int KPc = ((KT + kKPad - 1) / kKPad) * kKPad;
  typedef typename SV<kKB>::T SVec;
  constexpr int NB = (K + kKB - 1) / kKB;
  constexpr int R = kKB / 8;
  constexpr int NLINES = KPc / 16;
  static_assert(kKB == 16, "line warm-up and ghost masking are laid out for operand blocks of one 64-byte line");
  static_assert(!GHOST || K % kKB == 0, "ghost padding fills whole operand blocks");
  SVec u, rr, nu, nrr; // (assigned behind a wait before they are read; see beta_core_pk)
  EmisBlk<kKB> em, nem;
  SVec d, bt, nd, nbt, mk;
  Touched td, tbt;
  RowBlk<KT> f = readRowBlk<KT>(frow, 0, laneOff), nf; // the first block of delta: needed after the descending pass
  float tcarry = 0.f;
#pragma unroll
  for (int blk = NB - 1; blk >= 0; --blk) {
    FSMC_WAIT_OPERANDS(dg.waitCycles);
    if (blk == NB - 1) {
      landed(ops.u, ops.rr);
      if constexpr (kTouch && !SY) {
        heldRow<NLINES - 1>(ops.tu);
        heldRow<NLINES - 1>(ops.trr);
      }
      u = ops.u;
      rr = ops.rr;
      em = ops.em;
    } else {
      landed(nu, nrr);
      u = nu;
      rr = nrr;
      em = nem;
    }
    if (blk > 0) {
      nu = LD<kKB, SY>::loadAt(rowSet, kRowUsh * KPc + (blk - 1) * kKB);
      nrr = LD<kKB, SY>::loadAt(rowSet, kRowRR * KPc + (blk - 1) * kKB);
      nem = readEmis<kKB>(e, blk - 1);
    } else {
      d = LD<kKB, SY>::loadAt(rowSet, kRowD * KPc);
      bt = LD<kKB, SY>::loadAt(rowSet, kRowB * KPc);
      if constexpr (kTouch && !SY) {
        touchRow<1, NLINES - 1>(td, rowSet, kRowD * KPc);
        touchRow<1, NLINES - 1>(tbt, rowSet, kRowB * KPc);
      }
      if constexpr (GHOST && NB == 1) {
        mk = LD<kKB, SY>::loadAt(ghostMask, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sbi = R - 1; sbi >= 0; --sbi) {
      const int sb = blk * R + sbi;
      const int o = sbi * 8;
      if (sb * 8 >= K) {
        continue;
      }
      float T[9];
      T[8] = tcarry;
      // vec[k] = beta[k]*e[k] (kept in b), T[k] = U[k-1]*vec[k]
#pragma unroll
      for (int i = 0; i < 8; i += 2) {
        const int k = sb * 8 + i;
        if (k + 1 < K) {
          f32x2 v = {b[k], b[k + 1]};
          v = pmul(v, em.pair(o + i));
          const f32x2 t = pmul(pairOf(u, o + i), v);
          b[k] = v.x;
          b[k + 1] = v.y;
          T[i] = t.x;
          T[i + 1] = t.y;
        } else if (k < K) {
          b[k] = b[k] * em.at(o + i);
          T[i] = u[o + i] * b[k];
        }
      }
      // BU[k] = U[k]*vec[k+1] + RR[k]*BU[k+1], BU[K-1] = 0
#pragma unroll
      for (int i = 7; i >= 0; --i) {
        const int k = sb * 8 + i;
        if (k < K) {
          if (k == K - 1) {
            w[k] = 0.f;
          } else {
            w[k] = T[i + 1] + rr[o + i] * w[k + 1];
          }
        }
      }
      tcarry = T[0];
    }
  }
  // ascending: BL[k] = BL[k-1] + B[k-1]*vec[k-1];  beta'[k] = (BL[k] + D[k]*vec[k]) + BU[k];  the three sums
  float BL = 0.f;
  float sum = 0.f;
  down = 0.f;
  stay = 0.f;
  up = 0.f;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    FSMC_WAIT_OPERANDS(dg.waitCycles);
    if (blk > 0) {
      landed(nd, nbt);
      d = nd;
      bt = nbt;
      f = nf;
    } else {
      landed(d, bt);
      if constexpr (kTouch && !SY) {
        heldRow<NLINES - 1>(td);
        heldRow<NLINES - 1>(tbt);
      }
    }
    if constexpr (GHOST) {
      if (blk == NB - 1) {
        landed(mk);
      }
    }
    if (blk + 1 < NB) {
      nd = LD<kKB, SY>::loadAt(rowSet, kRowD * KPc + (blk + 1) * kKB);
      nbt = LD<kKB, SY>::loadAt(rowSet, kRowB * KPc + (blk + 1) * kKB);
      if constexpr (GHOST) {
        if (blk + 1 == NB - 1) {
          mk = LD<kKB, SY>::loadAt(ghostMask, (NB - 1) * kKB);
        }
      }
      nf = readRowBlk<KT>(frow, blk + 1, laneOff);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kKB; i += 2) {
      const int k = blk * kKB + i;
      if (k + 1 < K) {
        const f32x2 v = {b[k], b[k + 1]};
        const f32x2 dv = pmul(pairOf(d, i), v);
        const f32x2 bv = pmul(pairOf(bt, i), v);
        f32x2 bl;
        bl.x = BL;
        bl.y = BL + bv.x;
        f32x2 x = padd(bl, dv);
        const f32x2 bu = {w[k], w[k + 1]};
        x = padd(x, bu);
        if constexpr (GHOST) {
          if (blk == NB - 1) {
            x = pmul(x, pairOf(mk, i));
          }
        }
        const f32x2 fv = f.pair(i);
        const f32x2 pd = pmul(fv, bl);
        const f32x2 ps = pmul(fv, dv);
        const f32x2 pu = pmul(fv, bu);
        w[k] = x.x;
        w[k + 1] = x.y;
        sum = sum + x.x;
        sum = sum + x.y;
        down = down + pd.x;
        down = down + pd.y;
        stay = stay + ps.x;
        stay = stay + ps.y;
        up = up + pu.x;
        up = up + pu.y;
        BL = (k + 1 < K - 1) ? bl.y + bv.y : bl.y;
      } else if (k < K) {
        const float fk = f.at(i);
        const float dvk = d[i] * b[k];
        down = down + fk * BL;
        stay = stay + fk * dvk;
        up = up + fk * w[k];
        w[k] = (BL + dvk) + w[k];
        sum = sum + w[k];
        if (k < K - 1) {
          BL = BL + bt[i] * b[k];
        }
      }
    }
  }
  return sum;
}

// grid: any number of single-wave workgroups (one workspace slot each), no dynamic LDS.
template <int KT> __global__ __launch_bounds__(kWave, minWavesPerSimd(KT)) void transition_kernel(const TrnParams p)
{
  static_assert(KT >= 2 && KT <= 128, "a lane-per-pair member (fsmc_instances.h)");
  constexpr int KA = KT;
  using Sh = SweepShape<KT, 3>;
  constexpr bool SY = kTrnSyncLoads<KT>;

  __shared__ float4 ring[2][Sh::NC * Sh::E4];

  const int lane = threadIdx.x;
  const unsigned laneOff = threadIdx.x * (unsigned)sizeof(float4);
  const SweepParams sp = sweepParams(p);
  const cfloat_p tPi = (cfloat_p)sp.pi;
  const Tables tabs = {(cfloat_p)sp.rowSets, (cfloat_p)sp.cR, (cfloat_p)p.ghostMask};
  const int S = sp.S;
  const int C = p.chunk;
  const int nChunks = p.nChunks;
  char* const slot = p.ws + (size_t)blockIdx.x * p.slotBytes;
  char* const rowBuf = slot;
  char* const ckptBuf = slot + (size_t)C * Sh::kVecBytes; // (slot 0 belongs to no chunk: b waits there during a chunk's sweep)
  const int lastStart = (nChunks - 1) * C;       // sweep 1 keeps the rows from this site on

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

    float a[KA], w[KA]; // a: delta in the sweeps, b in the walk
    Diag dg;

    // one site of a forward sweep: delta of site pos in a, stored as row `r` of the buffer
    auto forwardSite = [&](const int pos, const int r) {
      const int c = obs.classAt(pos);
      const float4* er = &ring[pos & 1][c * Sh::E4];
      const float sum = forwardStep<KT, KA, SY>(a, w, er, tPi, tabs, stepRows, sp.stepRow, S, lane, pos, dg);
      scale_pk<KT, KA>(a, a, sum);
      store_vec<KT, KA>(KT, (float4*)(rowBuf + (size_t)r * Sh::kVecBytes), laneOff, a);
    };

    // the values of site t into this lane's two rows: four sites of each in registers, out as aligned float4 where the
    // row has four, as single floats at its ends
    const size_t rowFloat = pl.outIdx * (size_t)S; // this pair's first float of the slice's rows
    float4 qd = {0.f, 0.f, 0.f, 0.f}, qu = {0.f, 0.f, 0.f, 0.f};
    auto emit = [&](const int t, const float pd, const float pu) {
      const size_t A = rowFloat + (size_t)t;
      const unsigned ph = (unsigned)A & 3u;
      qd.x = ph == 0u ? pd : qd.x;
      qd.y = ph == 1u ? pd : qd.y;
      qd.z = ph == 2u ? pd : qd.z;
      qd.w = ph == 3u ? pd : qd.w;
      qu.x = ph == 0u ? pu : qu.x;
      qu.y = ph == 1u ? pu : qu.y;
      qu.z = ph == 2u ? pu : qu.z;
      qu.w = ph == 3u ? pu : qu.w;
      if ((ph == 0u || t == 0) && pl.valid) {
        const size_t D4 = A & ~(size_t)3;
        if (ph == 0u && t + 3 < S) {
          *(float4*)(p.down + D4) = qd;
          *(float4*)(p.up + D4) = qu;
        } else {
          const float vd[4] = {qd.x, qd.y, qd.z, qd.w}, vu[4] = {qu.x, qu.y, qu.z, qu.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const long long site = (long long)(D4 + (size_t)i) - (long long)rowFloat;
            if (site >= (long long)t && site < (long long)S) {
              p.down[D4 + (size_t)i] = vd[i];
              p.up[D4 + (size_t)i] = vu[i];
            }
          }
        }
      }
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

    // ---- the walk, chunk by chunk descending; every chunk but the last is swept again from its checkpoint first
    beta_init<KT, KA>(KT, p.K, a);
    for (int ch = nChunks - 1; ch >= 0; --ch) {
      const int lo = ch * C;
      const int hi = (lo + C < S ? lo + C : S) - 1; // the chunk's last site
      const int tlo = lo > 1 ? lo : 1;              // the walk's last site of the chunk
      if (hi < tlo) {
        continue; // (site 0 alone)
      }
      if (ch != nChunks - 1) {
        store_vec<KT, KA>(KT, (float4*)ckptBuf, laneOff, a); // b
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
        waitVm0();
        load_vec<KT, KA>(KT, (const float4*)ckptBuf, laneOff, a);
      }
      waitVm0(); // the chunk's rows are written
      stage(hi);
      for (int t = hi; t >= tlo; --t) {
        landedRows();
        if (t > tlo) {
          stage(t - 1); // into the slot of site t + 1, whose step is over
        }
        const int c = obs.classAt(t);
        const float4* er = &ring[t & 1][c * Sh::E4];
        const cfloat_p rowSet = rowSetOf<KT>(tabs, stepRows.at(sp.stepRow, S, lane, t));
        // delta of site t - 1: a row of the chunk, or the checkpoint in front of it
        const char* const fr = t > lo ? rowBuf + (size_t)(t - 1 - lo) * Sh::kVecBytes : ckptBuf + (size_t)ch * Sh::kVecBytes;
        BetaOps<KT> ops;
        beta_issue_pk<KT, SY>(ops, rowSet, er);
        float down, stay, up;
        const float sum = transition_core_pk<KT, KA, kGhost<KT>, SY>(a, w, ops, rowSet, er, tabs.ghostMask,
                                                                     uniformPtr(fr), laneOff, down, stay, up, dg);
        scale_pk<KT, KA>(a, w, sum);
        const float z = (down + stay) + up;
        const float r = 1.0f / z;
        emit(t, down * r, up * r);
      }
    }
    emit(0, 0.f, 0.f);
  }
}

} // namespace fsmc
