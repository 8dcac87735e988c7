// fsmc_pair_sweep.h -- what surrounds a step in the per-pair sweep kernels, once: forward_kernel (fsmc_pair_loglik.h),
// viterbi_kernel (fsmc_pair_viterbi.h), sample_kernel (fsmc_pair_samples.h) and transition_kernel
// (fsmc_pair_transitions.h) are built from these pieces and keep only their own recurrences, walks and outputs.
//
// A sweep kernel: lane = pair, one wave per group, the waves of the launch pull groups from an atomic queue
// (pullGroup, pairLane).  Per site it needs the observation class of the lane's pair from the packed haplotype words
// (ObsWords), the emission rows of the site in a two-slot LDS ring fed by LDS-DMA one site ahead (stageRows,
// landedRows), and the table row of the step (RowIndexBlock).  The constants of a kernel of member KT are
// SweepShape<KT, NC>.  The first site is pi * emission, scaled (firstSite); the forward step behind the emission row
// (forwardInit at site 0, otherwise alpha_step and the ascending sum) is forwardStep, which sample_kernel and
// transition_kernel call (forward_kernel keeps the same lines in its loop: as a function they move its 16- and 32-state
// members across an occupancy step); the scaling sums are multiplied up as a mantissa / exponent pair (likelihoodTimes).
// A lane's pair and rows (laneInGroup, hapRows) and RowIndexBlock are fsmc_lane_scaffold.h's, shared with the decode
// kernels; the decode kernels keep their own observation words and emission ring.
//
// The checkpointed replay of viterbi_kernel, sample_kernel and transition_kernel, which walk a pair's sequence DOWN
// over what a sweep UP left per site (back-pointers, forward vectors) without a row for every site.  A wave's workspace
// slot is [chunk sites] rows of the kernel's row size, then one stored vector (store_vec) per chunk: the checkpoints.
// Sweep 1 runs the whole sequence; before the first step of every chunk but the first it stores the vector of the
// site before as that chunk's checkpoint; the rows of the LAST chunk stay in the buffer, the rows of every earlier chunk
// all land on the buffer's first row, which is rewritten later: no branch in the step (row = pos >= lastStart ? pos -
// lastStart : 0).  Then the chunks are walked descending; a chunk other than the last is first swept again from its
// checkpoint for its rows: the observation words start over (ObsWords::restart), nothing of the walk before is in
// flight when the ring is restarted (waitVm0), the checkpoint is loaded, the sites are staged one ahead as in sweep 1.
// Without rows (viterbi_kernel's probabilities alone) there are no checkpoints and lastStart = S.  The three kernels
// each write these loops out around their own step and walk: moved behind functions that take the step and the walk
// they compile to other register counts in several members (profiles/README.md, r23), so only the description is
// shared.  The planner's side is planReplay (fsmc_plan.h).
//
// State rows leave in aligned dwords of four sites (packState): a pair's row of S bytes starts wherever the row before
// ended, so neighbouring rows share a dword where S % 4 != 0; a dword goes out whole where all four bytes are the
// row's and byte by byte at the row's two ends.  transition_kernel applies the same rule to its two float rows (emit).
// Vector stores only.  Everything is force-inlined and lives in registers.
#pragma once

#include <hip/hip_runtime.h>

#include "fsmc_kernels.h"

namespace fsmc
{

// What every sweep kernel needs of its launch.
struct SweepParams {
  int S;       // sites
  int W;       // 64-bit words per haplotype row
  int nGroups; // groups of the slice
  unsigned pairBase; // first pair of the slice: the outputs are indexed by pair of the work list minus this
  const float* pi;      // [KP]
  const float* cR;      // [KP]
  const float* rowSets; // [rows][5][KP]
  const int* stepRow;   // [S] row of the (site) step into site q
  const float4* emis3;  // [S][3 or 4][KP/4]
  const unsigned long long* haps; // [nHaps][W]
  const fsmc_pair* pairs;
  const fsmc_group* groups; // the slice's first group
  unsigned* counter;        // head of the group queue
};
// FwdParams, VitParams, SmpParams and TrnParams are flat kernel arguments that carry these fields under these names,
// each at the place it always had (moving an argument moves the compiled kernels); the kernels read them through this
// view.
template <typename Params> __device__ __forceinline__ SweepParams sweepParams(const Params& p)
{
  return SweepParams{p.S,     p.W,    p.nGroups, p.pairBase, p.pi,     p.cR,     p.rowSets,
                     p.stepRow, p.emis3, p.haps,  p.pairs,    p.groups, p.counter};
}

// The shape of a sweep kernel of family member KT with NC emission rows a site (the observation classes; + the gap's
// in sequence mode).
template <int KT, int NC_> struct SweepShape {
  static constexpr int KPc = ((KT + kKPad - 1) / kKPad) * kKPad; // the member's padded states
  static constexpr int E4 = KPc / 4;                             // float4 per emission row: KP / 4 of the member's models
  static constexpr int NC = NC_;
  static constexpr int NL = (NC * E4 + kWave - 1) / kWave;       // DMA requests per site
  static constexpr int K4 = (KT + 3) / 4;
  static constexpr size_t kVecBytes = (size_t)K4 * kWave * sizeof(float4); // a stored vector (store_vec)
};

// The next group of the queue, wave-uniform (the slice is done when it is not below nGroups).
__device__ __forceinline__ unsigned pullGroup(unsigned* counter, const int lane)
{
  unsigned g = 0;
  if (lane == 0) {
    g = atomicAdd(counter, 1u);
  }
  return __builtin_amdgcn_readfirstlane(g);
}

// This lane's pair of group g: whether the lane has one, its index in the work list and in the slice's outputs, and
// its two haplotype rows.
struct PairLane {
  bool valid;
  unsigned pairIdx;
  size_t outIdx;
  const unsigned long long* rowA;
  const unsigned long long* rowB;
};
__device__ __forceinline__ PairLane pairLane(const SweepParams& p, const unsigned g, const int lane)
{
  const cuint_p gw = (cuint_p)(p.groups + (size_t)g);
  const LanePair lp = laneInGroup(gw[0], (int)gw[1], lane);
  const HapRows hap = hapRows(p, lp.pairIdx);
  return PairLane{lp.valid, lp.pairIdx, (size_t)(lp.pairIdx - p.pairBase), hap.rowA, hap.rowB};
}

// Observation class of a lane's pair at site q: 0 het, 1 hom major, 2 hom minor (obsIsZero / obsIsTwo of
// HMM.cpp:647-652 as a row select).  The two words of 64 sites are read once per 64 sites, or after restart() when a
// sweep starts somewhere else.
struct ObsWords {
  const unsigned long long* rowA;
  const unsigned long long* rowB;
  int wordIdx = -1;
  unsigned long long xw = 0, aw = 0;
  __device__ __forceinline__ int classAt(const int q)
  {
    const int wi = q >> 6;
    if (__builtin_expect(wi != wordIdx, 0)) {
      const unsigned long long wa = rowA[wi];
      const unsigned long long wb = rowB[wi];
      xw = wa ^ wb;
      aw = wa & wb;
      wordIdx = wi;
    }
    const int bit = q & 63;
    return ((xw >> bit) & 1ull) ? 0 : 1 + (int)((aw >> bit) & 1ull);
  }
  __device__ __forceinline__ void restart()
  {
    wordIdx = -1;
  }
};

// The n4 float4 of a site's emission rows at `rows` into the ring slot `slot` (NL requests of a wave, laneOff = 16 *
// lane): asynchronous, counted in vmcnt, visible to this wave's LDS reads behind a vmcnt wait that covers it
// (landedRows); the slot's previous rows must no longer be read.
template <int NL>
__device__ __forceinline__ void stageRows(const float4* rows, float4* slot, const int n4, const int lane,
                                          const unsigned laneOff)
{
  const gchar_p src = uniformPtr(rows);
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    if (lane + i * kWave < n4) {
      dmaToLds((gf32x4_p)(src + (size_t)i * (kWave * sizeof(float4)) + laneOff), slot + i * kWave);
    }
  }
}
// Every request so far has landed and this wave's LDS reads may see it.
__device__ __forceinline__ void landedRows()
{
  waitVm0();
  __builtin_amdgcn_wave_barrier();
  FSMC_GCN_ASM("" ::: "memory");
}

// alpha at the first site, NOT yet scaled, and its sum: the operations of alpha_init up to its 1.0f / sum
// (HMM.cpp:736-747), k ascending from 0.f.
template <int KT, int KA> __device__ __forceinline__ float forwardInit(float (&a)[KA], cfloat_p pi, const float4* e)
{
  float sum = 0.f;
  float4 ev = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if ((k & 3) == 0) {
      ev = e[k >> 2];
    }
    const float em = (k & 3) == 0 ? ev.x : (k & 3) == 1 ? ev.y : (k & 3) == 2 ? ev.z : ev.w;
    a[k] = pi[k] * em;
    sum = sum + a[k];
  }
  return sum;
}
// ... and scaled: the vector of the first site as every later step leaves it, and its sum.
template <int KT, int KA> __device__ __forceinline__ float firstSite(float (&a)[KA], cfloat_p pi, const float4* e)
{
  const float sum = forwardInit<KT, KA>(a, pi, e);
  scale_pk<KT, KA>(a, a, sum);
  return sum;
}

// One site of the forward sweep behind its emission row `er`: on entry a = delta of site pos - 1 (nothing at site 0),
// on exit a = the vector of site pos NOT yet scaled, the return value its sum -- forwardInit, or
// alpha_step<..., SCALE = false> with the table row of the step and the ascending sum of what it leaves.
template <int KT, int KA, bool SY>
__device__ __forceinline__ float forwardStep(float (&a)[KA], float (&w)[KA], const float4* er, cfloat_p tPi,
                                             const Tables& tabs, RowIndexBlock& stepRows, const int* stepRow, const int S,
                                             const int lane, const int pos, Diag& dg)
{
  if (__builtin_expect(pos == 0, 0)) {
    return forwardInit<KT, KA>(a, tPi, er);
  }
  alpha_step<KT, KA, false, SY>(KT, a, w, tabs, stepRows.at(stepRow, S, lane, pos), er, dg);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    sum = sum + a[k];
  }
  return sum;
}

// One site of the likelihood recurrence (fsmc_pair_loglik.h): (m, e) <- (m, e) * s.
__device__ __forceinline__ void likelihoodTimes(double& m, int& e, const double s)
{
  m = m * s;
  if (m != 0.0 && __builtin_isfinite(m)) {
    int de = 0;
    m = __builtin_frexp(m, &de);
    e += de;
  }
}

// The state x of site t into its byte of `acc`, the four states of the group under construction, and the group into the
// state rows `out` when t completes it; the return value: whether it did.  A row of S bytes starts at byte rowByte,
// wherever the row before ended, and is walked down: the aligned group of four is complete at its first byte and at
// the row's first site; a lane with a pair (`valid`) stores it as one dword where all four bytes are the row's,
// otherwise byte by byte what is the row's from site t on (neighbouring rows share a group where S % 4 != 0).
__device__ __forceinline__ bool packState(unsigned& acc, const unsigned x, unsigned char* const out, const size_t rowByte,
                                          const int t, const int S, const bool valid)
{
  const size_t A = rowByte + (size_t)t;
  const unsigned sh = 8u * ((unsigned)A & 3u);
  acc = (acc & ~(0xffu << sh)) | (x << sh);
  if (((unsigned)A & 3u) == 0u || t == 0) {
    const size_t D4 = A & ~(size_t)3;
    if (valid) {
      if (((unsigned)A & 3u) == 0u && t + 3 < S) {
        *(unsigned*)(out + D4) = acc;
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const long long site = (long long)(D4 + (size_t)b) - (long long)rowByte;
          if (site >= (long long)t && site < (long long)S) {
            out[D4 + (size_t)b] = (unsigned char)((acc >> (8 * b)) & 0xffu);
          }
        }
      }
    }
    return true;
  }
  return false;
}

} // namespace fsmc
