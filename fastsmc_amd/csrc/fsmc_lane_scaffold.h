// fsmc_lane_scaffold.h -- what the lane-per-pair kernels share around their steps, once: decode_kernel (fsmc_kernels.h),
// decode_kernel_bidir (fsmc_kernels_bidir.h) and the pair sweeps (fsmc_pair_sweep.h).
//
// Lane = pair, one wave (or two) per group of <= 64 pairs: a lane's pair and its two haplotype rows (laneInGroup,
// hapRows) and the table row of a step, the indices of 64 consecutive sites held in one register (RowIndexBlock).  For every
// decode family: the group a batch of the sums over pairs decodes next (sumsGroupOf).  Force-inlined, in registers.
//
// Included by fsmc_kernels.h behind the helpers it needs (kWave, waitVm0), not on its own.
#pragma once

namespace fsmc
{

// kModeSums: one BATCH per wave (or workgroup) and launch: wave i writes the sums of batch groupBase + i into plane i, and
// the host adds the planes to the accumulator one after the other -- the reference's order, batch by batch
// (HMM.cpp:1054-1073).  A batch of more than 64 pairs is several consecutive groups (p.batchFirst: first group of every
// batch): the wave decodes them in turn, one a round, and every group continues the batch's running sums where the group
// before left them.  The group of this round, or p.nGroups when the batch is done.
__device__ __forceinline__ unsigned sumsGroupOf(const KParams& p, const unsigned round)
{
  if (p.batchFirst) {
    const cuint_p bf = (cuint_p)p.batchFirst;
    const unsigned g = bf[p.groupBase + blockIdx.x] + round;
    return g >= bf[p.groupBase + blockIdx.x + 1] ? (unsigned)p.nGroups : g;
  }
  return round == 0 ? (unsigned)p.groupBase + blockIdx.x : (unsigned)p.nGroups;
}

// This lane's pair of a group: whether the lane has one, and its index in the work list ...
struct LanePair {
  bool valid;
  unsigned pairIdx;
};
__device__ __forceinline__ LanePair laneInGroup(const unsigned firstPair, const int nPairsInGroup, const int lane)
{
  const bool valid = lane < nPairsInGroup;
  return LanePair{valid, firstPair + (valid ? (unsigned)lane : 0u)}; // (an idle lane repeats the group's first pair)
}
// ... and the two haplotype rows of a pair.
struct HapRows {
  const unsigned long long* rowA;
  const unsigned long long* rowB;
};
template <typename Params> __device__ __forceinline__ HapRows hapRows(const Params& p, const unsigned pairIdx)
{
  const fsmc_pair pr = p.pairs[pairIdx];
  return HapRows{p.haps + (size_t)pr.hap_a * p.W, p.haps + (size_t)pr.hap_b * p.W};
}

// Table rows: the indices of 64 consecutive sites of rows[0 .. S) sit in one register (lane = site % 64, one coalesced
// load per 64 sites; lanes beyond the last site repeat it) and are picked with v_readlane.  (As scalar loads, one per
// site, each was waited for on the spot -- the register allocator had no SGPR to keep it in flight -- a round trip to L2
// per site in the loop heads.)  The load is waited for here, once per 64 sites: otherwise the compiler, which cannot tell
// at the v_readlane whether this load is the pending one, waits for vmcnt(0) at EVERY site -- right behind the
// emission-row request that was just issued.
struct RowIndexBlock {
  int vec = 0, blk = -1; // (in this order: the other way round costs the kernels two registers a lane)
  __device__ __forceinline__ int at(const int* rows, const int S, const int lane, const int site)
  {
    const int b = site >> 6;
    if (__builtin_expect(b != blk, 0)) {
      const int idx = b * kWave + lane;
      vec = rows[idx < S ? idx : S - 1];
      blk = b;
      waitVm0();
    }
    return __builtin_amdgcn_readlane(vec, site & (kWave - 1));
  }
};

} // namespace fsmc
