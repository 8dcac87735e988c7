// fsmc_site_consumers.h -- the consumers of a site's posterior that more than one decode kernel runs, once: the per-pair
// mean / MAP rows of the lane-per-pair kernels (decode_kernel, fsmc_kernels.h; decode_kernel_bidir,
// fsmc_kernels_bidir.h) and the writer of an IBD record of decode_kernel and decode_kernel_any (fsmc_kernels_any.h;
// decode_kernel_w2 computes the pair index of a record only when it keeps it and has the body written out).
// Force-inlined: the state arrays stay in registers.
//
// The combine, the dump and the sums over pairs of the two lane-per-pair kernels stay written out in both: as functions
// they compile to other code than in place, in some instantiations to more registers, spills or code.
//
// Included by fsmc_kernels.h behind the helpers it needs (segment_ages), not on its own.
#pragma once

namespace fsmc
{

// HMM::writePerPairOutput (HMM.cpp:1378-1409): mean = sum_k post * E[t_k] (k ascending from 0.f), MAP = first strictly
// larger posterior.  coal: the expected coalescence times in LDS (as scalar loads -- one per state, all live at once:
// hundreds of spilled scalars -- the 128-state member of decode_kernel_bidir returned wrong and, with several groups,
// irreproducible means; with the times in LDS it is bit-equal like the others).
template <int KT, int KA>
__device__ __forceinline__ void consumePerPair(const float (&w)[KA], const float cq, const float* coal, const bool valid,
                                               const unsigned pairIdx, const int pos, const KParams& p)
{
  float mean = 0.f;
  float best = 0.f;
  int arg = 0;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    const float post = w[k] * cq;
    mean = mean + post * coal[k];
    if (best < post) {
      arg = k;
      best = post;
    }
  }
  if (valid) {
    if (p.ppMean) p.ppMean[(size_t)pairIdx * p.S + pos] = mean;
    if (p.ppMap) p.ppMap[(size_t)pairIdx * p.S + pos] = arg;
  }
}

// One IBD record: the segment [s0, s1] of pair pairIdx with posterior acc and, with TRACK, the age estimates from the
// lane's per-state posterior sums `sps` (HMM.cpp:1087-1107).  The cold path, run only when a segment closes.
template <bool TRACK>
__device__ __forceinline__ void emitIbdRecord(const KParams& p, const int K, const float4* sps, cfloat_p pi, cfloat_p expT,
                                              const unsigned pairIdx, const int s0, const int s1, const float acc)
{
  const unsigned idx = atomicAdd(&p.counters[1], 1u);
  float mean = 0.f, mapv = 0.f;
  if constexpr (TRACK) {
    segment_ages(K, p.ageThr, sps, pi, expT, (p.flags & FSMC_WANT_MEAN) != 0, (p.flags & FSMC_WANT_MAP) != 0, mean, mapv);
  }
  if (idx < p.recCap) {
    fsmc_ibd_record r;
    r.pair = pairIdx;
    r.start = s0;
    r.end = s1;
    r.prob = acc;
    r.post_mean = mean;
    r.map = mapv;
    p.recs[idx] = r;
  }
}

} // namespace fsmc
