// fsmc_pair_layout.h -- where the fsmc_decode_pair_* entry points keep what on the device: for each of the eight, the
// bytes a group of the work list takes (what plan::planSlices cuts the list by), and, once the slices are known, the
// sizes of the staging, row and spec buffers and every region's offset inside the entry point's accumulator buffer.
//
// Deciding, not doing, as fsmc_plan.h: pure arithmetic on plain sizes and flags.  Nothing here knows the device's
// runtime, a kernel, the context or the environment.  An entry point asks for its layout once, allocates the totals and
// forms every device pointer as base + offset, so a size and the placement it has to hold cannot disagree.
// tests/pair_layout_driver.cpp runs these functions on a CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "fsmc_plan.h"

namespace fsmc
{
namespace layout
{
constexpr size_t kLanes = (size_t)plan::kWave; // pairs of a full group
constexpr size_t kSpecBytes = 8;               // sizeof(PairCdfSpec), fsmc_pair_cdf.h (the library's host side asserts it)

// Blocks of 64 sites: a wave of the reductions owns one.
inline size_t siteBlocks(size_t S) { return (S + kLanes - 1) / kLanes; }
// Groups a slice may have where a reduction's grid is groups x site blocks (cdf, tail summaries).
inline size_t sliceMostBySiteBlocks(size_t S) { return (size_t)INT32_MAX / siteBlocks(S); }
// A full group's dump in the staging buffer, [site][k][lane] floats.
inline size_t dumpGroupBytes(size_t K, size_t S) { return kLanes * K * S * sizeof(float); }
inline size_t roundUp8(size_t bytes) { return (bytes + 7) / 8 * 8; }

// ---- posteriors: ppAcc = [expCoal, K floats][sum, K x S floats] ------------------------------------------------------
struct Posteriors {
  size_t groupBytes = 0; // a group in the staging buffer; and its rows, at most, where rows are wanted
  size_t stageBytes = 0; // ppStage: a slice's dump
  size_t rowBytes = 0;   // one pair's table, [K][S] floats
  size_t rowsBytes = 0;  // ppRows: the largest slice's tables (0: no rows wanted, the buffer is left alone)
  size_t offCoal = 0, offSum = 0, accBytes = 0;
};
inline size_t posteriorsGroupBytes(size_t K, size_t S, bool wantRows)
{
  return dumpGroupBytes(K, S) * (wantRows ? 2 : 1);
}
inline Posteriors posteriors(size_t K, size_t S, bool wantRows, size_t slice, size_t slicePairsMax)
{
  const size_t plane = K * S; // floats of one pair's table, and of the sum
  Posteriors L;
  L.groupBytes = posteriorsGroupBytes(K, S, wantRows);
  L.stageBytes = slice * dumpGroupBytes(K, S);
  L.rowBytes = plane * sizeof(float);
  L.rowsBytes = wantRows ? slicePairsMax * L.rowBytes : 0;
  L.offCoal = 0;
  L.offSum = K * sizeof(float);
  L.accBytes = L.offSum + plane * sizeof(float);
  return L;
}

// ---- minima: pmAcc = [expCoal, KP floats][the carried state, 4 x S][the ranges' partials, 4 x rangesMax x S] -----------
// The ranges: a wave owns 64 sites of one range.  A large slice is cut so that every SIMD of the chip gets a few waves
// (4 x 4 x CUs of them over the site blocks), a range no shorter than 16 pairs: the partials stay a small fraction of
// the rows.  FSMC_DIAG_MINIMA_RANGE=<pairs> (plan::Diag::minimaRange) -- tests: several ranges on a small problem.
struct Minima {
  size_t groupBytes = 0; // a full group's rows in the staging buffer
  size_t siteBlocks = 0;
  size_t rangeLen = 0, rangesMax = 0;
  bool tooManyRanges = false; // ranges x site blocks beyond one launch's grid
  size_t stageBytes = 0;      // ppStage: the largest slice's mean and / or MAP rows
  size_t vec = 0;             // one [S] vector of floats or int32s
  // min of the means, its argmin, min of the MAPs, its argmin: the state, then the partials in the same order
  size_t offCoal = 0, offState[4] = {0, 0, 0, 0}, offParts[4] = {0, 0, 0, 0}, accBytes = 0;
};
inline size_t minimaGroupBytes(size_t S, size_t nOut) { return kLanes * S * sizeof(float) * nOut; }
inline Minima minima(int nCU, size_t S, size_t KP, size_t nOut, size_t slicePairsMax, const plan::Diag& diag)
{
  Minima L;
  L.groupBytes = minimaGroupBytes(S, nOut);
  L.siteBlocks = siteBlocks(S);
  const size_t wavesWanted = (size_t)16 * (size_t)nCU;
  const size_t rangesWanted = std::max<size_t>(1, (wavesWanted + L.siteBlocks - 1) / L.siteBlocks);
  L.rangeLen = std::max<size_t>(16, (slicePairsMax + rangesWanted - 1) / rangesWanted);
  L.rangeLen = plan::lowered(L.rangeLen, diag.minimaRange);
  L.rangesMax = (slicePairsMax + L.rangeLen - 1) / L.rangeLen;
  L.tooManyRanges = L.rangesMax * L.siteBlocks > (size_t)INT32_MAX;
  L.stageBytes = slicePairsMax * S * sizeof(float) * nOut;
  L.vec = S * sizeof(float);
  L.offCoal = 0;
  const size_t coalBytes = KP * sizeof(float);
  for (size_t i = 0; i < 4; ++i) {
    L.offState[i] = coalBytes + i * L.vec;
    L.offParts[i] = coalBytes + 4 * L.vec + i * L.rangesMax * L.vec;
  }
  L.accBytes = coalBytes + 4 * L.vec + 4 * L.rangesMax * L.vec;
  return L;
}

// ---- bins: pbAcc = [expCoal, KP floats][edges, B + 1][a slice's outputs, those asked for, pairs x B each] ---------------
struct Bins {
  static constexpr int kOutputs = 5; // mean, min of the means, its argmin, min of the MAPs, its argmin
  size_t groupBytes = 0; // a full group's rows in the staging buffer and its cells in the output buffer
  size_t stageBytes = 0; // ppStage: the largest slice's mean and / or MAP rows
  size_t edgeBytes = 0;
  size_t outBytes = 0;   // one output of the largest slice
  size_t offCoal = 0, offEdges = 0, offOut[kOutputs] = {0, 0, 0, 0, 0}, accBytes = 0; // (offOut of an output not asked for: unused)
};
inline size_t binsGroupBytes(size_t S, size_t B, size_t nRows, size_t nOut)
{
  return kLanes * sizeof(float) * (S * nRows + B * nOut);
}
inline Bins bins(size_t S, size_t KP, size_t B, size_t nRows, const bool (&want)[Bins::kOutputs], size_t slicePairsMax)
{
  size_t nOut = 0;
  for (bool w : want) {
    nOut += w ? 1 : 0;
  }
  Bins L;
  L.groupBytes = binsGroupBytes(S, B, nRows, nOut);
  L.stageBytes = slicePairsMax * S * sizeof(float) * nRows;
  L.edgeBytes = (B + 1) * sizeof(int32_t);
  L.outBytes = slicePairsMax * B * sizeof(float);
  L.offCoal = 0;
  L.offEdges = KP * sizeof(float);
  size_t next = L.offEdges + L.edgeBytes;
  for (int i = 0; i < Bins::kOutputs; ++i) {
    L.offOut[i] = next;
    next += want[i] ? L.outBytes : 0;
  }
  L.accBytes = next;
  return L;
}

// ---- log-likelihoods: plAcc = a slice's [mant][bin mant] doubles, [expo][bin expo] ints, then the edges, B + 1 --------
struct Loglik {
  size_t groupBytes = 0;
  size_t edgeBytes = 0;
  size_t offMant = 0, offBinMant = 0, offExpo = 0, offBinExpo = 0, offEdges = 0, accBytes = 0;
};
inline size_t loglikGroupBytes(size_t B) { return kLanes * (sizeof(double) + sizeof(int32_t)) * (1 + B); }
inline Loglik loglik(size_t B, size_t slicePairsMax)
{
  const size_t n = slicePairsMax;
  Loglik L;
  L.groupBytes = loglikGroupBytes(B);
  L.edgeBytes = (B + 1) * sizeof(int32_t);
  L.offMant = 0;
  L.offBinMant = n * sizeof(double);
  L.offExpo = L.offBinMant + n * B * sizeof(double);
  L.offBinExpo = L.offExpo + n * sizeof(int32_t);
  L.offEdges = L.offBinExpo + n * B * sizeof(int32_t);
  L.accBytes = L.offEdges + L.edgeBytes;
  return L;
}

// ---- Viterbi paths: pvAcc = a slice's [mant] doubles, [expo] ints; its state rows, [pair][S] bytes, are in ppRows -------
struct Viterbi {
  size_t groupBytes = 0;
  size_t rowsBytes = 0; // ppRows (where states are wanted): the largest slice's rows, whole dwords
  size_t offMant = 0, offExpo = 0, accBytes = 0; // (where the probabilities are wanted)
};
inline size_t viterbiGroupBytes(size_t S, bool wantStates, bool wantProb)
{
  return kLanes * ((wantStates ? S : 0) + (wantProb ? sizeof(double) + sizeof(int32_t) : 0));
}
inline Viterbi viterbi(size_t S, bool wantStates, bool wantProb, size_t slicePairsMax)
{
  const size_t n = slicePairsMax;
  Viterbi L;
  L.groupBytes = viterbiGroupBytes(S, wantStates, wantProb);
  L.rowsBytes = (n * S + 3) / 4 * 4;
  L.offMant = 0;
  L.offExpo = n * sizeof(double);
  L.accBytes = L.offExpo + n * sizeof(int32_t);
  return L;
}

// ---- sampled paths: no accumulator; a slice's state rows, [pair][sample][S] bytes, are in ppRows -----------------------
struct Samples {
  size_t groupBytes = 0;
  size_t pairBytes = 0; // one pair's rows
  size_t rowsBytes = 0; // ppRows: the largest slice's rows, whole dwords
};
inline size_t samplesGroupBytes(size_t S, size_t nSamples) { return kLanes * nSamples * S; }
inline Samples samples(size_t S, size_t nSamples, size_t slicePairsMax)
{
  Samples L;
  L.groupBytes = samplesGroupBytes(S, nSamples);
  L.pairBytes = nSamples * S;
  L.rowsBytes = (slicePairsMax * L.pairBytes + 3) / 4 * 4;
  return L;
}

// ---- change probabilities: ppRows = [down | up][pair of slice, a multiple of four][S] floats (both halves start on 16
// bytes); pxAcc = [edges, B + 1][weights, S ones][a slice's bin outputs, 2 x pairs x B] where bins are wanted ------------
struct Transitions {
  size_t groupBytes = 0;
  size_t rowsPerOut = 0; // rows of one direction in ppRows
  size_t rowsBytes = 0;  // ppRows
  size_t outBytes = 0;   // the bin cells of both directions, the largest slice
  size_t offEdges = 0, offWeights = 0, offBins = 0, accBytes = 0;
};
inline size_t transitionsGroupBytes(size_t S, size_t B) { return kLanes * 2 * sizeof(float) * (S + B); }
inline Transitions transitions(size_t S, size_t B, size_t slicePairsMax)
{
  Transitions L;
  L.groupBytes = transitionsGroupBytes(S, B);
  L.rowsPerOut = (slicePairsMax + 3) / 4 * 4;
  L.rowsBytes = 2 * L.rowsPerOut * S * sizeof(float);
  L.outBytes = 2 * L.rowsPerOut * B * sizeof(float);
  L.offEdges = 0;
  L.offWeights = B ? roundUp8((B + 1) * sizeof(int32_t)) : 0;
  L.offBins = L.offWeights + (B ? roundUp8(S * sizeof(float)) : 0);
  L.accBytes = L.offBins + L.outBytes;
  return L;
}

// ---- tails and quantiles: no accumulator; ppRows =[output][pair of slice][S] ----------------------------------------
struct Cdf {
  size_t groupBytes = 0; // a group in the staging buffer and its rows, at most
  size_t stageBytes = 0; // ppStage: a slice's dump
  size_t outCells = 0;   // cells of one output of the largest slice
  size_t rowsBytes = 0;  // ppRows
  size_t specBytes = 0;  // pcSpec
};
inline size_t cdfGroupBytes(size_t K, size_t S, size_t nOut)
{
  return dumpGroupBytes(K, S) + kLanes * S * sizeof(float) * nOut;
}
inline Cdf cdf(size_t K, size_t S, size_t nOut, size_t slice, size_t slicePairsMax)
{
  Cdf L;
  L.groupBytes = cdfGroupBytes(K, S, nOut);
  L.stageBytes = slice * dumpGroupBytes(K, S);
  L.outCells = slicePairsMax * S;
  L.rowsBytes = nOut * L.outCells * sizeof(float);
  L.specBytes = nOut * kSpecBytes;
  return L;
}

// ---- tail summaries: ptAcc = [sum, n_tail x S doubles][edges, B + 1][weights, S][a slice's outputs, up to 2 x n_tail x
// pairs x B]; edges and weights take whole 8 bytes, and no room where they are not wanted (B: 0 without bin outputs) -----
struct Tail {
  size_t groupBytes = 0; // a group in the staging buffer, its rows and its cells in the output buffer
  size_t stageBytes = 0; // ppStage: a slice's dump
  size_t rowsBytes = 0;  // ppRows: [cut][pair of slice][S]
  size_t specBytes = 0;  // pcSpec
  size_t sumBytes = 0;
  size_t outBytes = 0;   // one output of the largest slice, every cut
  size_t offSum = 0, offEdges = 0, offWeights = 0, offMean = 0, offLength = 0, accBytes = 0;
};
inline size_t tailGroupBytes(size_t K, size_t S, size_t nTail, size_t B, bool wantMean, bool wantLength)
{
  const size_t nBinOut = (wantMean ? 1 : 0) + (wantLength ? 1 : 0);
  return dumpGroupBytes(K, S) + kLanes * sizeof(float) * nTail * (S + B * nBinOut);
}
inline Tail tail(size_t K, size_t S, size_t nTail, size_t B, bool wantMean, bool wantLength, size_t slice,
                 size_t slicePairsMax)
{
  const bool wantBins = wantMean || wantLength;
  Tail L;
  L.groupBytes = tailGroupBytes(K, S, nTail, B, wantMean, wantLength);
  L.stageBytes = slice * dumpGroupBytes(K, S);
  L.rowsBytes = nTail * slicePairsMax * S * sizeof(float);
  L.specBytes = nTail * kSpecBytes;
  L.sumBytes = nTail * S * sizeof(double);
  L.outBytes = nTail * slicePairsMax * B * sizeof(float);
  const size_t edgeBytes = wantBins ? roundUp8((B + 1) * sizeof(int32_t)) : 0;
  const size_t weightBytes = wantLength ? roundUp8(S * sizeof(float)) : 0;
  L.offSum = 0;
  L.offEdges = L.sumBytes;
  L.offWeights = L.offEdges + edgeBytes;
  L.offMean = L.offWeights + weightBytes;
  L.offLength = L.offMean + (wantMean ? L.outBytes : 0);
  L.accBytes = L.offLength + (wantLength ? L.outBytes : 0);
  return L;
}
} // namespace layout
} // namespace fsmc
