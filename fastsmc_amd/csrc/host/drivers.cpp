#include "drivers.hpp"

#include "hashing.hpp"

#include <stdexcept>

namespace fsmc_host
{

namespace
{
// (in the member-initialiser list, before Data reads the files: the device comes up while the host parses)
DecodingParams withDeviceStarting(DecodingParams p)
{
  warmUpDevice(p.gpuDevice);
  return p;
}
} // namespace

ASMC::ASMC(DecodingParams params) : mParams(withDeviceStarting(std::move(params))), mHmm(Data(mParams), mParams) {}

ASMC::ASMC(const std::string& inFileRoot, const std::string& decodingQuantFile, const std::string& outFileRoot)
    : mParams(inFileRoot, decodingQuantFile, outFileRoot.empty() ? inFileRoot : outFileRoot, 1, 1, "array", false,
              true, false, false, 0.f, false, true, false, "", false, true, true),
      mHmm(Data(mParams), mParams)
{
}

DecodingReturnValues ASMC::decodeAllInJob()
{
  mHmm.decodeAll(mParams.jobs, mParams.jobInd);
  return mHmm.getDecodingReturnValues();
}

void ASMC::decodePairs(const std::vector<unsigned long>& hapIndicesA, const std::vector<unsigned long>& hapIndicesB,
                       const PairOutputs& outputs)
{
  if (hapIndicesA.empty() || hapIndicesA.size() != hapIndicesB.size()) {
    throw std::runtime_error("Vector of A indices (" + std::to_string(hapIndicesA.size()) +
                             ") must be the same size as vector of B indices (" +
                             std::to_string(hapIndicesB.size()) + ").\n");
  }
  if (!outputs.tailStates.empty() || !outputs.tailSummaryStates.empty()) {
    throw std::runtime_error("tail states are derived from the tail times: leave them empty");
  }
  // (first: arguments these refuse leave the last call's results as they are)
  PairOutputs o = outputs;
  o.tailStates = tailStatesOf(o.tailTimes);
  o.tailSummaryStates = tailStatesOf(o.tailSummaryTimes);
  if (!o.siteWeights.empty() && o.siteBins.empty()) {
    throw std::runtime_error("site weights need site bins");
  }
  mHmm.setPairOutputs(o);
  mHmm.getDecodePairsReturnStruct().initialise(hapIndicesA.size(), mHmm.getData().sites,
                                               mHmm.getDecodingQuantities().states, o);
  mHmm.decodeHapPairs(hapIndicesA, hapIndicesB);
  mHmm.finishDecoding();
  mHmm.getDecodePairsReturnStruct().finaliseCalculations();
}

void ASMC::decodePairs(const std::vector<std::string>& hapIdsA, const std::vector<std::string>& hapIdsB,
                       const PairOutputs& outputs)
{
  if (hapIdsA.size() != hapIdsB.size()) {
    throw std::runtime_error("Vector of A IDs (" + std::to_string(hapIdsA.size()) +
                             ") must be the same size as vector of B IDs (" + std::to_string(hapIdsB.size()) + ").\n");
  }
  std::vector<unsigned long> a(hapIdsA.size()), b(hapIdsB.size());
  const auto& ids = mHmm.getData().IIDList;
  for (size_t i = 0; i < hapIdsA.size(); ++i) {
    const auto [strA, hapA] = combinedIdToIndPlusHap(hapIdsA[i]);
    const auto [strB, hapB] = combinedIdToIndPlusHap(hapIdsB[i]);
    a[i] = dipToHapId(getIndIdxFromIdString(ids, strA), hapA);
    b[i] = dipToHapId(getIndIdxFromIdString(ids, strB), hapB);
  }
  decodePairs(a, b, outputs);
}

std::vector<int> ASMC::tailStatesOf(const std::vector<float>& tailTimes)
{
  const auto& dq = mHmm.getDecodingQuantities();
  std::vector<int> cuts;
  for (const float t : tailTimes) {
    int c = 0;
    while (c < static_cast<int>(dq.states) && dq.discretization[static_cast<size_t>(c)] < t) {
      c++;
    }
    if (c == 0) {
      throw std::runtime_error("tail time " + std::to_string(t) + ": no interval of the discretization starts below it");
    }
    cuts.push_back(c);
  }
  return cuts;
}

FastSMC::FastSMC(DecodingParams params) : mParams(withDeviceStarting(std::move(params))), mHmm(Data(mParams), mParams) {}

FastSMC::FastSMC(const std::string& inFileRoot, const std::string& outFileRoot)
    : mParams(withDeviceStarting(DecodingParams(inFileRoot, inFileRoot + ".decodingQuantities.gz", outFileRoot, true))),
      mHmm(Data(mParams), mParams)
{
}

void FastSMC::run()
{
  mHmm.decodeAll(mParams.jobs, mParams.jobInd);
  if (!mParams.hashing) {
    mHmm.closeIBDFile();
    return;
  }
  // identification step: candidate (pair, window)s -> HMM::decodeFromHashing (FastSMC.cpp:118-235)
  runHashing(mHmm.getData(), mParams, mHmm);
  mHmm.finishFromHashing();
}

} // namespace fsmc_host
