// drivers.hpp -- the two driver classes of the reference's API: ASMC (pair-list decode, ASMC.hpp/.cpp)
// and FastSMC (IBD detection, FastSMC.hpp/.cpp), as thin owners of Data + HMM.
#pragma once

#include <string>
#include <vector>

#include "hmm.hpp"

namespace fsmc_host
{

class ASMC
{
public:
  explicit ASMC(DecodingParams params);
  // ASMC.cpp:28-49: array mode, posterior sums + per-pair mean + MAP enabled
  ASMC(const std::string& inFileRoot, const std::string& decodingQuantFile, const std::string& outFileRoot = "");

  DecodingReturnValues decodeAllInJob(); // ASMC.cpp:51-78
  // ASMC.cpp:80-100: decode the listed pairs into the return structure.  `outputs` says what is stored (PairOutputs,
  // pair_outputs.hpp); its tailStates / tailSummaryStates are made here from tailTimes / tailSummaryTimes (generations,
  // tailStatesOf) and must come empty.  A request that is refused throws before the last call's results or any queued
  // work are touched.
  void decodePairs(const std::vector<unsigned long>& hapIndicesA, const std::vector<unsigned long>& hapIndicesB,
                   const PairOutputs& outputs = {});
  // ASMC.cpp:102-128: the same for "<individual ID>#<1|2>" strings
  void decodePairs(const std::vector<std::string>& hapIdsA, const std::vector<std::string>& hapIdsB,
                   const PairOutputs& outputs = {});
  // the state cut of a tail time T (generations): #{k : discretization[k] < (float)T}, the loop of
  // HMM::getStateThreshold (HMM.cpp:504-513); throws for a time no interval starts below
  std::vector<int> tailStatesOf(const std::vector<float>& tailTimes);
  DecodePairsReturnStruct getCopyOfResults() { return mHmm.getDecodePairsReturnStruct(); }
  const DecodePairsReturnStruct& getRefOfResults() { return mHmm.getDecodePairsReturnStruct(); }
  HMM& hmm() { return mHmm; }

private:
  DecodingParams mParams;
  HMM mHmm;
};

class FastSMC
{
public:
  explicit FastSMC(DecodingParams params);
  // FastSMC.cpp:34-39: decoding quantities at <in>.decodingQuantities.gz, FastSMC defaults
  FastSMC(const std::string& inFileRoot, const std::string& outFileRoot);
  void run(); // FastSMC.cpp:41-238
  HMM& hmm() { return mHmm; }
  std::string outputFileName() const { return mHmm.ibdFileName(mParams.jobs, mParams.jobInd); }

private:
  DecodingParams mParams;
  HMM mHmm;
};

} // namespace fsmc_host
