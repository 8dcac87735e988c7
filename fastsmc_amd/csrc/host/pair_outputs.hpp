// pair_outputs.hpp -- what a pair-list decode (ASMC.decodePairs) is asked for, and the structure it is returned in.
#pragma once

#include <string>
#include <tuple>
#include <vector>

namespace fsmc_host
{

// What one call wants stored: HMM holds the request of the call under way, the return structure a copy of the request it
// was sized for.  Everything off / empty asks for nothing.
struct PairOutputs {
  bool posteriors = false, sumOfPosteriors = false; // per pair [states][sites] / their sum over the pairs
  bool means = false, maps = false;                 // the [pairs][sites] posterior-mean / MAP rows (and their minima)
  // the four [sites] minima without the [pairs][sites] matrices (computed on the device, fsmc_decode_pair_minima)
  bool minMeans = false, minMaps = false;
  // per pair, summaries of the mean / MAP rows over bins of sites (fsmc_decode_pair_bins): bin b is sites
  // [siteBins[b], siteBins[b + 1])
  std::vector<int> siteBins;
  // per pair and site, where the posterior mass lies (fsmc_decode_pair_cdf): the sum of the posterior over the first
  // tailStates[j] states (tailTimes[j]: the time in generations the cut was made from), and the smallest state at which
  // that running sum reaches quantiles[j]
  // (the times are what the caller asked in, kept for the return structure to report; ASMC::decodePairs derives the
  // states from them and refuses a request that brings states of its own; HMM decodes from the states and never reads
  // the times, so its setters of states leave them as they were)
  std::vector<float> tailTimes;
  std::vector<int> tailStates;
  std::vector<float> quantiles;
  // the tail probabilities reduced on the device, their rows not stored (fsmc_decode_pair_tail_summaries): summed over
  // the pairs per site and, with siteBins, per pair the mean over each bin and, with siteWeights ([sites]), the weighted
  // sum over it
  std::vector<float> tailSummaryTimes;
  std::vector<int> tailSummaryStates;
  std::vector<float> siteWeights;
  // per pair, the likelihood of its observations as mantissa, exponent and logarithm, from the forward sweep alone
  // (fsmc_decode_pair_loglik); with siteBins also per bin, started afresh at the bin's first site
  bool logLikelihoods = false;
  // per pair, the most probable joint state sequence (the Viterbi path) and its probability as mantissa, exponent and
  // logarithm (fsmc_decode_pair_viterbi): models of at most 128 states, array mode
  bool viterbiPaths = false;
  // per pair, this many state sequences (1 ... 64; 0: none) drawn from the joint posterior over sequences with this seed
  // (fsmc_decode_pair_samples): models of at most 128 states, array mode
  int sampledPaths = 0;
  unsigned long long sampleSeed = 0;
  // per pair and site, the posterior probability that the state is lower / higher than at the site before
  // (fsmc_decode_pair_transitions): the [pairs][sites] rows, and / or their sums over bins of sites with edges of their
  // own (transitionBins[b], transitionBins[b + 1]); models of at most 128 states, array mode
  bool transitionRows = false;
  std::vector<int> transitionBins;

  // Throws what the ABI would refuse, with its messages: more than 8 tail states or quantiles, a cut outside [1, states],
  // a quantile outside (0, 1]; then the same for the tail summaries, and weights without cuts, not one a site or not
  // finite; then fewer than two bin edges, edges outside [0, sites] or not strictly ascending; then log-likelihoods of a
  // model of more than 128 states; then Viterbi paths of a model of more than 128 states or of a sequence-mode model;
  // then sampled paths outside 0 ... 64, of a model of more than 128 states or of a sequence-mode model; then change
  // probabilities of a model of more than 128 states or of a sequence-mode model, or with bad bin edges.
  void check(long sites, long states, bool sequence = false) const;

  // the minima come from the device where their rows are not stored (stored rows: finaliseCalculations, as ever)
  bool minMeansOnDevice() const { return minMeans && !means; }
  bool minMapsOnDevice() const { return minMaps && !maps; }
  bool cdf() const { return !tailStates.empty() || !quantiles.empty(); }
  bool transitions() const { return transitionRows || !transitionBins.empty(); }
  // anything at all that goes into the return structure
  bool any() const
  {
    return means || maps || posteriors || sumOfPosteriors || minMeansOnDevice() || minMapsOnDevice() ||
           !siteBins.empty() || cdf() || !tailSummaryStates.empty() || logLikelihoods || viterbiPaths ||
           sampledPaths != 0 || transitions();
  }
};

// DecodePairsReturnStruct.hpp:29-124; matrices row-major
struct DecodePairsReturnStruct {
  std::vector<std::tuple<unsigned long, std::string, unsigned long, std::string>> perPairIndices;
  std::vector<std::vector<float>> perPairPosteriors; // per pair [states][sites]
  std::vector<float> sumOfPosteriors;                // [states][sites]
  std::vector<float> perPairPosteriorMeans;          // [pairs][sites]
  std::vector<float> minPosteriorMeans;              // [sites]
  std::vector<int> argminPosteriorMeans;             // [sites]
  std::vector<int> perPairMAPs;                      // [pairs][sites]
  std::vector<int> minMAPs, argminMAPs;              // [sites]
  long numPairs = 0, numSites = 0, numStates = 0;
  // what the vectors were sized for: the bin edges, times, cuts, quantiles and weights the outputs below belong to
  PairOutputs request;
  // [pairs][bins], empty without bins
  std::vector<float> binMeanPosteriorMeans, binMinPosteriorMeans;
  std::vector<int> binArgminPosteriorMeans, binMinMAPs, binArgminMAPs;
  // [tails][pairs][sites] and [quantiles][pairs][sites]
  std::vector<float> perPairTailProbabilities;
  std::vector<int> perPairQuantileStates;
  // per site the fp64 sum over the pairs in pair order, [tails][sites]; per pair the mean over each bin and, with site
  // weights, the weighted sum over it, [tails][pairs][bins] (empty without bins / without weights)
  std::vector<double> sumOfTailProbabilities;
  std::vector<float> binTailMeans, binTailLengths;
  // the likelihood of each pair's observations: likelihood = mantissa * 2^exponent, logLikelihood = log(mantissa) +
  // exponent * ln 2 in fp64; [pairs], and with bins [pairs][bins]: the bin's observations given everything before it
  std::vector<double> perPairLikelihoodMantissas, perPairLogLikelihoods;
  std::vector<int> perPairLikelihoodExponents;
  std::vector<double> binLikelihoodMantissas, binLogLikelihoods;
  std::vector<int> binLikelihoodExponents;
  // the most probable joint state sequence of each pair, [pairs][sites], and its probability P(path, observations) =
  // mantissa * 2^exponent with its logarithm in fp64, [pairs]
  std::vector<unsigned char> perPairViterbiStates;
  std::vector<double> perPairViterbiMantissas, perPairViterbiLogProbabilities;
  std::vector<int> perPairViterbiExponents;
  // state sequences drawn from the joint posterior of each pair, [pairs][samples][sites]
  std::vector<unsigned char> perPairSampledStates;
  // the posterior probability that the state at a site is lower / higher than at the site before, [pairs][sites], and
  // their sums over the bins of request.transitionBins, [pairs][bins]
  std::vector<float> perPairDownProbabilities, perPairUpProbabilities;
  std::vector<float> binExpectedDowns, binExpectedUps;
  size_t numWritten = 0;

  void initialise(size_t nPairs, long sites, long states, const PairOutputs& outputs);
  void finaliseCalculations();
};

} // namespace fsmc_host
