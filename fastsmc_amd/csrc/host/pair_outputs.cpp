// pair_outputs.cpp -- the request of a pair-list decode checked, and its return structure sized and finished.
#include "pair_outputs.hpp"

#include <cmath>
#include <stdexcept>

namespace fsmc_host
{

namespace
{
void checkTailCount(const std::vector<int>& cuts)
{
  if (cuts.size() > 8) {
    throw std::runtime_error("at most 8 tail states a call");
  }
}

void checkTailRange(const std::vector<int>& cuts, long states)
{
  for (const int c : cuts) {
    if (c < 1 || c > static_cast<int>(states)) {
      throw std::runtime_error("tail state " + std::to_string(c) + " outside [1, K]");
    }
  }
}

// column-wise min / first argmin of a stored [pairs][sites] matrix (DecodePairsReturnStruct.hpp:105-118)
template <typename T>
void firstMinima(const std::vector<T>& rows, long pairs, long sites, std::vector<T>& min, std::vector<int>& argmin)
{
  for (long s = 0; !rows.empty() && s < sites; ++s) {
    long arg = 0;
    T best = rows[static_cast<size_t>(s)];
    for (long p = 1; p < pairs; ++p) {
      const T v = rows[static_cast<size_t>(p * sites + s)];
      if (v < best) {
        best = v;
        arg = p;
      }
    }
    min[static_cast<size_t>(s)] = best;
    argmin[static_cast<size_t>(s)] = static_cast<int>(arg);
  }
}
} // namespace

void PairOutputs::check(long sites, long states, bool sequence) const
{
  // (the messages of fsmc_decode_pair_cdf)
  checkTailCount(tailStates);
  if (quantiles.size() > 8) {
    throw std::runtime_error("at most 8 quantiles a call");
  }
  checkTailRange(tailStates, states);
  for (const float q : quantiles) {
    if (!std::isfinite(q) || !(q > 0.f) || q > 1.f) {
      throw std::runtime_error("quantile " + std::to_string(q) + " not finite or outside (0, 1]");
    }
  }
  // (the messages of fsmc_decode_pair_tail_summaries)
  checkTailCount(tailSummaryStates);
  checkTailRange(tailSummaryStates, states);
  if (!siteWeights.empty()) {
    if (tailSummaryStates.empty()) {
      throw std::runtime_error("site weights need tail summary times");
    }
    if (siteWeights.size() != static_cast<size_t>(sites)) {
      throw std::runtime_error("site weights: " + std::to_string(siteWeights.size()) + " values for " +
                               std::to_string(sites) + " sites");
    }
    for (size_t t = 0; t < siteWeights.size(); ++t) {
      if (!std::isfinite(siteWeights[t])) {
        throw std::runtime_error("site weight " + std::to_string(t) + " is not finite");
      }
    }
  }
  if (!siteBins.empty()) { // (the messages of fsmc_decode_pair_bins)
    if (siteBins.size() < 2) {
      throw std::runtime_error("need one bin at least (n_bins + 1 edges)");
    }
    if (siteBins.front() < 0 || static_cast<long>(siteBins.back()) > sites) {
      throw std::runtime_error("bin edges must lie in [0, sites]");
    }
    for (size_t b = 0; b + 1 < siteBins.size(); ++b) {
      if (siteBins[b] >= siteBins[b + 1]) {
        throw std::runtime_error("bin edges must be strictly ascending");
      }
    }
  }
  if (logLikelihoods && states > 128) { // (the message of fsmc_decode_pair_loglik)
    throw std::runtime_error("per-pair log-likelihoods: no forward kernel for a model of more than 128 states (" +
                             std::to_string(states) + ")");
  }
  if (viterbiPaths && states > 128) { // (the messages of fsmc_decode_pair_viterbi)
    throw std::runtime_error("per-pair Viterbi paths: no Viterbi kernel for a model of more than 128 states (" +
                             std::to_string(states) + ")");
  }
  if (viterbiPaths && sequence) {
    throw std::runtime_error("per-pair Viterbi paths: no Viterbi kernel for a sequence-mode model");
  }
  if (sampledPaths < 0 || sampledPaths > 64) { // (the messages of fsmc_decode_pair_samples)
    throw std::runtime_error("sampled paths: n_samples must be 1 ... 64 (" + std::to_string(sampledPaths) + ")");
  }
  if (sampledPaths && states > 128) {
    throw std::runtime_error("sampled paths: no sampling kernel for a model of more than 128 states (" +
                             std::to_string(states) + ")");
  }
  if (sampledPaths && sequence) {
    throw std::runtime_error("sampled paths: no sampling kernel for a sequence-mode model");
  }
  if (transitions() && states > 128) { // (the messages of fsmc_decode_pair_transitions)
    throw std::runtime_error("change probabilities: no transition kernel for a model of more than 128 states (" +
                             std::to_string(states) + ")");
  }
  if (transitions() && sequence) {
    throw std::runtime_error("change probabilities: no transition kernel for a sequence-mode model");
  }
  if (!transitionBins.empty()) {
    if (transitionBins.size() < 2) {
      throw std::runtime_error("need one bin at least (n_bins + 1 edges)");
    }
    if (transitionBins.front() < 0 || static_cast<long>(transitionBins.back()) > sites) {
      throw std::runtime_error("bin edges must lie in [0, sites]");
    }
    for (size_t b = 0; b + 1 < transitionBins.size(); ++b) {
      if (transitionBins[b] >= transitionBins[b + 1]) {
        throw std::runtime_error("bin edges must be strictly ascending");
      }
    }
  }
}

void DecodePairsReturnStruct::initialise(size_t nPairs, long sites, long states, const PairOutputs& outputs)
{
  request = outputs;
  const PairOutputs& o = request;
  numWritten = 0;
  numPairs = static_cast<long>(nPairs);
  numSites = sites;
  numStates = states;
  const size_t S = static_cast<size_t>(sites), K = static_cast<size_t>(states);
  perPairIndices.assign(nPairs, {});
  perPairPosteriors.assign(o.posteriors ? nPairs : 0, std::vector<float>(o.posteriors ? K * S : 0));
  sumOfPosteriors.assign(o.sumOfPosteriors ? K * S : 0, 0.f);
  // the [sites] minima go with their [pairs][sites] matrix, or stand alone
  perPairPosteriorMeans.assign(o.means ? nPairs * S : 0, 0.f);
  minPosteriorMeans.assign(o.means || o.minMeans ? S : 0, 0.f);
  argminPosteriorMeans.assign(o.means || o.minMeans ? S : 0, 0);
  perPairMAPs.assign(o.maps ? nPairs * S : 0, 0);
  minMAPs.assign(o.maps || o.minMaps ? S : 0, 0);
  argminMAPs.assign(o.maps || o.minMaps ? S : 0, 0);
  // the per-pair summaries over bins of sites: [pairs][bins]
  const size_t cells = o.siteBins.size() < 2 ? 0 : nPairs * (o.siteBins.size() - 1);
  binMeanPosteriorMeans.assign(cells, 0.f);
  binMinPosteriorMeans.assign(cells, 0.f);
  binArgminPosteriorMeans.assign(cells, 0);
  binMinMAPs.assign(cells, 0);
  binArgminMAPs.assign(cells, 0);
  // the per-pair tail probabilities and quantile states: [outputs][pairs][sites]
  perPairTailProbabilities.assign(o.tailStates.size() * nPairs * S, 0.f);
  perPairQuantileStates.assign(o.quantiles.size() * nPairs * S, 0);
  // the tail probabilities reduced over pairs, [tails][sites], and over bins, [tails][pairs][bins]
  sumOfTailProbabilities.assign(o.tailSummaryStates.size() * S, 0.0);
  binTailMeans.assign(o.tailSummaryStates.size() * cells, 0.f);
  binTailLengths.assign(o.siteWeights.empty() ? 0 : o.tailSummaryStates.size() * cells, 0.f);
  // the likelihoods: [pairs] and [pairs][bins]
  perPairLikelihoodMantissas.assign(o.logLikelihoods ? nPairs : 0, 0.0);
  perPairLikelihoodExponents.assign(o.logLikelihoods ? nPairs : 0, 0);
  perPairLogLikelihoods.assign(o.logLikelihoods ? nPairs : 0, 0.0);
  binLikelihoodMantissas.assign(o.logLikelihoods ? cells : 0, 0.0);
  binLikelihoodExponents.assign(o.logLikelihoods ? cells : 0, 0);
  binLogLikelihoods.assign(o.logLikelihoods ? cells : 0, 0.0);
  // the Viterbi paths: [pairs][sites] and [pairs]
  perPairViterbiStates.assign(o.viterbiPaths ? nPairs * S : 0, 0);
  perPairViterbiMantissas.assign(o.viterbiPaths ? nPairs : 0, 0.0);
  perPairViterbiExponents.assign(o.viterbiPaths ? nPairs : 0, 0);
  perPairViterbiLogProbabilities.assign(o.viterbiPaths ? nPairs : 0, 0.0);
  // the sampled paths: [pairs][samples][sites]
  perPairSampledStates.assign(o.sampledPaths > 0 ? nPairs * static_cast<size_t>(o.sampledPaths) * S : 0, 0);
  // the change probabilities: [pairs][sites] and [pairs][bins of their own]
  const size_t changeCells = o.transitionBins.size() < 2 ? 0 : nPairs * (o.transitionBins.size() - 1);
  perPairDownProbabilities.assign(o.transitionRows ? nPairs * S : 0, 0.f);
  perPairUpProbabilities.assign(o.transitionRows ? nPairs * S : 0, 0.f);
  binExpectedDowns.assign(changeCells, 0.f);
  binExpectedUps.assign(changeCells, 0.f);
}

void DecodePairsReturnStruct::finaliseCalculations()
{
  firstMinima(perPairPosteriorMeans, numPairs, numSites, minPosteriorMeans, argminPosteriorMeans);
  firstMinima(perPairMAPs, numPairs, numSites, minMAPs, argminMAPs);
}

} // namespace fsmc_host
