// pair_layout_driver.cpp -- fsmc_pair_layout.h on a CPU: reads cases from stdin, one a line, and prints every field of
// each layout on one line (tests/test_pair_layout.py holds the table and the expected lines).
//
// A case is an entry point's name and key=value inputs; a key left out has the default below.  A region of the entry
// point's accumulator buffer is printed as name=offset:bytes:element size; a region the call has no use for is left out.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "fsmc_pair_layout.h"

using namespace fsmc;

namespace
{
struct Case {
  std::map<std::string, std::string> kv;
  size_t u(const char* key, size_t dflt) const
  {
    const auto it = kv.find(key);
    return it == kv.end() ? dflt : (size_t)std::strtoull(it->second.c_str(), nullptr, 10);
  }
  bool b(const char* key, bool dflt) const { return u(key, dflt ? 1 : 0) != 0; }
};

void region(const char* name, size_t off, size_t bytes, size_t elem)
{
  std::printf(" %s=%zu:%zu:%zu", name, off, bytes, elem);
}

void run(const std::string& fn, const Case& c)
{
  const size_t K = c.u("K", 69), KP = c.u("KP", 80), S = c.u("S", 640), B = c.u("B", 0), nT = c.u("nTail", 1);
  const size_t slice = c.u("slice", 1), n = c.u("pairs", 64);
  if (fn == "posteriors") {
    const layout::Posteriors L = layout::posteriors(K, S, c.b("rows", true), slice, n);
    std::printf("groupBytes=%zu stageBytes=%zu rowBytes=%zu rowsBytes=%zu accBytes=%zu", L.groupBytes, L.stageBytes,
                L.rowBytes, L.rowsBytes, L.accBytes);
    region("coal", L.offCoal, K * 4, 4);
    region("sum", L.offSum, K * S * 4, 4);
  } else if (fn == "minima") {
    plan::Diag diag;
    diag.minimaRange = (long)c.u("minimaRange", 0);
    const layout::Minima L = layout::minima((int)c.u("nCU", 256), S, KP, c.u("nOut", 2), n, diag);
    std::printf("groupBytes=%zu siteBlocks=%zu rangeLen=%zu rangesMax=%zu tooManyRanges=%d stageBytes=%zu vec=%zu accBytes=%zu",
                L.groupBytes, L.siteBlocks, L.rangeLen, L.rangesMax, L.tooManyRanges ? 1 : 0, L.stageBytes, L.vec,
                L.accBytes);
    region("coal", L.offCoal, KP * 4, 4);
    static const char* const names[4] = {"minMean", "argMean", "minMap", "argMap"};
    for (int i = 0; i < 4; ++i) {
      region(names[i], L.offState[i], L.vec, 4);
    }
    for (int i = 0; i < 4; ++i) {
      region((std::string("part.") + names[i]).c_str(), L.offParts[i], L.rangesMax * L.vec, 4);
    }
  } else if (fn == "bins") {
    static const char* const names[5] = {"mean", "minMean", "argMean", "minMap", "argMap"};
    bool want[5];
    for (int i = 0; i < 5; ++i) {
      want[i] = c.b(names[i], true);
    }
    const layout::Bins L = layout::bins(S, KP, B, c.u("nRows", 2), want, n);
    std::printf("groupBytes=%zu stageBytes=%zu edgeBytes=%zu outBytes=%zu accBytes=%zu", L.groupBytes, L.stageBytes,
                L.edgeBytes, L.outBytes, L.accBytes);
    region("coal", L.offCoal, KP * 4, 4);
    region("edges", L.offEdges, L.edgeBytes, 4);
    for (int i = 0; i < 5; ++i) {
      if (want[i]) {
        region(names[i], L.offOut[i], L.outBytes, 4);
      }
    }
  } else if (fn == "loglik") {
    const layout::Loglik L = layout::loglik(B, n);
    std::printf("groupBytes=%zu edgeBytes=%zu accBytes=%zu", L.groupBytes, L.edgeBytes, L.accBytes);
    region("mant", L.offMant, n * 8, 8);
    region("binMant", L.offBinMant, n * B * 8, 8);
    region("expo", L.offExpo, n * 4, 4);
    region("binExpo", L.offBinExpo, n * B * 4, 4);
    region("edges", L.offEdges, L.edgeBytes, 4);
  } else if (fn == "viterbi") {
    const layout::Viterbi L = layout::viterbi(S, c.b("states", true), c.b("prob", true), n);
    std::printf("groupBytes=%zu rowsBytes=%zu accBytes=%zu", L.groupBytes, L.rowsBytes, L.accBytes);
    region("mant", L.offMant, n * 8, 8);
    region("expo", L.offExpo, n * 4, 4);
  } else if (fn == "cdf") {
    const layout::Cdf L = layout::cdf(K, S, c.u("nOut", 1), slice, n);
    std::printf("groupBytes=%zu sliceMost=%zu stageBytes=%zu outCells=%zu rowsBytes=%zu specBytes=%zu", L.groupBytes,
                layout::sliceMostBySiteBlocks(S), L.stageBytes, L.outCells, L.rowsBytes, L.specBytes);
  } else if (fn == "tail") {
    const bool mean = c.b("mean", false), length = c.b("length", false);
    const layout::Tail L = layout::tail(K, S, nT, B, mean, length, slice, n);
    std::printf("groupBytes=%zu sliceMost=%zu stageBytes=%zu rowsBytes=%zu specBytes=%zu sumBytes=%zu outBytes=%zu accBytes=%zu",
                L.groupBytes, layout::sliceMostBySiteBlocks(S), L.stageBytes, L.rowsBytes, L.specBytes, L.sumBytes,
                L.outBytes, L.accBytes);
    region("sum", L.offSum, L.sumBytes, 8);
    if (mean || length) {
      region("edges", L.offEdges, (B + 1) * 4, 4);
    }
    if (length) {
      region("weights", L.offWeights, S * 4, 4);
    }
    if (mean) {
      region("binMean", L.offMean, L.outBytes, 4);
    }
    if (length) {
      region("binLength", L.offLength, L.outBytes, 4);
    }
  } else {
    std::printf("unknown entry point %s", fn.c_str());
  }
  std::printf("\n");
}
} // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') {
      continue;
    }
    std::stringstream words(line);
    std::string fn, word;
    words >> fn;
    Case c;
    while (words >> word) {
      const size_t eq = word.find('=');
      if (eq != std::string::npos) {
        c.kv[word.substr(0, eq)] = word.substr(eq + 1);
      }
    }
    run(fn, c);
  }
  return 0;
}
