// pair_transitions_driver.cpp -- the HIP-free part of fsmc_decode_pair_transitions on a CPU: reads cases from stdin, one
// a line, and prints every field of each result on one line (tests/test_pair_transition_lists.py holds the checks).
//   layout S B slicePairsMax          -> layout::transitions (fsmc_pair_layout.h)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fsmc_pair_layout.h"

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::stringstream in(line);
    std::string fn;
    in >> fn;
    if (fn == "layout") {
      size_t S = 0, B = 0, pairs = 0;
      in >> S >> B >> pairs;
      const fsmc::layout::Transitions L = fsmc::layout::transitions(S, B, pairs);
      std::printf("groupBytes=%zu rowsPerOut=%zu rowsBytes=%zu outBytes=%zu offEdges=%zu offWeights=%zu offBins=%zu "
                  "accBytes=%zu\n",
                  L.groupBytes, L.rowsPerOut, L.rowsBytes, L.outBytes, L.offEdges, L.offWeights, L.offBins, L.accBytes);
    } else if (!fn.empty()) {
      std::printf("unknown case %s\n", fn.c_str());
      return 1;
    }
  }
  return 0;
}
