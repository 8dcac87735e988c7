// pair_samples_driver.cpp -- the HIP-free parts of fsmc_decode_pair_samples on a CPU: reads cases from stdin, one a
// line, and prints every field of each result on one line (tests/test_pair_sample_lists.py holds the table and the
// expected lines).
//   philox c0 c1 c2 c3 k0 k1          (hexadecimal)  -> the four output words of Philox4x32-10 (fsmc_philox.h)
//   uniform seed hap_a hap_b r t      (decimal)      -> the bits of the float32 uniform and its value
//   planSamples key=value ...         -> plan::planSamples (fsmc_plan.h); keys left out have the defaults below
//   planViterbi key=value ...         -> plan::planViterbi with state rows, the same keys: the other caller of planReplay
//   layout S n slicePairsMax          -> layout::samples (fsmc_pair_layout.h)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "fsmc_pair_layout.h"
#include "fsmc_philox.h"
#include "fsmc_plan.h"

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::stringstream in(line);
    std::string fn;
    in >> fn;
    if (fn == "philox") {
      uint32_t v[6];
      for (uint32_t& x : v) {
        in >> std::hex >> x;
      }
      const fsmc::Philox4 o = fsmc::philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5]);
      std::printf("%08x %08x %08x %08x\n", o.v[0], o.v[1], o.v[2], o.v[3]);
    } else if (fn == "uniform") {
      uint64_t seed = 0;
      uint32_t a = 0, b = 0, r = 0, t = 0;
      in >> seed >> a >> b >> r >> t;
      const float u = fsmc::sampleUniform((uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), a, b, r, t);
      uint32_t bits;
      std::memcpy(&bits, &u, sizeof(bits));
      std::printf("%08x %.9g\n", bits, (double)u);
    } else if (fn == "planSamples" || fn == "planViterbi") {
      std::map<std::string, uint64_t> kv = {{"nCU", 256}, {"perCU", 8},        {"S", 640},      {"member", 69},
                                            {"nGroups", 10}, {"chunkSites", 0}, {"hard", 1ull << 40}, {"soft", 0}};
      std::string tok;
      while (in >> tok) {
        const size_t eq = tok.find('=');
        kv[tok.substr(0, eq)] = std::strtoull(tok.c_str() + eq + 1, nullptr, 10);
      }
      fsmc::plan::Settings set;
      set.nCU = (int)kv["nCU"];
      set.chunkSites = (uint32_t)kv["chunkSites"];
      const fsmc::plan::WsBudget budget{kv["hard"], kv["soft"] ? kv["soft"] : kv["hard"]};
      fsmc::plan::LaunchPlan p;
      std::string why;
      const int rc = fn == "planSamples"
                         ? fsmc::plan::planSamples(set, (int)kv["S"], (int)kv["member"], (int)kv["perCU"],
                                                   (size_t)kv["nGroups"], budget, p, why)
                         : fsmc::plan::planViterbi(set, (int)kv["S"], (int)kv["member"], (int)kv["perCU"],
                                                   (size_t)kv["nGroups"], true, budget, p, why);
      if (rc != FSMC_OK) {
        std::printf("rc=%d why=\"%s\"\n", rc, why.c_str());
      } else {
        std::printf("rc=0 chunk=%d chunkRows=%d maxChunks=%d resident=%d wsSlot=%zu slots=%d waves=%d bytes=%zu\n", p.chunk,
                    p.chunkRows, p.maxChunks, p.residentChunks, p.wsSlot, p.slots, p.wavesPerWindow, p.bytes);
      }
    } else if (fn == "layout") {
      size_t S = 0, n = 0, pairs = 0;
      in >> S >> n >> pairs;
      const fsmc::layout::Samples L = fsmc::layout::samples(S, n, pairs);
      std::printf("groupBytes=%zu pairBytes=%zu rowsBytes=%zu\n", L.groupBytes, L.pairBytes, L.rowsBytes);
    } else if (!fn.empty()) {
      std::printf("unknown case %s\n", fn.c_str());
      return 1;
    }
  }
  return 0;
}
