// fsmc_philox.h -- Philox4x32-10 (Salmon et al., SC'11) and the uniform the samplers draw from it, in plain integer C++:
// the same text runs in sample_kernel (fsmc_pair_samples.h) and on a CPU (tests/pair_samples_driver.cpp checks the known
// answers).  Nothing here knows the device's runtime.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define FSMC_HD __host__ __device__ __forceinline__
#else
#define FSMC_HD inline
#endif

namespace fsmc
{

struct Philox4 {
  uint32_t v[4];
};

// Ten rounds; the key is raised by the Weyl constants between rounds (nine times).
FSMC_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// The uniform of (seed, pair, sample r, site t): key = (seed & 0xffffffff, seed >> 32), counter = (t >> 2, r, hap_a,
// hap_b), u = float(out[t & 3] >> 8) * 2^-24 -- 24 bits, exact, in [0, 1).
FSMC_HD float sampleUniform(uint32_t seedLo, uint32_t seedHi, uint32_t hapA, uint32_t hapB, uint32_t r, uint32_t t)
{
  const Philox4 o = philox4x32_10(t >> 2, r, hapA, hapB, seedLo, seedHi);
  const uint32_t s = t & 3u;
  const uint32_t x = s == 0u ? o.v[0] : s == 1u ? o.v[1] : s == 2u ? o.v[2] : o.v[3];
  return (float)(x >> 8) * 5.9604644775390625e-8f;
}

} // namespace fsmc
