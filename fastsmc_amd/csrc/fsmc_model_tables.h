// fsmc_model_tables.h -- a model's tables as the kernels read them, built on the host: the padded row length and the
// wave-group member, the checks of a model description and of a work list, the zero-padded rows, the RowSet copy, the
// ghost mask, the step-row arrays and the emission table.
//
// Building, not uploading: plain arithmetic on the caller's arrays, every table returned as a std::vector.  Nothing here
// knows the device's runtime, the context or the environment -- fsmc_model_create and fsmc_worklist_upload check, ask
// for the shape, build and upload.  The library's bit-exact parity rests on the arithmetic below (the emission table
// above all), so tests/model_tables_driver.cpp runs it on a CPU and tests/test_model_tables.py compares bit patterns.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fastsmc_hip.h"
#include "fsmc_constants.h"
#include "fsmc_plan.h"

namespace fsmc
{
namespace model
{
// The padded row length of a model of K states and, for the wave-group kernel, its waves per group (0 for every other
// model).  Rows are zero padded to whole operand blocks of any tunable width; wide models (128 < K <= kMaxStatesW2): NW
// waves per group hold KP / NW states each (fsmc_kernels_w2.h), the padding states are ghosts.  `built`: the members
// the library is built with.
struct Shape {
  int KP = 0;
  int w2NW = 0;
};
inline Shape shapeOf(int K, const plan::Diag& diag, const std::vector<plan::W2Member>& built)
{
  Shape s;
  s.KP = (K + kKPad - 1) / kKPad * kKPad;
  if (K > 128 && K <= kMaxStatesW2) {
    const plan::W2Member w = plan::w2Member(K, diag, built);
    s.w2NW = w.NW;
    s.KP = w.NW * w.KH;
  }
  return s;
}

// The checks of a model description, in the order the callers' tests know: FSMC_OK, or the status with its message in
// `why`.
inline int checkDesc(const fsmc_model_desc& d, std::string& why)
{
  if (d.K < 2 || d.S < 1 || d.n_rows < 1) {
    why = "need K >= 2, S >= 1, n_rows >= 1";
    return FSMC_EINVAL;
  }
  if (d.K > kMaxStatesAny) {
    why = "more than " + std::to_string(kMaxStatesAny) + " states";
    return FSMC_EUNSUPPORTED;
  }
  if (!d.pi || !d.col_ratios || !d.exp_times || !d.D || !d.B || !d.U || !d.RR || !d.step_row || !d.e1 || !d.e0m1 ||
      !d.e2m0) {
    why = "null table pointer in model description";
    return FSMC_EINVAL;
  }
  if (d.state_threshold > (uint32_t)d.K || d.age_threshold > (uint32_t)d.K) {
    why = "state/age threshold larger than K";
    return FSMC_EINVAL;
  }
  const bool seq = d.sequence != 0;
  if (seq && (!d.gap_row_f || !d.site_row_f || !d.gap_row_b || !d.site_row_b || !d.hom)) {
    why = "sequence mode needs gap_row_f, site_row_f, gap_row_b, site_row_b and hom";
    return FSMC_EINVAL;
  }
  const int32_t* rowArrays[5] = {d.step_row, seq ? d.gap_row_f : nullptr, seq ? d.site_row_f : nullptr,
                                 seq ? d.gap_row_b : nullptr, seq ? d.site_row_b : nullptr};
  static const char* const rowNames[5] = {"step_row", "gap_row_f", "site_row_f", "gap_row_b", "site_row_b"};
  for (int a = 0; a < 5; ++a) {
    for (int32_t s = 1; rowArrays[a] && s < d.S; ++s) {
      if (rowArrays[a][s] < 0 || rowArrays[a][s] >= d.n_rows) {
        why = std::string(rowNames[a]) + "[" + std::to_string(s) + "] outside the transition tables";
        return FSMC_EINVAL;
      }
    }
  }
  return FSMC_OK;
}

// The checks of a work list (neither array null, neither count zero: the caller's): the groups partition the pair list in
// order, a wave's worth of pairs at the most each, the scan window inside the decode window.
inline int checkWorklist(size_t n_pairs, const fsmc_group* groups, size_t n_groups, std::string& why)
{
  if (n_pairs > 0xFFFFFFF0ull) {
    why = "too many pairs for one work list";
    return FSMC_EINVAL;
  }
  size_t covered = 0;
  for (size_t g = 0; g < n_groups; ++g) {
    const fsmc_group& G = groups[g];
    if (G.n_pairs < 1 || G.n_pairs > (uint32_t)plan::kWave) {
      why = "group " + std::to_string(g) + ": n_pairs must be 1..64";
      return FSMC_EINVAL;
    }
    if (G.first_pair != covered) {
      why = "group " + std::to_string(g) + ": groups must partition the pair list in order";
      return FSMC_EINVAL;
    }
    if (!(G.from < G.to) || !(G.from <= G.scan_from && G.scan_from < G.scan_to && G.scan_to <= G.to)) {
      why = "group " + std::to_string(g) + ": need from <= scan_from < scan_to <= to";
      return FSMC_EINVAL;
    }
    covered += G.n_pairs;
  }
  if (covered != n_pairs) {
    why = "groups cover " + std::to_string(covered) + " pairs, list has " + std::to_string(n_pairs);
    return FSMC_EINVAL;
  }
  return FSMC_OK;
}

// rows padded to KP floats so that every table row starts 16-byte aligned
inline std::vector<float> padRows(const float* src, size_t rows, int K, int KP)
{
  std::vector<float> out(rows * (size_t)KP, 0.f);
  for (size_t r = 0; r < rows; ++r) {
    std::memcpy(&out[r * KP], src + r * K, sizeof(float) * (size_t)K);
  }
  return out;
}

// RowSet copy for the packed steps, [rows][D | B | U | Ush | RR][KP]: the rows of one key side by side so that one base
// register and immediate offsets address all of them.  Ush is U moved up one state: the packed beta step multiplies
// vec[k] = beta[k]*e[k] by U[k-1] (the term U[k-1]*vec[k] of BU[k-1], HMM.cpp:986-1005).
inline std::vector<float> rowSets(const float* D, const float* B, const float* U, const float* RR, size_t n_rows, int K,
                                  int KP)
{
  const size_t n = n_rows;
  std::vector<float> rs(n * kRowSetParts * (size_t)KP, 0.f);
  for (size_t r = 0; r < n; ++r) {
    float* q = &rs[r * kRowSetParts * KP];
    for (int k = 0; k < K; ++k) {
      q[kRowD * KP + k] = D[r * K + k];
      q[kRowB * KP + k] = B[r * K + k];
      q[kRowU * KP + k] = U[r * K + k];
      q[kRowRR * KP + k] = RR[r * K + k];
      if (k >= 1) {
        q[kRowUsh * KP + k] = U[r * K + (k - 1)];
      }
    }
  }
  return rs;
}

// [KP]: 1.0f for the K real states, 0.0f for the padding states
inline std::vector<float> ghostMask(int K, int KP)
{
  std::vector<float> mask((size_t)KP, 0.f);
  std::fill(mask.begin(), mask.begin() + K, 1.0f);
  return mask;
}

// A step-row array of S sites as the kernels read it: entry 0, which no step uses, is 0 whatever the caller left there.
inline std::vector<int> stepRows(const int32_t* src, int32_t S)
{
  std::vector<int> rows(src, src + S);
  rows[0] = 0;
  return rows;
}

// The emission table, [S][3 or 4][KP].  The reference evaluates e = (e1 + e0m1*isZero) + e2m0*isTwo with isZero/isTwo
// in {0,1} (HMM.cpp:827-828, 959-961).  The three reachable (isZero,isTwo) combinations are tabulated here with the same
// fp32 expression, so the kernel's row select is bit-identical (the factors are volatile: a compiler that folds x*0
// turns -0.0 into +0.0).
// Sequence mode adds a fourth row per site: the homozygous emission of the gap before it, which the reference
// passes as all three emission vectors with all-zero observations (HMM.cpp:764-766): (h + h*0) + h*0.
inline std::vector<float> emissions(const fsmc_model_desc& d, int KP)
{
  const int K = d.K;
  const bool seq = d.sequence != 0;
  const int NC = seq ? 4 : 3;
  std::vector<float> emis((size_t)d.S * NC * KP, 0.f);
  static const float zs[3] = {0.f, 1.f, 1.f};
  static const float ts[3] = {0.f, 0.f, 1.f};
  for (int32_t s = 0; s < d.S; ++s) {
    for (int c = 0; c < 3; ++c) {
      float* dst = &emis[((size_t)s * NC + c) * KP];
      const volatile float z = zs[c];
      const volatile float t = ts[c];
      for (int k = 0; k < K; ++k) {
        const size_t i = (size_t)s * K + k;
        dst[k] = d.e1[i] + d.e0m1[i] * z + d.e2m0[i] * t;
      }
    }
    if (seq) {
      float* dst = &emis[((size_t)s * NC + 3) * KP];
      const volatile float zero = 0.f;
      for (int k = 0; k < K; ++k) {
        const float h = d.hom[(size_t)s * K + k];
        dst[k] = h + h * zero + h * zero;
      }
    }
  }
  return emis;
}
} // namespace model
} // namespace fsmc
