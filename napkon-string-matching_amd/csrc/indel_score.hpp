// The RAW fuzzy_match score, shared by every kernel that emits it (indel_raw.hip, indel_raw_coarse.hpp, top_k_raw.hip).
#pragma once
#include "nsm_common.hpp"

namespace nsm {

// The exact double sequence of `QRatio(a, b) / 100` once LCS is known (oracle/score_functions.py).
__device__ __forceinline__ double indel_score(int la, int lb, int lcs) {
  if (la == 0 || lb == 0) return 0.0;
  const double maximum = static_cast<double>(la + lb);
  const double dist = static_cast<double>(la + lb - 2 * lcs);
  const double norm_sim = 1.0 - dist / maximum;
  return (norm_sim * 100.0) / 100.0;
}

}  // namespace nsm
