// The token-set measures of the per-item sweeps (top_k_raw_kernels.hpp, top_k_levels_kernels.hpp) and of the listed-pair
// kernels (pairs_kernels.hpp), as policies: everything those kernels know about a measure is in one object here.
//
// For sets of a and b ids that share k (k <= min(a, b)) a measure is one IEEE double division num(k) / den(a, b):
//   JaccardMeasure      k / (a + b - k)     intersection_vs_union   -- the default argument of every kernel template
//   DiceMeasure         2 k / (a + b)       intersection_vs_mean
//   OverlapMeasure      k / min(a, b)       intersection_vs_smaller
//   ContainmentMeasure  k / a               intersection_vs_left (a: the LEFT set)
// and a policy object m answers
//   m.defined(a, b)       is the denominator non-zero?  (an undefined pair is the host's ZeroDivisionError: never emitted)
//   m.score(a, b, k)      the exact double (defined pairs only)
//   m.need(a, b, eff)     the least k with score(a, b, k) >= eff, min(a, b) + 1 when none: an analytic guess at most the
//                         answer (guess - 1 < eff den(1 + 2^-53) - 1, so score(guess - 1) < eff by 1 / den >> 2^-53), then
//                         the walk up on the exact double, so the bound never rounds a pair away
//   m.bound(a, b)         score(a, b, min(a, b)), -inf when undefined: the class bound of the RAW walk.  Non-increasing
//                         away from a in b for every measure here: Jaccard min / max; Dice 2 min / (a + b) (b <= a:
//                         2b / (a + b) grows with b; b >= a: 2a / (a + b) falls); overlap flat 1; containment
//                         min(a, b) / a, b / a below a and flat 1 above
//   m.up_first(a0, lo, hi)  walk to class hi before class lo?  Only the order of the sweep, never its records
//   m.part(a, b, k)       one step of the levels sum: score, 0.0 when undefined (such a pair never leaves the device)
//   m.later(a1, b1, k)    upper bound of every step after step 1 of a levels pair whose step-1 sets have a1 and b1 ids
//                         and whose whole rows share at most k: the later sets contain the step-1 sets, so a later
//                         denominator is at least den(a1, b1) and a later numerator at most num(k)
// The three new measures share one instantiation of every kernel: RuntimeMeasure switches on a wave-uniform code (a
// scalar branch beside a double division), DESIGN 4.16 has the build times that decided it.
#pragma once
#include "nsm_common.hpp"
#include "nsm_hip_measures.h"

namespace nsm {

__device__ __forceinline__ double topk_jaccard_score(int a, int b, int inter) {  // the RAW Jaccard grid's quotient
  return static_cast<double>(inter) / static_cast<double>(a + b - inter);
}

// Least intersection of a set of a ids and one of b ids (a + b >= 1) whose Jaccard score reaches `eff`, or
// min(a, b) + 1 when none does: a start below the answer, then the walk up on the exact double score.
__device__ __forceinline__ int jaccard_need(int a, int b, double eff) {
  if (eff <= 0.0) return 0;
  const int top = min(a, b);
  int need = static_cast<int>(floor(eff * static_cast<double>(a + b) / (1.0 + eff))) - 1;
  need = max(0, min(need, top + 1));
  while (need <= top && topk_jaccard_score(a, b, need) < eff) ++need;
  return need;
}

// Upper bound of |A n B| / |A u B| for sets of a and b ids that share at most `inter` (inter <= min(a, b)).
__device__ __forceinline__ double lev_top_jac(int a, int b, int inter) {
  const int uni = a + b - inter;
  return uni ? static_cast<double>(inter) / static_cast<double>(uni) : 0.0;
}

struct JaccardMeasure {
  __host__ __device__ explicit JaccardMeasure(int = NSM_MEASURE_UNION) {}
  __device__ __forceinline__ bool defined(int a, int b) const { return a + b > 0; }
  __device__ __forceinline__ double score(int a, int b, int k) const { return topk_jaccard_score(a, b, k); }
  __device__ __forceinline__ int need(int a, int b, double eff) const { return jaccard_need(a, b, eff); }
  __device__ __forceinline__ double bound(int a, int b) const {
    return a + b == 0 ? -__builtin_inf() : topk_jaccard_score(a, b, min(a, b));
  }
  // bound of class hi for a0: a0 / hi; of class lo: lo / a0
  __device__ __forceinline__ bool up_first(int a0, int lo, int hi) const {
    return static_cast<long long>(a0) * a0 >= static_cast<long long>(lo) * hi;
  }
  __device__ __forceinline__ double part(int a, int b, int k) const { return lev_top_jac(a, b, k); }
  __device__ __forceinline__ double later(int a1, int b1, int k) const {
    const int m = max(a1, b1);
    return m ? fmin(1.0, static_cast<double>(k) / static_cast<double>(m)) : 1.0;
  }
};

// What a quotient measure adds to its num / den / guess (guess: eff den / num(1), before the ceiling).
template <class Self>
struct QuotientMeasure {
  __device__ __forceinline__ const Self& self() const { return static_cast<const Self&>(*this); }
  __device__ __forceinline__ bool defined(int a, int b) const { return self().den(a, b) > 0; }
  __device__ __forceinline__ double score(int a, int b, int k) const {
    return static_cast<double>(self().num(k)) / static_cast<double>(self().den(a, b));
  }
  __device__ __forceinline__ int need(int a, int b, double eff) const {
    if (eff <= 0.0) return 0;
    const int top = min(a, b);
    int need = static_cast<int>(fmin(ceil(self().guess(a, b, eff)), static_cast<double>(top + 2))) - 1;
    need = max(0, min(need, top + 1));
    while (need <= top && score(a, b, need) < eff) ++need;
    return need;
  }
  __device__ __forceinline__ double bound(int a, int b) const {
    return defined(a, b) ? score(a, b, min(a, b)) : -__builtin_inf();
  }
  __device__ __forceinline__ bool up_first(int a0, int lo, int hi) const { return bound(a0, hi) >= bound(a0, lo); }
  __device__ __forceinline__ double part(int a, int b, int k) const { return defined(a, b) ? score(a, b, k) : 0.0; }
  __device__ __forceinline__ double later(int a1, int b1, int k) const {
    return defined(a1, b1) ? fmin(1.0, score(a1, b1, k)) : 1.0;
  }
};

struct DiceMeasure : QuotientMeasure<DiceMeasure> {  // 2 k / (a + b)
  __host__ __device__ explicit DiceMeasure(int = NSM_MEASURE_MEAN) {}
  __device__ __forceinline__ int num(int k) const { return 2 * k; }
  __device__ __forceinline__ int den(int a, int b) const { return a + b; }
  __device__ __forceinline__ double guess(int a, int b, double eff) const { return eff * static_cast<double>(a + b) * 0.5; }
};

struct OverlapMeasure : QuotientMeasure<OverlapMeasure> {  // k / min(a, b)
  __host__ __device__ explicit OverlapMeasure(int = NSM_MEASURE_SMALLER) {}
  __device__ __forceinline__ int num(int k) const { return k; }
  __device__ __forceinline__ int den(int a, int b) const { return min(a, b); }
  __device__ __forceinline__ double guess(int a, int b, double eff) const { return eff * static_cast<double>(min(a, b)); }
};

struct ContainmentMeasure : QuotientMeasure<ContainmentMeasure> {  // k / a
  __host__ __device__ explicit ContainmentMeasure(int = NSM_MEASURE_LEFT) {}
  __device__ __forceinline__ int num(int k) const { return k; }
  __device__ __forceinline__ int den(int a, int) const { return a; }
  __device__ __forceinline__ double guess(int a, int, double eff) const { return eff * static_cast<double>(a); }
};

// The three above behind one wave-uniform code (NSM_MEASURE_MEAN / _SMALLER / _LEFT; the entries have refused any other).
struct RuntimeMeasure : QuotientMeasure<RuntimeMeasure> {
  int code;
  __host__ __device__ explicit RuntimeMeasure(int c) : code(c) {}
  __device__ __forceinline__ int num(int k) const { return code == NSM_MEASURE_MEAN ? DiceMeasure{}.num(k) : k; }
  __device__ __forceinline__ int den(int a, int b) const {
    return code == NSM_MEASURE_MEAN      ? DiceMeasure{}.den(a, b)
           : code == NSM_MEASURE_SMALLER ? OverlapMeasure{}.den(a, b)
                                         : ContainmentMeasure{}.den(a, b);
  }
  __device__ __forceinline__ double guess(int a, int b, double eff) const {
    return code == NSM_MEASURE_MEAN      ? DiceMeasure{}.guess(a, b, eff)
           : code == NSM_MEASURE_SMALLER ? OverlapMeasure{}.guess(a, b, eff)
                                         : ContainmentMeasure{}.guess(a, b, eff);
  }
};

// Host side: the name of a measure code for messages, nullptr for a code no entry accepts.
inline const char* measure_name(int32_t measure) {
  switch (measure) {
    case NSM_MEASURE_UNION: return "union";
    case NSM_MEASURE_MEAN: return "mean";
    case NSM_MEASURE_SMALLER: return "smaller";
    case NSM_MEASURE_LEFT: return "left";
    default: return nullptr;
  }
}

// The check every nsm_set_* entry runs right after its null-argument check, before any HIP call.
inline int check_measure(const char* who, int32_t measure) {
  if (measure_name(measure)) return 0;
  set_error("%s: unknown measure %d (0 union, 1 mean, 2 smaller, 3 left)", who, measure);
  return NSM_E_BADARG;
}

}  // namespace nsm
