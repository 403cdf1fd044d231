// Threshold profiles of the RAW grids: for a ladder of thresholds t[0] < ... < t[T-1] the number of hits of
// nsm_*_raw_grid at every t[k], and the best score of every left and of every right item among the hits at t[0] -- without
// the hits.  The output is O(N + M + T) whatever the data: the question "what would this threshold do" at exactly the
// thresholds where the hits are too many to materialise (fuzzy_match at 0 is N M records).
//
// The sweep is the one of top_k_raw.hip -- the same kernels (top_k_raw_kernels.hpp), same work split, class walk and
// bounds -- instantiated with the tally sink (score_tally.hpp) in place of the lists: there is no floor, so everything
// prunes against t[0] alone, and a scored pair at or above t[0] is counted instead of kept.  The scores are the doubles
// the RAW grids emit and the ladder is compared exactly, so pairs[k] == the length of the grid's hit list at t[k].
#include "score_tally.hpp"
#include "top_k_raw_kernels.hpp"

namespace nsm {

template <int W, bool PRUNE, bool HIST>
static int launch_indel_profile(const nsm_str_table* l, const nsm_str_table* r, const TopIndelParams& p, const TallyOut& o,
                                unsigned long long* stats, hipStream_t s) {
  auto* kern = indel_top_k_kernel<W, PRUNE, HIST, false, ScoreTally>;
  const size_t lds = static_cast<size_t>(kTopG) * p.pm_stride * W * 8;
  if (lds > 64 * 1024) {
    const int st = hip_status(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  static_cast<int>(lds)), "indel profile kernel LDS");
    if (st) return st;
  }
  hipLaunchKernelGGL(kern, dim3((p.n_left + kTopG - 1) / kTopG), dim3(kWave), lds, s, l->codes, l->len, l->orig,
                     reinterpret_cast<const uint32_t*>(l->hist), r->codes, r->len_start, r->orig,
                     reinterpret_cast<const uint32_t*>(r->hist), static_cast<nsm_hit*>(nullptr), static_cast<nsm_hit*>(nullptr),
                     static_cast<unsigned long long*>(nullptr), stats, p, static_cast<const int32_t*>(nullptr),
                     static_cast<int32_t*>(nullptr), o);
  return hip_status(hipGetLastError(), "indel profile kernel launch");
}

template <int W>
static int dispatch_indel_profile(bool prune, bool hist, const nsm_str_table* l, const nsm_str_table* r, const TopIndelParams& p,
                                  const TallyOut& o, unsigned long long* stats, hipStream_t s) {
  if (!prune) return launch_indel_profile<W, false, false>(l, r, p, o, stats, s);
  if (hist) return launch_indel_profile<W, true, true>(l, r, p, o, stats, s);
  return launch_indel_profile<W, true, false>(l, r, p, o, stats, s);
}

template <int W>
static int dispatch_jaccard_profile(bool prune, const nsm_set_table* l, const nsm_set_table* r, const TopJacParams& p,
                                    const TallyOut& o, unsigned long long* stats, hipStream_t s) {
  auto launch = [&](auto pruned) {
    hipLaunchKernelGGL((jaccard_top_k_kernel<W, decltype(pruned)::value, false, ScoreTally>), dim3((p.n_left + kTopG - 1) / kTopG),
                       dim3(kWave), 0, s, l->ids, l->cnt, l->sig, l->sig2, l->orig, r->ids, r->size_start, r->sig, r->sig2,
                       r->orig, static_cast<nsm_hit*>(nullptr), static_cast<nsm_hit*>(nullptr),
                       static_cast<unsigned long long*>(nullptr), stats, p, static_cast<const int32_t*>(nullptr),
                       static_cast<int32_t*>(nullptr), o);
    return hip_status(hipGetLastError(), "jaccard profile kernel launch");
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

}  // namespace nsm

extern "C" int nsm_indel_raw_profile(const nsm_str_table* left, const nsm_str_table* right, const double* thresholds,
                                     int32_t n_thresholds, uint32_t flags, uint64_t* pairs, double* left_best,
                                     double* right_best, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_indel_raw_profile";
  if (!left || !right) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_profile_args(who, thresholds, n_thresholds, pairs, left_best, right_best)) return st;
  if (int st = check_raw_str_query(who, left, right)) return st;
  TopIndelParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = 0;
  p.pm_stride = ((left->alphabet + 1) + 63) / 64 * 64;
  p.threshold = thresholds[0];
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  const bool hist = prune && left->hist && right->hist && left->stride <= 128;  // (as in nsm_indel_raw_top_k)
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return run_profile(thresholds, n_thresholds, left->orig, left->n, right->orig, right->n, pairs, left_best, right_best, s,
                     [&](const TallyOut& o) {
                       return by_stride(left->stride, [&](auto kc) {
                         return dispatch_indel_profile<decltype(kc)::value>(prune, hist, left, right, p, o, st64, s);
                       });
                     });
}

extern "C" int nsm_jaccard_raw_profile(const nsm_set_table* left, const nsm_set_table* right, const double* thresholds,
                                       int32_t n_thresholds, uint32_t flags, uint64_t* pairs, double* left_best,
                                       double* right_best, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_jaccard_raw_profile";
  if (!left || !right) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_profile_args(who, thresholds, n_thresholds, pairs, left_best, right_best)) return st;
  if (int st = check_raw_set_query(who, left, right)) return st;
  TopJacParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = 0;
  p.threshold = thresholds[0];
  const bool prune = (flags & NSM_FLAG_PRUNE) && left->sig && right->sig;
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return run_profile(thresholds, n_thresholds, left->orig, left->n, right->orig, right->n, pairs, left_best, right_best, s,
                     [&](const TallyOut& o) {
                       return by_width(left->width, [&](auto wc) {
                         return dispatch_jaccard_profile<decltype(wc)::value>(prune, left, right, p, o, st64, s);
                       });
                     });
}
