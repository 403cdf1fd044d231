// Threshold profiles of the LEVELS grids (compare_terms over fuzzy_match / intersection_vs_union): hit counts of a ladder
// of thresholds and the best score per left and per right item, after the category predicate and without the banned
// pairs -- see profile_raw.hip.  The sweep is the one of top_k_levels.hip (top_k_levels_kernels.hpp) instantiated with the
// tally sink (score_tally.hpp): every bound and early exit prunes against t[0], with the margins it always had, and the
// blacklist is consulted for every pair at or above t[0] before it is counted.
#include "score_tally.hpp"
#include "top_k_levels_kernels.hpp"

namespace nsm {

template <int K>
static int dispatch_indel_levels_profile(bool prune, const nsm_level_items* li, const nsm_str_table* ls, const nsm_level_items* ri,
                                         const nsm_str_table* rs, const int32_t* bs, const int32_t* bj,
                                         const TopLevIndelParams& p, const TallyOut& o, unsigned long long* stats, hipStream_t s) {
  auto launch = [&](auto pruned) {
    const size_t lds = static_cast<size_t>(p.pm_stride) * kPmWords<K> * 8 + static_cast<size_t>(16 * K) * kWave * 4;
    hipLaunchKernelGGL((indel_levels_top_k_kernel<K, decltype(pruned)::value, ScoreTally>), dim3(p.n_left), dim3(kWave), lds, s,
                       li->first, li->nlev, li->orig, li->cat, ls->codes, ls->len, ls->hist, ri->first, ri->nlev, ri->orig,
                       ri->cat, rs->codes, rs->len, rs->hist, bs, bj, static_cast<nsm_hit*>(nullptr),
                       static_cast<nsm_hit*>(nullptr), static_cast<unsigned long long*>(nullptr), stats, p, o);
    return hip_status(hipGetLastError(), "indel levels profile kernel launch");
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

template <int W>
static int dispatch_jaccard_levels_profile(bool prune, const nsm_set_table* l, const nsm_set_table* r, const int32_t* bs,
                                           const int32_t* bj, const TopLevJacParams& p, const TallyOut& o,
                                           unsigned long long* stats, hipStream_t s) {
  auto launch = [&](auto pruned) {
    hipLaunchKernelGGL((jaccard_levels_top_k_kernel<W, decltype(pruned)::value, ScoreTally>), dim3(p.n_left), dim3(kWave), 0, s,
                       l->ids, l->cnt, l->nlev, l->plen, l->cat, l->filt, l->orig, r->ids, r->cnt, r->nlev, r->plen, r->cat,
                       r->filt, r->orig, bs, bj, static_cast<nsm_hit*>(nullptr), static_cast<nsm_hit*>(nullptr),
                       static_cast<unsigned long long*>(nullptr), stats, p, o);
    return hip_status(hipGetLastError(), "jaccard levels profile kernel launch");
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

}  // namespace nsm

extern "C" int nsm_indel_levels_profile(const nsm_level_items* left, const nsm_str_table* left_strings,
                                        const nsm_level_items* right, const nsm_str_table* right_strings,
                                        const double* thresholds, int32_t n_thresholds, int32_t category_mode, uint32_t flags,
                                        const int32_t* banned_start, const int32_t* banned_j, uint64_t* pairs,
                                        double* left_best, double* right_best, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_indel_levels_profile";
  if (!left || !right || !left_strings || !right_strings) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_profile_args(who, thresholds, n_thresholds, pairs, left_best, right_best)) return st;
  if (int st = check_levels_str_query(who, left, left_strings, right, right_strings, category_mode, banned_start, banned_j))
    return st;
  TopLevIndelParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = 0;
  p.pm_stride = ((left_strings->alphabet + 1) + 63) / 64 * 64;
  p.cat_mode = category_mode;
  p.hist = (left_strings->hist && right_strings->hist) ? 1 : 0;
  p.threshold = thresholds[0];
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return run_profile(
      thresholds, n_thresholds, left->orig, left->n, right->orig, right->n, pairs, left_best, right_best, s, [&](const TallyOut& o) {
        return by_stride(left_strings->stride, [&](auto kc) {
          return dispatch_indel_levels_profile<decltype(kc)::value>(prune, left, left_strings, right, right_strings, banned_start,
                                                                    banned_j, p, o, st64, s);
        });
      });
}

extern "C" int nsm_jaccard_levels_profile(const nsm_set_table* left, const nsm_set_table* right, const double* thresholds,
                                          int32_t n_thresholds, int32_t category_mode, uint32_t flags,
                                          const int32_t* banned_start, const int32_t* banned_j, uint64_t* pairs,
                                          double* left_best, double* right_best, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_jaccard_levels_profile";
  if (!left || !right) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_profile_args(who, thresholds, n_thresholds, pairs, left_best, right_best)) return st;
  if (int st = check_levels_set_query(who, left, right, category_mode, banned_start, banned_j)) return st;
  TopLevJacParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = 0;
  p.lev_stride_l = left->max_levels;
  p.lev_stride_r = right->max_levels;
  p.cat_mode = category_mode;
  p.threshold = thresholds[0];
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return run_profile(thresholds, n_thresholds, left->orig, left->n, right->orig, right->n, pairs, left_best, right_best, s,
                     [&](const TallyOut& o) {
                       return by_width(left->width, [&](auto wc) {
                         return dispatch_jaccard_levels_profile<decltype(wc)::value>(prune, left, right, banned_start, banned_j, p, o,
                                                                                     st64, s);
                       });
                     });
}
