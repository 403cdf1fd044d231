// The LEVELS per-item queries of the token-set measures beside Jaccard (nsm_hip_measures.h): nsm_set_levels_top_k,
// nsm_set_levels_profile, nsm_set_levels_floor_grid -- compare_terms with the measure as score_func.  The sweep is the one
// of top_k_levels.hip -- jaccard_levels_top_k_kernel (top_k_levels_kernels.hpp) with its three sinks -- instantiated ONCE
// more with RuntimeMeasure (set_measure.hpp): the score of a step and the bounds of step 1 and of the later steps are the
// measure's, the margins and everything else are unchanged.  NSM_MEASURE_UNION is forwarded to the nsm_jaccard_* entry.
#include "floor_gate.hpp"
#include "score_tally.hpp"
#include "top_k_levels_kernels.hpp"

namespace nsm {

static TopLevJacParams set_levels_params(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, int32_t k,
                                         int32_t category_mode, double threshold) {
  TopLevJacParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = k;
  p.lev_stride_l = left->max_levels;
  p.lev_stride_r = right->max_levels;
  p.cat_mode = category_mode;
  p.threshold = threshold;
  p.measure = measure;
  return p;
}

// The sweep with sink S: list / out / out_count are the top-k query's, `sx` the sink's own argument.
template <class S>
static int launch_set_levels(const char* what, const nsm_set_table* l, const nsm_set_table* r, bool prune, const int32_t* bs,
                             const int32_t* bj, const TopLevJacParams& p, nsm_hit* list, nsm_hit* out,
                             unsigned long long* out_count, unsigned long long* stats, const typename S::Extra& sx,
                             hipStream_t s) {
  return by_width(l->width, [&](auto wc) {
    auto launch = [&](auto pruned) {
      hipLaunchKernelGGL((jaccard_levels_top_k_kernel<decltype(wc)::value, decltype(pruned)::value, S, RuntimeMeasure>),
                         dim3(p.n_left), dim3(kWave), 0, s, l->ids, l->cnt, l->nlev, l->plen, l->cat, l->filt, l->orig, r->ids,
                         r->cnt, r->nlev, r->plen, r->cat, r->filt, r->orig, bs, bj, list, out, out_count, stats, p, sx);
      return hip_status(hipGetLastError(), what);
    };
    return prune ? launch(std::true_type{}) : launch(std::false_type{});
  });
}

}  // namespace nsm

extern "C" int nsm_set_levels_top_k(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, double threshold,
                                    int32_t k, int32_t category_mode, uint32_t flags, const int32_t* banned_start,
                                    const int32_t* banned_j, nsm_hit* out, unsigned long long* out_count, uint64_t* stats,
                                    void* stream) {
  using namespace nsm;
  const char* who = "nsm_set_levels_top_k";
  if (!left || !right || !out_count || !out) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_measure(who, measure)) return st;
  if (measure == NSM_MEASURE_UNION)
    return nsm_jaccard_levels_top_k(left, right, threshold, k, category_mode, flags, banned_start, banned_j, out, out_count,
                                    stats, stream);
  if (int st = check_k(who, k)) return st;
  if (int st = check_levels_set_query(who, left, right, category_mode, banned_start, banned_j)) return st;
  int keff = 0;
  if (int st = clamp_k(who, k, right->n, &keff)) return st;
  if (left->n == 0 || right->n == 0) return 0;
  const TopLevJacParams p = set_levels_params(left, right, measure, keff, category_mode, threshold);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  TopOut o{{static_cast<hipStream_t>(stream)}, out, out_count, reinterpret_cast<unsigned long long*>(stats)};
  if (int st = o.sc.alloc(left->n, keff, false)) return st;
  return o.sc.release(launch_set_levels<TopLists<false>>("set levels top-k kernel launch", left, right, prune, banned_start,
                                                         banned_j, p, o.sc.list, o.out, o.out_count, o.stats,
                                                         TopLists<false>::Extra{}, o.sc.s));
}

extern "C" int nsm_set_levels_profile(const nsm_set_table* left, const nsm_set_table* right, int32_t measure,
                                      const double* thresholds, int32_t n_thresholds, int32_t category_mode, uint32_t flags,
                                      const int32_t* banned_start, const int32_t* banned_j, uint64_t* pairs, double* left_best,
                                      double* right_best, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_set_levels_profile";
  if (!left || !right) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_measure(who, measure)) return st;
  if (measure == NSM_MEASURE_UNION)
    return nsm_jaccard_levels_profile(left, right, thresholds, n_thresholds, category_mode, flags, banned_start, banned_j, pairs,
                                      left_best, right_best, stats, stream);
  if (int st = check_profile_args(who, thresholds, n_thresholds, pairs, left_best, right_best)) return st;
  if (int st = check_levels_set_query(who, left, right, category_mode, banned_start, banned_j)) return st;
  const TopLevJacParams p = set_levels_params(left, right, measure, 0, category_mode, thresholds[0]);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return run_profile(thresholds, n_thresholds, left->orig, left->n, right->orig, right->n, pairs, left_best, right_best, s,
                     [&](const TallyOut& o) {
                       return launch_set_levels<ScoreTally>("set levels profile kernel launch", left, right, prune, banned_start,
                                                            banned_j, p, nullptr, nullptr, nullptr, st64, o, s);
                     });
}

extern "C" int nsm_set_levels_floor_grid(const nsm_set_table* left, const nsm_set_table* right, int32_t measure,
                                         double threshold, const double* left_floor, const double* right_floor,
                                         int32_t category_mode, uint32_t flags, const int32_t* banned_start,
                                         const int32_t* banned_j, nsm_hit* hits, uint64_t capacity,
                                         unsigned long long* hit_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_set_levels_floor_grid";
  if (int st = check_floor_out(who, left && right, hits, capacity, hit_count)) return st;
  if (int st = check_measure(who, measure)) return st;
  if (measure == NSM_MEASURE_UNION)
    return nsm_jaccard_levels_floor_grid(left, right, threshold, left_floor, right_floor, category_mode, flags, banned_start,
                                         banned_j, hits, capacity, hit_count, stats, stream);
  bool empty = false;
  if (int st = check_floor_rows(who, left->n, right->n, &empty)) return st;
  if (empty) return 0;
  if (int st = check_levels_set_query(who, left, right, category_mode, banned_start, banned_j)) return st;
  const TopLevJacParams p = set_levels_params(left, right, measure, 0, category_mode, threshold);
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  const FloorOut o{left_floor, right_floor, left->orig, left->n, hits, capacity, hit_count};
  return launch_set_levels<FloorGate>("set levels floor kernel launch", left, right, prune, banned_start, banned_j, p, nullptr,
                                      nullptr, nullptr, reinterpret_cast<unsigned long long*>(stats), o,
                                      static_cast<hipStream_t>(stream));
}
