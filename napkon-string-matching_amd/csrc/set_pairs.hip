// Listed pairs under the token-set measures beside Jaccard (nsm_hip_measures.h): nsm_set_raw_pairs and
// nsm_set_levels_pairs.  The kernels are those of pairs.hip (pairs_kernels.hpp: one wavefront scores one pair)
// instantiated ONCE more with RuntimeMeasure (set_measure.hpp); a pair whose measure divides by zero -- RAW: the pair's
// denominator, levels: the denominator of any step it visits -- gets -1.0 as every other pair without a score does.
// NSM_MEASURE_UNION is forwarded to the nsm_jaccard_* entry.
#include "pairs_kernels.hpp"

extern "C" int nsm_set_raw_pairs(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, const int32_t* left_row,
                                 int32_t left_ids, const int32_t* right_row, int32_t right_ids, nsm_hit* pairs, uint64_t n_pairs,
                                 void* stream) {
  using namespace nsm;
  const char* who = "nsm_set_raw_pairs";
  if (int st = check_pair_args(who, left && right, pairs, n_pairs, left_row, left_ids, right_row, right_ids)) return st;
  if (int st = check_measure(who, measure)) return st;
  if (measure == NSM_MEASURE_UNION)
    return nsm_jaccard_raw_pairs(left, right, left_row, left_ids, right_row, right_ids, pairs, n_pairs, stream);
  if (int st = check_set_tables(who, left, right)) return st;
  if (left->seg || left->seg_start || right->seg || right->seg_start) return partitioned(who);
  if (int st = check_pair_rows(who, left->n, right->n, left->ids && left->cnt, right->ids && right->cnt)) return st;
  if (n_pairs == 0) return 0;
  const PairList l{pairs, n_pairs, left_row, right_row, left_ids, right_ids, left->n, right->n};
  return by_width(left->width, [&](auto wc) {
    return launch_pairs("set raw pairs kernel launch", n_pairs, [&](dim3 grid) {
      hipLaunchKernelGGL((jaccard_raw_pairs_kernel<decltype(wc)::value, RuntimeMeasure>), grid, dim3(kBlock), 0,
                         static_cast<hipStream_t>(stream), left->ids, left->cnt, right->ids, right->cnt, l,
                         RuntimeMeasure(measure));
    });
  });
}

extern "C" int nsm_set_levels_pairs(const nsm_set_table* left, const nsm_set_table* right, int32_t measure,
                                    const int32_t* left_row, int32_t left_ids, const int32_t* right_row, int32_t right_ids,
                                    nsm_hit* pairs, uint64_t n_pairs, void* stream) {
  using namespace nsm;
  const char* who = "nsm_set_levels_pairs";
  if (int st = check_pair_args(who, left && right, pairs, n_pairs, left_row, left_ids, right_row, right_ids)) return st;
  if (int st = check_measure(who, measure)) return st;
  if (measure == NSM_MEASURE_UNION)
    return nsm_jaccard_levels_pairs(left, right, left_row, left_ids, right_row, right_ids, pairs, n_pairs, stream);
  if (int st = check_set_tables(who, left, right)) return st;
  if (left->seg || left->seg_start || right->seg || right->seg_start) return partitioned(who);
  if (!left->nlev || !left->plen || !right->nlev || !right->plen || left->max_levels < 1 || right->max_levels < 1) {
    set_error("%s: levels tables need nlev and plen", who);
    return NSM_E_BADARG;
  }
  if (int st = check_pair_rows(who, left->n, right->n, left->ids && left->cnt, right->ids && right->cnt)) return st;
  if (n_pairs == 0) return 0;
  const PairList l{pairs, n_pairs, left_row, right_row, left_ids, right_ids, left->n, right->n};
  return by_width(left->width, [&](auto wc) {
    return launch_pairs("set levels pairs kernel launch", n_pairs, [&](dim3 grid) {
      hipLaunchKernelGGL((jaccard_levels_pairs_kernel<decltype(wc)::value, RuntimeMeasure>), grid, dim3(kBlock), 0,
                         static_cast<hipStream_t>(stream), left->ids, left->cnt, left->nlev, left->plen, left->max_levels,
                         right->ids, right->cnt, right->nlev, right->plen, right->max_levels, l, RuntimeMeasure(measure));
    });
  });
}
