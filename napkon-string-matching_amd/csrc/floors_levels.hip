// Floor grids of the LEVELS grids (compare_terms over fuzzy_match / intersection_vs_union): the hits of the levels grid at
// `threshold`, after the category predicate and without the banned pairs, that also reach their own items' floors -- see
// floors_raw.hip.  The sweep is the one of top_k_levels.hip (top_k_levels_kernels.hpp) instantiated with the gate sink
// (floor_gate.hpp): every bound and early exit prunes against max(threshold, left floor), with the margins it always had;
// the exact floor comparisons come after the category predicate, and the blacklist is consulted only for a pair that
// passed them.
#include "floor_gate.hpp"
#include "top_k_levels_kernels.hpp"

namespace nsm {

template <int K>
static int dispatch_indel_levels_floors(bool prune, const nsm_level_items* li, const nsm_str_table* ls, const nsm_level_items* ri,
                                        const nsm_str_table* rs, const int32_t* bs, const int32_t* bj, const TopLevIndelParams& p,
                                        const FloorOut& o, unsigned long long* stats, hipStream_t s) {
  auto launch = [&](auto pruned) {
    const size_t lds = static_cast<size_t>(p.pm_stride) * kPmWords<K> * 8 + static_cast<size_t>(16 * K) * kWave * 4;
    hipLaunchKernelGGL((indel_levels_top_k_kernel<K, decltype(pruned)::value, FloorGate>), dim3(p.n_left), dim3(kWave), lds, s,
                       li->first, li->nlev, li->orig, li->cat, ls->codes, ls->len, ls->hist, ri->first, ri->nlev, ri->orig,
                       ri->cat, rs->codes, rs->len, rs->hist, bs, bj, static_cast<nsm_hit*>(nullptr),
                       static_cast<nsm_hit*>(nullptr), static_cast<unsigned long long*>(nullptr), stats, p, o);
    return hip_status(hipGetLastError(), "indel levels floor kernel launch");
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

template <int W>
static int dispatch_jaccard_levels_floors(bool prune, const nsm_set_table* l, const nsm_set_table* r, const int32_t* bs,
                                          const int32_t* bj, const TopLevJacParams& p, const FloorOut& o,
                                          unsigned long long* stats, hipStream_t s) {
  auto launch = [&](auto pruned) {
    hipLaunchKernelGGL((jaccard_levels_top_k_kernel<W, decltype(pruned)::value, FloorGate>), dim3(p.n_left), dim3(kWave), 0, s,
                       l->ids, l->cnt, l->nlev, l->plen, l->cat, l->filt, l->orig, r->ids, r->cnt, r->nlev, r->plen, r->cat,
                       r->filt, r->orig, bs, bj, static_cast<nsm_hit*>(nullptr), static_cast<nsm_hit*>(nullptr),
                       static_cast<unsigned long long*>(nullptr), stats, p, o);
    return hip_status(hipGetLastError(), "jaccard levels floor kernel launch");
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

}  // namespace nsm

extern "C" int nsm_indel_levels_floor_grid(const nsm_level_items* left, const nsm_str_table* left_strings,
                                           const nsm_level_items* right, const nsm_str_table* right_strings, double threshold,
                                           const double* left_floor, const double* right_floor, int32_t category_mode,
                                           uint32_t flags, const int32_t* banned_start, const int32_t* banned_j, nsm_hit* hits,
                                           uint64_t capacity, unsigned long long* hit_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_indel_levels_floor_grid";
  if (int st = check_floor_out(who, left && right && left_strings && right_strings, hits, capacity, hit_count)) return st;
  bool empty = false;
  if (int st = check_floor_rows(who, left->n, right->n, &empty)) return st;
  if (empty) return 0;
  if (int st = check_levels_str_query(who, left, left_strings, right, right_strings, category_mode, banned_start, banned_j))
    return st;
  TopLevIndelParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = 0;
  p.pm_stride = ((left_strings->alphabet + 1) + 63) / 64 * 64;
  p.cat_mode = category_mode;
  p.hist = (left_strings->hist && right_strings->hist) ? 1 : 0;
  p.threshold = threshold;
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  const FloorOut o{left_floor, right_floor, left->orig, left->n, hits, capacity, hit_count};
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return by_stride(left_strings->stride, [&](auto kc) {
    return dispatch_indel_levels_floors<decltype(kc)::value>(prune, left, left_strings, right, right_strings, banned_start,
                                                             banned_j, p, o, st64, s);
  });
}

extern "C" int nsm_jaccard_levels_floor_grid(const nsm_set_table* left, const nsm_set_table* right, double threshold,
                                             const double* left_floor, const double* right_floor, int32_t category_mode,
                                             uint32_t flags, const int32_t* banned_start, const int32_t* banned_j, nsm_hit* hits,
                                             uint64_t capacity, unsigned long long* hit_count, uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_jaccard_levels_floor_grid";
  if (int st = check_floor_out(who, left && right, hits, capacity, hit_count)) return st;
  bool empty = false;
  if (int st = check_floor_rows(who, left->n, right->n, &empty)) return st;
  if (empty) return 0;
  if (int st = check_levels_set_query(who, left, right, category_mode, banned_start, banned_j)) return st;
  TopLevJacParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = 0;
  p.lev_stride_l = left->max_levels;
  p.lev_stride_r = right->max_levels;
  p.cat_mode = category_mode;
  p.threshold = threshold;
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  const FloorOut o{left_floor, right_floor, left->orig, left->n, hits, capacity, hit_count};
  auto* st64 = reinterpret_cast<unsigned long long*>(stats);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  return by_width(left->width, [&](auto wc) {
    return dispatch_jaccard_levels_floors<decltype(wc)::value>(prune, left, right, banned_start, banned_j, p, o, st64, s);
  });
}
