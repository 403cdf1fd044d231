// Per-item top-k of the LEVELS grids: for every left item the best min(k, #eligible) right items in the order (score
// descending, caller's j ascending), eligible = score >= threshold, the pair passes the category predicate and is not
// banned.  The query of gen_comparable (reference: types/comparable_data.py:223-232, compare_terms :248-265, category
// predicate :464-490) when only the best few candidates of an item are wanted -- rapidfuzz's process.extract(limit=) over
// compare_terms.  The output is bounded by N k records whatever the data, unlike the threshold grids.
//
//   score(i, j) = sum_{s=1..max(Ll,Lr)} 2^-s * ratio(left level min(s,Ll-1), right level min(s,Lr-1)),
//
// accumulated in double in that order, exactly as indel_levels.hip / jaccard_levels_impl.hpp do (the records are the
// levels grid's doubles, bit for bit).
//
// Mapping to CDNA4
//   * one wavefront (a workgroup of its own) owns ONE left item; its levels, category mask and list state are
//     wave-uniform, the lanes stream the right items 64 at a time;
//   * the list lives in a slice of stream-ordered scratch that only this wave touches (TopLists, top_k_lists.hpp); once it
//     is full its worst record is the item's FLOOR.  A pair is skipped only when an upper bound of its score is STRICTLY
//     below eff = max(threshold, floor) (a pair that equals the floor may still win on j).  The floor only moves when a
//     record enters the list, i.e. between two chunks of 64 right items;
//   * bounds, cheapest first: category mask; step 1 by length / set size plus the weight 1/2 - 2^-S of the later steps
//     (their ratios are at most 1); then step 1 by histogram (Indel: LCS <= (la + lb - L1) / 2 over the 32-bucket symbol
//     histograms) or by signature (Jaccard: |A_1 n B_1| <= popcount(sig1 & sig1'), and every later step is at most
//     min(1, |A n B| / max(|A_1|, |B_1|)) because the levels are suffix-nested); then the exact steps, a lane leaving as
//     soon as its partial sum plus the weight of the steps still to come (< 2^-s) is below eff.  Every bound carries a
//     margin (1e-6 on the bounds, 1e-9 on the early exit) far above the rounding of the double sum, so no pair whose exact
//     score reaches the floor is ever dropped;
//   * exact steps: Indel -- the left level's match masks in LDS (rebuilt only when the left level changes) and the lanes'
//     right level strings in an LDS text image, the multi-word bit-parallel LCS of indel_wide.hpp; Jaccard -- the
//     left item's ids in LDS, the position matrix of the right item's ids (the xor/min trick of jaccard_levels_impl.hpp)
//     once per pair, then a byte-parallel count per step;
//   * the blacklist (CSR keyed by the left caller id) is only consulted for a pair that is about to enter the list;
//   * at the end the wave reserves its records in `out` with one atomic and copies its list there.
#include "top_k_levels_kernels.hpp"

namespace nsm {

// ---------------------------------------------------------------------------------------------------------------- launch
template <int K>
static int dispatch_indel_levels(bool prune, const nsm_level_items* li, const nsm_str_table* ls, const nsm_level_items* ri,
                                 const nsm_str_table* rs, const int32_t* bs, const int32_t* bj, const TopLevIndelParams& p,
                                 const TopOut& o) {
  auto launch = [&](auto pruned) {
    const size_t lds = static_cast<size_t>(p.pm_stride) * kPmWords<K> * 8 + static_cast<size_t>(16 * K) * kWave * 4;
    hipLaunchKernelGGL((indel_levels_top_k_kernel<K, decltype(pruned)::value>), dim3(p.n_left), dim3(kWave), lds, o.sc.s,
                       li->first, li->nlev, li->orig, li->cat, ls->codes, ls->len, ls->hist, ri->first, ri->nlev, ri->orig,
                       ri->cat, rs->codes, rs->len, rs->hist, bs, bj, o.sc.list, o.out, o.out_count, o.stats, p,
                       TopLists<false>::Extra{});
    return hip_status(hipGetLastError(), "indel_levels_top_k_kernel launch");
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

template <int W>
static int dispatch_jaccard_levels(bool prune, const nsm_set_table* l, const nsm_set_table* r, const int32_t* bs,
                                   const int32_t* bj, const TopLevJacParams& p, const TopOut& o) {
  auto launch = [&](auto pruned) {
    hipLaunchKernelGGL((jaccard_levels_top_k_kernel<W, decltype(pruned)::value>), dim3(p.n_left), dim3(kWave), 0, o.sc.s, l->ids,
                       l->cnt, l->nlev, l->plen, l->cat, l->filt, l->orig, r->ids, r->cnt, r->nlev, r->plen, r->cat, r->filt,
                       r->orig, bs, bj, o.sc.list, o.out, o.out_count, o.stats, p,
                       TopLists<false>::Extra{});
    return hip_status(hipGetLastError(), "jaccard_levels_top_k_kernel launch");
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

}  // namespace nsm

extern "C" int nsm_indel_levels_top_k(const nsm_level_items* left, const nsm_str_table* left_strings,
                                      const nsm_level_items* right, const nsm_str_table* right_strings, double threshold,
                                      int32_t k, int32_t category_mode, uint32_t flags, const int32_t* banned_start,
                                      const int32_t* banned_j, nsm_hit* out, unsigned long long* out_count, uint64_t* stats,
                                      void* stream) {
  using namespace nsm;
  const char* who = "nsm_indel_levels_top_k";
  if (!left || !right || !left_strings || !right_strings || !out_count || !out) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_k(who, k)) return st;
  if (int st = check_levels_str_query(who, left, left_strings, right, right_strings, category_mode, banned_start, banned_j))
    return st;
  int keff = 0;
  if (int st = clamp_k(who, k, right->n, &keff)) return st;
  if (left->n == 0 || right->n == 0) return 0;
  TopLevIndelParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = keff;
  p.pm_stride = ((left_strings->alphabet + 1) + 63) / 64 * 64;
  p.cat_mode = category_mode;
  p.hist = (left_strings->hist && right_strings->hist) ? 1 : 0;
  p.threshold = threshold;
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  TopOut o{{static_cast<hipStream_t>(stream)}, out, out_count, reinterpret_cast<unsigned long long*>(stats)};
  if (int st = o.sc.alloc(left->n, keff, false)) return st;
  return o.sc.release(by_stride(left_strings->stride, [&](auto kc) {
    return dispatch_indel_levels<decltype(kc)::value>(prune, left, left_strings, right, right_strings, banned_start, banned_j, p, o);
  }));
}

extern "C" int nsm_jaccard_levels_top_k(const nsm_set_table* left, const nsm_set_table* right, double threshold, int32_t k,
                                        int32_t category_mode, uint32_t flags, const int32_t* banned_start,
                                        const int32_t* banned_j, nsm_hit* out, unsigned long long* out_count,
                                        uint64_t* stats, void* stream) {
  using namespace nsm;
  const char* who = "nsm_jaccard_levels_top_k";
  if (!left || !right || !out_count || !out) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_k(who, k)) return st;
  if (int st = check_levels_set_query(who, left, right, category_mode, banned_start, banned_j)) return st;
  int keff = 0;
  if (int st = clamp_k(who, k, right->n, &keff)) return st;
  if (left->n == 0 || right->n == 0) return 0;
  TopLevJacParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = keff;
  p.lev_stride_l = left->max_levels;
  p.lev_stride_r = right->max_levels;
  p.cat_mode = category_mode;
  p.threshold = threshold;
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  TopOut o{{static_cast<hipStream_t>(stream)}, out, out_count, reinterpret_cast<unsigned long long*>(stats)};
  if (int st = o.sc.alloc(left->n, keff, false)) return st;
  return o.sc.release(by_width(left->width, [&](auto wc) {
    return dispatch_jaccard_levels<decltype(wc)::value>(prune, left, right, banned_start, banned_j, p, o);
  }));
}
