// Per-item top-k of the RAW grids: for every left row the best min(k, #eligible) right rows in the order (score
// descending, caller's j ascending), eligible = score >= threshold.  The query of rapidfuzz's
// process.extract(query, choices, limit, score_cutoff) for fuzzy_match (reference: compare/score_functions.py:20-27) and
// intersection_vs_union (:6-13); terminology/mesh.py:207-220 asks it 1 x M per item.  The output is bounded by N k
// records whatever the data, unlike the threshold grids.
//
// Mapping to CDNA4
//   * one wavefront (a workgroup of its own) owns G consecutive rows of the LEFT table (sorted by length / set size, so
//     the rows have nearly the same size); their lengths, histograms / signatures and the state of their lists are
//     wave-uniform (SGPRs), the lanes stream right rows.  Every right row a lane fetches serves G pairs;
//   * the right table is visited class by class (len_start / size_start), starting at the class of the group's first
//     row and walking outwards in the order of decreasing class bound 2 min(la, lb) / (la + lb) (Jaccard: min / max);
//   * each row keeps its list -- at most k (score, j) records -- in its own slice of a stream-ordered scratch buffer
//     that only this wave touches (no atomics, deterministic); once the list is full its worst record is the row's
//     FLOOR.  A class, or a pair, is skipped only when its upper bound is STRICTLY below max(threshold, floor): a pair
//     that equals the floor may still win on j.  The sweep ends when no row can gain from the classes left;
//   * bounds: the exact class bound, then the 32-bucket histogram bound LCS <= (la + lb - L1) / 2 (strides 64 and 128:
//     a bucket of a longer row can saturate its uint8) / the signature bound of nsm_hip.h (sig, sig2);
//   * survivors get their exact score: the multi-word bit-parallel LCS with the G rows' match masks resident in LDS
//     (add_chain of indel_wide.hpp), or a merge of the two ascending id rows; the score is the double the RAW grids emit;
//   * at the end the wave reserves its records in `out` with one atomic and copies its lists there.
//
// Grouped variants (GROUPED, nsm_*_raw_top_k_grouped): right row j belongs to group right_group[j] and a list keeps at most
// one record per group, the group's best row -- terminology/mesh.py:207-220's sort + drop_duplicates(subset="Id") + limit.
// Everything above is unchanged; the difference is the list object (TopLists<true>, top_k_lists.hpp).
#include "top_k_raw_kernels.hpp"

namespace nsm {

// ---------------------------------------------------------------------------------------------------------------- launch
// rgroup == nullptr: the ungrouped kernels (rgroup and glist unused); else the grouped ones
template <int W, bool PRUNE, bool HIST>
static int launch_indel_top_k(const nsm_str_table* l, const nsm_str_table* r, const int32_t* rgroup, const TopIndelParams& p,
                              const TopOut& o) {
  return by_grouped(rgroup != nullptr, [&](auto grouped) {
    auto* kern = indel_top_k_kernel<W, PRUNE, HIST, decltype(grouped)::value>;
    const size_t lds = static_cast<size_t>(kTopG) * p.pm_stride * W * 8;
    if (lds > 64 * 1024) {
      const int st = hip_status(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    static_cast<int>(lds)), "indel_top_k_kernel LDS");
      if (st) return st;
    }
    hipLaunchKernelGGL(kern, dim3((p.n_left + kTopG - 1) / kTopG), dim3(kWave), lds, o.sc.s, l->codes, l->len, l->orig,
                       reinterpret_cast<const uint32_t*>(l->hist), r->codes, r->len_start, r->orig,
                       reinterpret_cast<const uint32_t*>(r->hist), o.sc.list, o.out, o.out_count, o.stats, p, rgroup, o.sc.glist,
                       typename TopLists<decltype(grouped)::value>::Extra{});
    return hip_status(hipGetLastError(), "indel_top_k_kernel launch");
  });
}

template <int W>
static int dispatch_indel(bool prune, bool hist, const nsm_str_table* l, const nsm_str_table* r, const int32_t* rgroup,
                          const TopIndelParams& p, const TopOut& o) {
  if (!prune) return launch_indel_top_k<W, false, false>(l, r, rgroup, p, o);
  if (hist) return launch_indel_top_k<W, true, true>(l, r, rgroup, p, o);
  return launch_indel_top_k<W, true, false>(l, r, rgroup, p, o);
}

template <int W>
static int dispatch_jaccard(bool prune, const nsm_set_table* l, const nsm_set_table* r, const int32_t* rgroup,
                            const TopJacParams& p, const TopOut& o) {
  auto launch = [&](auto pruned) {
    return by_grouped(rgroup != nullptr, [&](auto grouped) {
      hipLaunchKernelGGL((jaccard_top_k_kernel<W, decltype(pruned)::value, decltype(grouped)::value>),
                         dim3((p.n_left + kTopG - 1) / kTopG), dim3(kWave), 0, o.sc.s, l->ids, l->cnt, l->sig, l->sig2, l->orig,
                         r->ids, r->size_start, r->sig, r->sig2, r->orig, o.sc.list, o.out, o.out_count, o.stats, p, rgroup,
                         o.sc.glist, typename TopLists<decltype(grouped)::value>::Extra{});
      return hip_status(hipGetLastError(), "jaccard_top_k_kernel launch");
    });
  };
  return prune ? launch(std::true_type{}) : launch(std::false_type{});
}

// The checks both RAW entries start with, in this order: null arguments, k < 1, the group column.
static int check_raw_args(const char* who, const void* left, const void* right, const void* out, const void* out_count,
                          int32_t k, bool grouped, const int32_t* right_group) {
  if (!left || !right || !out_count || !out) {
    set_error("%s: null argument", who);
    return NSM_E_BADARG;
  }
  if (int st = check_k(who, k)) return st;
  if (grouped && !right_group) {
    set_error("%s: right_group is null", who);
    return NSM_E_BADARG;
  }
  return 0;
}

// Both Indel entries: `grouped` asks for right_group (one record per group, top_k_lists.hpp).
static int indel_raw_top_k(const char* who, bool grouped, const nsm_str_table* left, const nsm_str_table* right,
                           const int32_t* right_group, double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                           unsigned long long* out_count, uint64_t* stats, void* stream) {
  if (int st = check_raw_args(who, left, right, out, out_count, k, grouped, right_group)) return st;
  if (int st = check_raw_str_query(who, left, right)) return st;
  int keff = 0;
  if (int st = clamp_k(who, k, right->n, &keff)) return st;
  if (left->n == 0 || right->n == 0) return 0;
  TopIndelParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = keff;
  p.pm_stride = ((left->alphabet + 1) + 63) / 64 * 64;
  p.threshold = threshold;
  const bool prune = (flags & NSM_FLAG_PRUNE) != 0;
  // (a 32-bucket count saturates at 255: the histogram bound holds for rows of at most 255 code units)
  const bool hist = prune && left->hist && right->hist && left->stride <= 128;
  TopOut o{{static_cast<hipStream_t>(stream)}, out, out_count, reinterpret_cast<unsigned long long*>(stats)};
  if (int st = o.sc.alloc(left->n, keff, grouped)) return st;
  const int32_t* rg = grouped ? right_group : nullptr;
  return o.sc.release(by_stride(left->stride, [&](auto kc) {
    return dispatch_indel<decltype(kc)::value>(prune, hist, left, right, rg, p, o);
  }));
}

static int jaccard_raw_top_k(const char* who, bool grouped, const nsm_set_table* left, const nsm_set_table* right,
                             const int32_t* right_group, double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                             unsigned long long* out_count, uint64_t* stats, void* stream) {
  if (int st = check_raw_args(who, left, right, out, out_count, k, grouped, right_group)) return st;
  if (int st = check_raw_set_query(who, left, right)) return st;
  int keff = 0;
  if (int st = clamp_k(who, k, right->n, &keff)) return st;
  if (left->n == 0 || right->n == 0) return 0;
  TopJacParams p;
  p.n_left = left->n;
  p.n_right = right->n;
  p.k = keff;
  p.threshold = threshold;
  const bool prune = (flags & NSM_FLAG_PRUNE) && left->sig && right->sig;
  TopOut o{{static_cast<hipStream_t>(stream)}, out, out_count, reinterpret_cast<unsigned long long*>(stats)};
  if (int st = o.sc.alloc(left->n, keff, grouped)) return st;
  const int32_t* rg = grouped ? right_group : nullptr;
  return o.sc.release(by_width(left->width, [&](auto wc) {
    return dispatch_jaccard<decltype(wc)::value>(prune, left, right, rg, p, o);
  }));
}

}  // namespace nsm

extern "C" int nsm_indel_raw_top_k(const nsm_str_table* left, const nsm_str_table* right, double threshold, int32_t k,
                                   uint32_t flags, nsm_hit* out, unsigned long long* out_count, uint64_t* stats, void* stream) {
  return nsm::indel_raw_top_k("nsm_indel_raw_top_k", false, left, right, nullptr, threshold, k, flags, out, out_count, stats,
                              stream);
}

extern "C" int nsm_indel_raw_top_k_grouped(const nsm_str_table* left, const nsm_str_table* right, const int32_t* right_group,
                                           double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                                           unsigned long long* out_count, uint64_t* stats, void* stream) {
  return nsm::indel_raw_top_k("nsm_indel_raw_top_k_grouped", true, left, right, right_group, threshold, k, flags, out,
                              out_count, stats, stream);
}

extern "C" int nsm_jaccard_raw_top_k(const nsm_set_table* left, const nsm_set_table* right, double threshold, int32_t k,
                                     uint32_t flags, nsm_hit* out, unsigned long long* out_count, uint64_t* stats,
                                     void* stream) {
  return nsm::jaccard_raw_top_k("nsm_jaccard_raw_top_k", false, left, right, nullptr, threshold, k, flags, out, out_count,
                                stats, stream);
}

extern "C" int nsm_jaccard_raw_top_k_grouped(const nsm_set_table* left, const nsm_set_table* right, const int32_t* right_group,
                                             double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                                             unsigned long long* out_count, uint64_t* stats, void* stream) {
  return nsm::jaccard_raw_top_k("nsm_jaccard_raw_top_k_grouped", true, left, right, right_group, threshold, k, flags, out,
                                out_count, stats, stream);
}
