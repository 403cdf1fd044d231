// Score LISTED pairs: nsm_*_pairs write the score of every (i, j) record of a caller's list in place -- rapidfuzz's
// process.cpdist beside extract (the top-k entries) and the threshold grids.  O(P) in, O(P) out: the scores of a validated
// mapping, of a whitelist, of another grid's hits (the records are nsm_hit, so any grid's output can be handed straight
// back in).  No threshold, no category predicate, no blacklist, no pruning: the caller has decided which pairs it wants.
//
// The score is the double the matching nsm_*_grid reports for the pair, bit for bit: indel_score (indel_score.hpp), the
// Jaccard quotients of the top-k kernels (topk_jaccard_score, lev_top_jac) and the levels sum
//   sum_{s=1..max(Ll,Lr)} 2^-s * part(level min(s,Ll-1), level min(s,Lr-1))
// accumulated in double in that order (levels_sum in pairs_kernels.hpp, the one copy both levels kernels use; the kernels,
// checks and launch helper live in that header so that set_pairs.hip can instantiate them with another measure).
// "No score" is -1.0: an id outside the row map, an id without a row, and the pairs the host resolves before a grid launch
// (two empty sets, an item without levels, an empty-vs-empty level of a levels Jaccard pair).
//
// Mapping to CDNA4: both rows of a pair are the pair's own, so there is no wave-uniform operand to share among 64 pairs
// as the grid kernels do.  Instead ONE WAVEFRONT SCORES ONE PAIR and takes pairs grid-stride; everything about the pair
// (ids, rows, lengths, levels, the LCS state) is wave-uniform and lives in SGPRs, the lanes hold the two rows.
//   * Indel: the SHORTER string is the pattern, K = stride / 64 code units per lane (word w, bit `lane`); the text sits
//     in the lanes too and is read back one unit at a time with v_readlane.  The match mask of pattern word w is
//     __ballot(pattern_w == unit); Hyyro's recurrence u = v & m; v = (v + u) | (v ^ u) runs on wave-uniform 64-bit words
//     with the carry handed from word w to w + 1; LCS = zero bits of v below the pattern length.
//   * Jaccard: lane p holds id p of both rows.  For every left position q the id is read with v_readlane and balloted
//     against the right ids; lane q keeps the matching right position (64: none).  |A n B| of a level pair is then
//     popcount(ballot(q < plenA && pos < plenB)): one match pass serves every step, which is what the suffix-nested layout
//     is stored for.  RAW is the single "level" (cntA, cntB).
//   * Levels: the steps run inside the wave; a level pair is rescored only when (a, b) changed.
// No LDS, no tables, one code path per stride / width.  Results leave through ordinary vector stores (lane 0).
#include "pairs_kernels.hpp"

extern "C" int nsm_indel_raw_pairs(const nsm_str_table* left, const nsm_str_table* right, const int32_t* left_row,
                                   int32_t left_ids, const int32_t* right_row, int32_t right_ids, nsm_hit* pairs,
                                   uint64_t n_pairs, void* stream) {
  using namespace nsm;
  const char* who = "nsm_indel_raw_pairs";
  if (int st = check_pair_args(who, left && right, pairs, n_pairs, left_row, left_ids, right_row, right_ids)) return st;
  if (int st = check_pair_strings(who, left, right)) return st;
  if (int st = check_pair_rows(who, left->n, right->n, left->codes && left->len, right->codes && right->len)) return st;
  if (n_pairs == 0) return 0;
  const PairList l{pairs, n_pairs, left_row, right_row, left_ids, right_ids, left->n, right->n};
  return by_stride(left->stride, [&](auto kc) {
    return launch_pairs("indel_raw_pairs_kernel launch", n_pairs, [&](dim3 grid) {
      hipLaunchKernelGGL((indel_raw_pairs_kernel<decltype(kc)::value>), grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                         left->codes, left->len, right->codes, right->len, l);
    });
  });
}

extern "C" int nsm_jaccard_raw_pairs(const nsm_set_table* left, const nsm_set_table* right, const int32_t* left_row,
                                     int32_t left_ids, const int32_t* right_row, int32_t right_ids, nsm_hit* pairs,
                                     uint64_t n_pairs, void* stream) {
  using namespace nsm;
  const char* who = "nsm_jaccard_raw_pairs";
  if (int st = check_pair_args(who, left && right, pairs, n_pairs, left_row, left_ids, right_row, right_ids)) return st;
  if (int st = check_set_tables(who, left, right)) return st;
  if (left->seg || left->seg_start || right->seg || right->seg_start) return partitioned(who);
  if (int st = check_pair_rows(who, left->n, right->n, left->ids && left->cnt, right->ids && right->cnt)) return st;
  if (n_pairs == 0) return 0;
  const PairList l{pairs, n_pairs, left_row, right_row, left_ids, right_ids, left->n, right->n};
  return by_width(left->width, [&](auto wc) {
    return launch_pairs("jaccard_raw_pairs_kernel launch", n_pairs, [&](dim3 grid) {
      hipLaunchKernelGGL((jaccard_raw_pairs_kernel<decltype(wc)::value>), grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                         left->ids, left->cnt, right->ids, right->cnt, l, JaccardMeasure{});
    });
  });
}

extern "C" int nsm_indel_levels_pairs(const nsm_level_items* left, const nsm_str_table* left_strings,
                                      const nsm_level_items* right, const nsm_str_table* right_strings,
                                      const int32_t* left_row, int32_t left_ids, const int32_t* right_row, int32_t right_ids,
                                      nsm_hit* pairs, uint64_t n_pairs, void* stream) {
  using namespace nsm;
  const char* who = "nsm_indel_levels_pairs";
  if (int st = check_pair_args(who, left && right && left_strings && right_strings, pairs, n_pairs, left_row, left_ids,
                               right_row, right_ids))
    return st;
  if (int st = check_pair_strings(who, left_strings, right_strings)) return st;
  if (left->seg || left->seg_start || right->seg || right->seg_start) return partitioned(who);
  if (left_strings->n < 0 || right_strings->n < 0) {
    set_error("%s: negative row count", who);
    return NSM_E_BADARG;
  }
  if (int st = check_pair_rows(who, left->n, right->n, left->first && left->nlev && left_strings->codes && left_strings->len,
                               right->first && right->nlev && right_strings->codes && right_strings->len))
    return st;
  if (n_pairs == 0) return 0;
  const PairList l{pairs, n_pairs, left_row, right_row, left_ids, right_ids, left->n, right->n};
  return by_stride(left_strings->stride, [&](auto kc) {
    return launch_pairs("indel_levels_pairs_kernel launch", n_pairs, [&](dim3 grid) {
      hipLaunchKernelGGL((indel_levels_pairs_kernel<decltype(kc)::value>), grid, dim3(kBlock), 0,
                         static_cast<hipStream_t>(stream), left->first, left->nlev, left_strings->codes, left_strings->len,
                         left_strings->n, right->first, right->nlev, right_strings->codes, right_strings->len,
                         right_strings->n, l);
    });
  });
}

extern "C" int nsm_jaccard_levels_pairs(const nsm_set_table* left, const nsm_set_table* right, const int32_t* left_row,
                                        int32_t left_ids, const int32_t* right_row, int32_t right_ids, nsm_hit* pairs,
                                        uint64_t n_pairs, void* stream) {
  using namespace nsm;
  const char* who = "nsm_jaccard_levels_pairs";
  if (int st = check_pair_args(who, left && right, pairs, n_pairs, left_row, left_ids, right_row, right_ids)) return st;
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
    return launch_pairs("jaccard_levels_pairs_kernel launch", n_pairs, [&](dim3 grid) {
      hipLaunchKernelGGL((jaccard_levels_pairs_kernel<decltype(wc)::value>), grid, dim3(kBlock), 0,
                         static_cast<hipStream_t>(stream), left->ids, left->cnt, left->nlev, left->plen, left->max_levels,
                         right->ids, right->cnt, right->nlev, right->plen, right->max_levels, l, JaccardMeasure{});
    });
  });
}
