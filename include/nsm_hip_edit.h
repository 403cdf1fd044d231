/*
 * nsm_hip_edit.h -- Levenshtein score functions beside the Indel ratio for the per-item string queries (part of
 * libnsm_hip.so's C ABI; additive, NSM_ABI_VERSION stays as nsm_hip.h has it).
 *
 * For prepared strings a (left, la code units) and b (right, lb code units) a metric is one IEEE double division and one
 * double subtraction of small integers:
 *
 *   NSM_METRIC_INDEL        2 LCS / (la + lb)          the Indel ratio                       fuzzy_match
 *   NSM_METRIC_EDIT         1 - d(a, b) / max(la, lb)  normalised Levenshtein similarity     levenshtein_match
 *   NSM_METRIC_EDIT_WITHIN  1 - w(a, b) / la           best approximate occurrence of a in b levenshtein_within
 *
 * d is the unit-cost Levenshtein distance; w = min over the substrings s of b (the empty one included) of d(a, s), so
 * 0 <= w <= la (Sellers).  A pair with an empty string on either side scores 0.0 under every metric, as in the Indel
 * kernels.  The left string is always the pattern: NSM_METRIC_EDIT_WITHIN is not symmetric.
 *
 * In levels mode the score of a pair is sum_{s=1..max(Ll,Lr)} 2^-s * m(a_s, b_s), accumulated in double in that order
 * -- compare_terms with the metric as score_func.
 *
 * Every nsm_edit_* entry has the signature of its nsm_indel_* counterpart (nsm_hip.h) with `metric` inserted after the
 * last table argument, and keeps that counterpart's arguments, checks and their order, no-allocation rule and
 * capturability.  What is added:
 *
 *   - right after the null-argument check and before any HIP call: an unknown metric is NSM_E_BADARG, and
 *     nsm_last_error names it;
 *   - NSM_METRIC_INDEL forwards to the nsm_indel_* entry: the records are bit-identical;
 *   - NSM_FLAG_PRUNE never changes the records.  The length filter of the sweep is the metric's own: the distance is at
 *     least |la - lb|, the occurrence distance at least la - lb (it prunes only towards shorter right strings); the
 *     32-bucket histogram filter d >= ceil(L1 / 2) serves NSM_METRIC_EDIT at every stride and is not used for
 *     NSM_METRIC_EDIT_WITHIN.
 *
 * A floor grid with both floor arrays NULL is the threshold grid of the metric (nsm_hip.h).  nsm_indel_raw_grid,
 * nsm_indel_levels_grid and nsm_indel_any_grid stay Indel-only: their filters are derived for Indel.
 */
#ifndef NSM_HIP_EDIT_H
#define NSM_HIP_EDIT_H

#include "nsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSM_METRIC_INDEL       0   /* accepted, records bit-identical to the nsm_indel_* entry */
#define NSM_METRIC_EDIT        1
#define NSM_METRIC_EDIT_WITHIN 2

int nsm_edit_raw_top_k(const nsm_str_table* left, const nsm_str_table* right, int32_t metric, double threshold, int32_t k,
                       uint32_t flags, nsm_hit* out, unsigned long long* out_count, uint64_t* stats, void* stream);

int nsm_edit_raw_top_k_grouped(const nsm_str_table* left, const nsm_str_table* right, int32_t metric,
                               const int32_t* right_group, double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                               unsigned long long* out_count, uint64_t* stats, void* stream);

int nsm_edit_raw_profile(const nsm_str_table* left, const nsm_str_table* right, int32_t metric, const double* thresholds,
                         int32_t n_thresholds, uint32_t flags, uint64_t* pairs, double* left_best, double* right_best,
                         uint64_t* stats, void* stream);

int nsm_edit_raw_floor_grid(const nsm_str_table* left, const nsm_str_table* right, int32_t metric, double threshold,
                            const double* left_floor, const double* right_floor, uint32_t flags, nsm_hit* hits,
                            uint64_t capacity, unsigned long long* hit_count, uint64_t* stats, void* stream);

int nsm_edit_raw_pairs(const nsm_str_table* left, const nsm_str_table* right, int32_t metric, const int32_t* left_row,
                       int32_t left_ids, const int32_t* right_row, int32_t right_ids, nsm_hit* pairs, uint64_t n_pairs,
                       void* stream);

int nsm_edit_levels_top_k(const nsm_level_items* left, const nsm_str_table* left_strings, const nsm_level_items* right,
                          const nsm_str_table* right_strings, int32_t metric, double threshold, int32_t k,
                          int32_t category_mode, uint32_t flags, const int32_t* banned_start, const int32_t* banned_j,
                          nsm_hit* out, unsigned long long* out_count, uint64_t* stats, void* stream);

int nsm_edit_levels_profile(const nsm_level_items* left, const nsm_str_table* left_strings, const nsm_level_items* right,
                            const nsm_str_table* right_strings, int32_t metric, const double* thresholds, int32_t n_thresholds,
                            int32_t category_mode, uint32_t flags, const int32_t* banned_start, const int32_t* banned_j,
                            uint64_t* pairs, double* left_best, double* right_best, uint64_t* stats, void* stream);

int nsm_edit_levels_floor_grid(const nsm_level_items* left, const nsm_str_table* left_strings, const nsm_level_items* right,
                               const nsm_str_table* right_strings, int32_t metric, double threshold, const double* left_floor,
                               const double* right_floor, int32_t category_mode, uint32_t flags, const int32_t* banned_start,
                               const int32_t* banned_j, nsm_hit* hits, uint64_t capacity, unsigned long long* hit_count,
                               uint64_t* stats, void* stream);

int nsm_edit_levels_pairs(const nsm_level_items* left, const nsm_str_table* left_strings, const nsm_level_items* right,
                          const nsm_str_table* right_strings, int32_t metric, const int32_t* left_row, int32_t left_ids,
                          const int32_t* right_row, int32_t right_ids, nsm_hit* pairs, uint64_t n_pairs, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NSM_HIP_EDIT_H */
