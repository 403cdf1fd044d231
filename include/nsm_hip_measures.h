/*
 * nsm_hip_measures.h -- token-set measures beside Jaccard for the per-item queries (part of libnsm_hip.so's C ABI;
 * additive, NSM_ABI_VERSION stays as nsm_hip.h has it).
 *
 * For token sets A (left) and B (right), a = |A|, b = |B|, k = |A n B|, a measure is ONE IEEE double division:
 *
 *   NSM_MEASURE_UNION    k / (a + b - k)   Jaccard                               intersection_vs_union
 *   NSM_MEASURE_MEAN     2 k / (a + b)     Sorensen-Dice                         intersection_vs_mean
 *   NSM_MEASURE_SMALLER  k / min(a, b)     overlap (Szymkiewicz-Simpson)         intersection_vs_smaller
 *   NSM_MEASURE_LEFT     k / a             containment of left in right          intersection_vs_left
 *
 * In levels mode the score of a pair is sum_{s=1..max(Ll,Lr)} 2^-s * m(A_s, B_s), accumulated in double in that order
 * -- compare_terms with the measure as score_func.
 *
 * Every nsm_set_* entry has the signature of its nsm_jaccard_* counterpart (nsm_hip.h) with `measure` inserted after
 * `right`, and keeps that counterpart's arguments, checks and their order, no-allocation rule and capturability.  What
 * is added:
 *
 *   - right after the null-argument check and before any HIP call: an unknown measure is NSM_E_BADARG, and
 *     nsm_last_error names it;
 *   - NSM_MEASURE_UNION forwards to the nsm_jaccard_* entry: the records are bit-identical;
 *   - a pair whose denominator is zero has no score.  The *_pairs entries write -1.0 for it (RAW: the pair's
 *     denominator; levels: the denominator of any step the pair visits), on top of the -1.0 cases of nsm_hip.h.  The
 *     top-k, profile and floor-grid entries never emit such a pair: the caller raises the reference's ZeroDivisionError
 *     before it asks (an empty item on the side the measure divides by);
 *   - NSM_FLAG_PRUNE never changes the records.  The size filter of the sweep is the measure's own: Dice prunes on
 *     sizes as Jaccard does, containment only downwards, overlap not at all (its bound is 1 for every size); the
 *     signature filter |A n B| <= popcount(sigA & sigB) bounds k and serves every measure.
 *
 * A floor grid with both floor arrays NULL is the threshold grid of the measure (nsm_hip.h).  nsm_jaccard_raw_grid,
 * nsm_jaccard_levels_grid and nsm_jaccard_any_grid stay Jaccard-only: their filters are derived for Jaccard.
 */
#ifndef NSM_HIP_MEASURES_H
#define NSM_HIP_MEASURES_H

#include "nsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSM_MEASURE_UNION   0   /* Jaccard: accepted, records bit-identical to the nsm_jaccard_* entry */
#define NSM_MEASURE_MEAN    1
#define NSM_MEASURE_SMALLER 2
#define NSM_MEASURE_LEFT    3

int nsm_set_raw_top_k(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, double threshold, int32_t k,
                      uint32_t flags, nsm_hit* out, unsigned long long* out_count, uint64_t* stats, void* stream);

int nsm_set_raw_top_k_grouped(const nsm_set_table* left, const nsm_set_table* right, int32_t measure,
                              const int32_t* right_group, double threshold, int32_t k, uint32_t flags, nsm_hit* out,
                              unsigned long long* out_count, uint64_t* stats, void* stream);

int nsm_set_raw_profile(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, const double* thresholds,
                        int32_t n_thresholds, uint32_t flags, uint64_t* pairs, double* left_best, double* right_best,
                        uint64_t* stats, void* stream);

int nsm_set_raw_floor_grid(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, double threshold,
                           const double* left_floor, const double* right_floor, uint32_t flags, nsm_hit* hits,
                           uint64_t capacity, unsigned long long* hit_count, uint64_t* stats, void* stream);

int nsm_set_raw_pairs(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, const int32_t* left_row,
                      int32_t left_ids, const int32_t* right_row, int32_t right_ids, nsm_hit* pairs, uint64_t n_pairs,
                      void* stream);

int nsm_set_levels_top_k(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, double threshold, int32_t k,
                         int32_t category_mode, uint32_t flags, const int32_t* banned_start, const int32_t* banned_j,
                         nsm_hit* out, unsigned long long* out_count, uint64_t* stats, void* stream);

int nsm_set_levels_profile(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, const double* thresholds,
                           int32_t n_thresholds, int32_t category_mode, uint32_t flags, const int32_t* banned_start,
                           const int32_t* banned_j, uint64_t* pairs, double* left_best, double* right_best, uint64_t* stats,
                           void* stream);

int nsm_set_levels_floor_grid(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, double threshold,
                              const double* left_floor, const double* right_floor, int32_t category_mode, uint32_t flags,
                              const int32_t* banned_start, const int32_t* banned_j, nsm_hit* hits, uint64_t capacity,
                              unsigned long long* hit_count, uint64_t* stats, void* stream);

int nsm_set_levels_pairs(const nsm_set_table* left, const nsm_set_table* right, int32_t measure, const int32_t* left_row,
                         int32_t left_ids, const int32_t* right_row, int32_t right_ids, nsm_hit* pairs, uint64_t n_pairs,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* NSM_HIP_MEASURES_H */
