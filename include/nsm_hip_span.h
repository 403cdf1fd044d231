/*
 * nsm_hip_span.h -- merge forests: the match groups of hit lists at EVERY threshold from one run (part of
 * libnsm_hip.so's C ABI; additive, NSM_ABI_VERSION stays as nsm_hip.h has it).
 *
 *   nsm_span_hits     the single-linkage hierarchy of what Mapping.update_mapping merges (reference:
 *                     napkon_string_matching/types/mapping.py): which score joined two items, and the groups a whole
 *                     ladder of thresholds would give, without one nsm_group_hits pass per threshold
 *
 * Definition.  Nodes, lists and edges are nsm_group_hits's (nsm_hip_groups.h): record (score, i, j) of a list
 * (left_base, left_ids, right_base, right_ids) joins node u = left_base + i and node v = right_base + j, and counts as an
 * edge iff score >= min_score and u != v (a NaN links nothing).  An edge's value is (score, lo, hi), lo = min(u, v),
 * hi = max(u, v).  Walk all edges of all lists together in canonical order -- the order of nsm_sort_hits's 128-bit key on
 * (score, lo, hi): score descending by its bit key (+0.0 before -0.0), then lo, then hi ascending -- and take an edge iff
 * its two ends are not yet connected by taken edges.  The taken values are the merge forest: the maximum spanning forest
 * of the lists under that order.  It does not depend on record order, list order, duplicates or scheduling (edges of
 * equal key are equal values, and at most one of them is taken).
 *
 *   cut            for every t >= min_score the components of the forest records with score >= t are the labels
 *                  nsm_group_hits gives for the same lists at min_score = t
 *   prefix         forest(min_score = t) is the records >= t of forest(min_score = t0), t >= t0
 *   decomposition  forest(A u B) = forest(forest(A) u B), the forest fed back as a list over the whole node space
 *                  (left_base = right_base = 0, left_ids = right_ids = nodes): a caller whose lists do not fit on the
 *                  device together feeds them one call at a time
 *   size           the number of records is nodes - the number of components
 *
 * The conventions of nsm_hip.h hold (device pointers, NSM_E_* codes, nsm_last_error) with ONE exception: this call
 * synchronises `stream` before it returns -- its rounds are driven from the host through device counters, as
 * nsm_assign_hits's are -- and so it cannot be captured into a graph.
 */
#ifndef NSM_HIP_SPAN_H
#define NSM_HIP_SPAN_H

#include "nsm_hip.h"
#include "nsm_hip_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSM_SPAN_NO_COMPACT 1u /* every round visits every edge.  Accepted, and what the call does anyway: dropping dead
                                  edges between the rounds was measured and did not pay */

/*
 *   lists         HOST array of n_lists descriptors (read before the call returns); the records are only read
 *   nodes         nodes == 0 returns 0 without a launch
 *   min_score     records with score >= min_score are edges
 *   flags         0 or NSM_SPAN_NO_COMPACT
 *   forest        device, room for max(nodes - 1, 0) records -- a forest cannot be larger, so there is no capacity argument
 *                 and no retry.  Records are (score, i = lo, j = hi) in GLOBAL node numbers, written in ANY order
 *                 (nsm_sort_hits with id_limit = nodes orders them)
 *   forest_count  device, zeroed by the caller; receives the number of records in `forest`
 *   label         device [nodes] or NULL: the smallest node of every node's component -- the words nsm_group_hits writes
 *                 for the same lists and min_score; every one of the `nodes` words is written
 *   stats         device [4] or NULL, ADDED to: [0] records with score >= min_score (self-loops and duplicates included,
 *                 as nsm_group_hits counts them), [1] forest records written, [2] rounds run, [3] edge visits summed over
 *                 the rounds.  Rounds are at most ceil(log2(max(nodes, 2))) + 1
 *
 * Checks before the first HIP call, in this order: NULL lists with n_lists > 0, a negative n_lists or nodes, NULL forest
 * with nodes > 1, NULL forest_count, unknown flag bits, then per list NULL hits with n > 0, a negative base or id count,
 * base + ids > nodes: NSM_E_BADARG; 2^31 or more records in total (ranks are 32-bit): NSM_E_UNSUPPORTED; nodes == 0:
 * return 0; a capturing stream: NSM_E_UNSUPPORTED before any launch.
 *
 * Check on the device, BEFORE anything is written; a violation returns NSM_E_BADARG with `forest`, `forest_count`,
 * `label` and `stats` untouched: every i lies in [0, left_ids) and every j in [0, right_ids) -- ALL records, whatever
 * their score.
 *
 * Scratch is stream-ordered and freed inside the call, and all of it is allocated before any output is written (a
 * failed allocation leaves the outputs untouched).  With R records in all lists together: 16 R bytes for the edges,
 * 16 R more (plus the radix sort's own temporary storage) when R exceeds 8192, 12 bytes per node and 64 bytes of control
 * words.
 */
int nsm_span_hits(const nsm_hit_list* lists, int32_t n_lists, int32_t nodes, double min_score, uint32_t flags,
                  nsm_hit* forest, unsigned long long* forest_count, int32_t* label, uint64_t* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSM_HIP_SPAN_H */
