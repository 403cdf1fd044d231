/*
 * nsm_hip_groups.h -- match groups: the connected components of hit lists (part of libnsm_hip.so's C ABI; additive,
 * NSM_ABI_VERSION stays as nsm_hip.h has it).
 *
 *   nsm_group_hits    what Mapping.update_mapping / MatchedMapping.read_excel(combine_entries=True) do on the host
 *                     (reference: napkon_string_matching/types/mapping.py): merge pairs that share an item into entries
 *
 * Definition.  Nodes are 0 .. nodes-1.  A list is a set of hit records with (left_base, left_ids, right_base, right_ids);
 * record (score, i, j) is an edge between node left_base + i and node right_base + j.  Only records with
 * score >= min_score count (a NaN score links nothing).  label[v] is the SMALLEST node of v's connected component, over
 * all lists together: independent of record order, list order, duplicates and the scheduling of any atomic.  A node no
 * record touches is its own label.  The two node ranges of a list may be disjoint (two cohorts), equal (a self-join: a
 * record (i, i) links nothing) or overlap.
 *
 * The conventions of nsm_hip.h hold (device pointers, NSM_E_* codes, nsm_last_error) with ONE exception: the call
 * synchronises `stream` once, to read the verdict of its checks, and so cannot be captured into a graph.  Everything
 * after the verdict is stream-ordered.
 */
#ifndef NSM_HIP_GROUPS_H
#define NSM_HIP_GROUPS_H

#include "nsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const nsm_hit* hits; /* device records, only read, ANY order */
  uint64_t n;
  int32_t left_base, left_ids, right_base, right_ids;
} nsm_hit_list;

#define NSM_GROUP_CONTINUE 1u /* `label` holds a forest (an earlier call's result): link the lists into it */

/*
 *   lists      HOST array of n_lists descriptors (read before the call returns)
 *   nodes      length of `label`; nodes == 0 returns 0 without a launch
 *   min_score  records with score >= min_score are edges
 *   flags      0: `label` is output only, every one of its `nodes` words is written.
 *              NSM_GROUP_CONTINUE: `label` holds an earlier call's result, or any forest with 0 <= label[v] <= v; the
 *              lists are linked into it -- a caller whose lists do not fit on the device together feeds them one call
 *              at a time.  With n_lists == 0 the call normalises the forest to smallest-node labels.
 *   label      device [nodes]
 *   stats      device [2] or NULL, ADDED to: [0] records with score >= min_score, [1] hooks made = the number of
 *              components before the call minus the number after
 *
 * Checks before the first HIP call, in this order: NULL lists with n_lists > 0, a negative n_lists or nodes, NULL label
 * with nodes > 0, unknown flag bits, then per list NULL hits with n > 0, a negative base or id count,
 * base + ids > nodes: NSM_E_BADARG; nodes == 0: return 0; a capturing stream: NSM_E_UNSUPPORTED before any launch.
 *
 * Checks on the device, BEFORE anything is linked or written; a violation returns NSM_E_BADARG with `label` and `stats`
 * untouched: every i lies in [0, left_ids) and every j in [0, right_ids) -- ALL records, whatever their score; under
 * NSM_GROUP_CONTINUE every label[v] lies in [0, v].
 *
 * Scratch (a few control words) is stream-ordered and freed inside the call.
 */
int nsm_group_hits(const nsm_hit_list* lists, int32_t n_lists, int32_t nodes, double min_score, uint32_t flags,
                   int32_t* label, uint64_t* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSM_HIP_GROUPS_H */
