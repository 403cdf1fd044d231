/*
 * nsm_hip_support.h -- edge support and truss peeling of hit lists: match groups that do not chain (part of
 * libnsm_hip.so's C ABI; additive, NSM_ABI_VERSION stays as nsm_hip.h has it).
 *
 *   nsm_support_hits   per record the number of common neighbours of its two ends, in the graph of all lists together
 *                      or -- with min_support > 0 -- in its (min_support + 2)-truss
 *
 * Definition.  Node space and lists are those of nsm_hip_groups.h.  Record (score, i, j) of a list is an EDGE RECORD iff
 * score >= min_score (a NaN never is) and u = left_base + i differs from v = right_base + j.  E is the set of unordered
 * pairs {u, v} of all edge records of all lists together: duplicates and the two orientations of a self-join collapse.
 * N(u) = {w : {u, w} in E}.  The support of an edge is |N(u) n N(v)|, the number of triangles it lies in.
 *
 * Peeling (min_support > 0) is synchronous: a round counts every alive edge's support among the alive edges, then
 * removes ALL alive edges with support < min_support at once; it stops after the first round that removes nothing.
 * What is left is the (min_support + 2)-truss, the largest subgraph in which every edge has min_support common
 * neighbours inside the subgraph.  The word written for a record:
 *     >= 0   an edge record whose edge is alive at the end: its support in the final graph (>= min_support)
 *     -1     not an edge record
 *     -2     an edge record whose edge was removed
 * The result is independent of record order, list order, duplicates and the scheduling of any atomic.  Two disjoint
 * cohorts form a bipartite graph, where every support is 0: min_support > 0 is meant for self-joins, overlapping node
 * ranges and runs of three or more cohorts.
 *
 * The conventions of nsm_hip.h hold (device pointers, NSM_E_* codes, nsm_last_error) with ONE exception: the call
 * synchronises `stream` -- once for the verdict of its checks and the number of edge records, and once per round for
 * the number of removed edges -- and so cannot be captured into a graph.
 */
#ifndef NSM_HIP_SUPPORT_H
#define NSM_HIP_SUPPORT_H

#include "nsm_hip_groups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NSM_E_SUPPORT_ROUNDS 10003 /* internal: more removing rounds than distinct edges */

/*
 *   lists        HOST array of n_lists descriptors (read before the call returns)
 *   nodes        size of the node space
 *   min_score    records with score >= min_score whose ends differ are edge records
 *   min_support  0: one counting pass, nothing is removed; > 0: peel to the (min_support + 2)-truss
 *   support      HOST array of n_lists device pointers; support[l] has lists[l].n words, written as above
 *   stats        device [5] or NULL, ADDED to: [0] edge records, [1] distinct edges, [2] distinct edges alive at the
 *                end, [3] rounds (counting passes, the last one included), [4] the sum of the final supports over the
 *                alive distinct edges = three times the triangles of the final graph
 *
 * Checks before the first HIP call, in this order, each NSM_E_BADARG: NULL lists or NULL support with n_lists > 0; a
 * negative n_lists, nodes or min_support; then per list NULL hits or NULL support[l] with n > 0, a negative base or id
 * count, base + ids > nodes.  Then: nodes == 0, or no records at all: return 0, nothing launched, nothing written; a
 * capturing stream: NSM_E_UNSUPPORTED before any launch; 2^31 records or more in all: NSM_E_UNSUPPORTED.
 *
 * Check on the device, BEFORE anything is written; a violation returns NSM_E_BADARG with `support` and `stats` untouched:
 * every i lies in [0, left_ids) and every j in [0, right_ids) -- ALL records, whatever their score.
 *
 * Scratch (16 bytes per record for the gathered arcs; 15 bytes per arc -- two per edge record -- for the sort's other
 * buffer, the supports, the queue and the alive flags; 4 bytes per node; rocPRIM's temporary storage) is stream-ordered
 * (hipMallocAsync / hipFreeAsync) and freed inside the call; the library keeps nothing.  Every round but the last
 * removes an edge; more removing rounds than distinct edges cannot happen and are reported as NSM_E_SUPPORT_ROUNDS, never
 * looped on.
 */
int nsm_support_hits(const nsm_hit_list* lists, int32_t n_lists, int32_t nodes, double min_score, int32_t min_support,
                     int32_t* const* support, uint64_t* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSM_HIP_SUPPORT_H */
