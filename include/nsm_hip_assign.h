/*
 * nsm_hip_assign.h -- one-to-one assignment of a hit list (part of libnsm_hip.so's C ABI; additive, NSM_ABI_VERSION
 * stays as nsm_hip.h has it).
 *
 *   nsm_assign_hits   the loop a consumer of Comparable.sort_by_score's frame (types/comparable.py:69-70) runs to turn
 *                     a one-to-many match list into a mapping: sort + take the best pair + mark both items + repeat
 *
 * Definition.  Walk the records in canonical order (score descending, i ascending, j ascending: the order
 * nsm_sort_hits leaves); take a record iff neither its i nor its j has been taken, and mark both.  The taken records are
 * the assignment: one-to-one, maximal (no record of the list has both items free), and a prefix in the score -- assigning
 * the records >= t gives the records >= t of the assignment.
 *
 * The conventions of nsm_hip.h hold (device pointers, NSM_E_* codes, nsm_last_error) with ONE exception: this call
 * synchronises `stream` before it returns -- its rounds are driven from the host through a device counter -- and so it
 * cannot be captured into a graph.
 */
#ifndef NSM_HIP_ASSIGN_H
#define NSM_HIP_ASSIGN_H

#include "nsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags, for A/B runs and tests; the records are the same either way */
#define NSM_ASSIGN_ROUNDS_ONLY 1u /* parallel rounds until no record is live */
#define NSM_ASSIGN_STREAM_ONLY 2u /* no rounds: the one-workgroup walk over the whole list */

/*
 *   hits       device, the first n records of a list nsm_sort_hits has ordered; a record's rank is its position.  The
 *              order is a PRECONDITION and is not checked: on an unordered list the result is the greedy walk in the
 *              order given.  Only read.  A record that repeats an (i, j) is a record like any other (never taken).
 *   n          below 2^31 (ranks are 32-bit), else NSM_E_UNSUPPORTED; n == 0 returns 0 without a launch
 *   left_ids, right_ids   every i must lie in [0, left_ids) and every j in [0, right_ids): the ids index the call's
 *              scratch.  This IS checked, on the device, before anything is matched: a violation returns NSM_E_BADARG
 *              with *out_count untouched and nothing written to `out`
 *   flags      0 = rounds while they pay, then the stream stage; NSM_ASSIGN_ROUNDS_ONLY, NSM_ASSIGN_STREAM_ONLY (both:
 *              NSM_E_BADARG)
 *   out        device, room for min(n, left_ids, right_ids) records -- the assignment cannot be larger, so there is no
 *              capacity argument and no retry; written in ANY order (nsm_sort_hits orders them)
 *   out_count  device, zeroed by the caller; receives the number of records in `out`
 *   stats      device [4] or NULL, ADDED to: [0] rounds run, [1] records still live when the stream stage starts,
 *              [2] matches made by rounds, [3] matches made by the stream stage
 *
 * Checks, all before the first HIP call, in this order: NULL hits with n > 0, NULL out with n > 0, NULL out_count, a
 * negative left_ids / right_ids, both route flags: NSM_E_BADARG; n >= 2^31: NSM_E_UNSUPPORTED; n == 0: return 0.  Then a
 * capturing stream: NSM_E_UNSUPPORTED before any launch.
 *
 * Scratch (one 32-bit word per id of either side, two 32-bit ranks per record) is stream-ordered and freed inside the
 * call.
 */
int nsm_assign_hits(const nsm_hit* hits, uint64_t n, int32_t left_ids, int32_t right_ids, uint32_t flags, nsm_hit* out,
                    unsigned long long* out_count, uint64_t* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSM_HIP_ASSIGN_H */
