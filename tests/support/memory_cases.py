"""The cases of tests/test_gpu_memory_contract.py that do not need a GPU to state: which grid, which threshold, which
capacities, and what the oracle says must come out.  tests/test_cpu_memory_contract.py checks their premises with the
oracle alone (enough hits to overflow every "too small" buffer, caller ids with gaps, top-k rows of every fill).

Grids: tests/support/threshold_probes.py (70 .. 90 x 229 items: several row batches, three full right tiles and a partial
one), any_operands.py for the two general kernels.
"""
import random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from support import any_operands as ao
from support import threshold_probes as tp

SMALL_CAPACITIES = (1, 63, 64, 65)  # around a wavefront's 64 records
START_COUNT = 5                     # a hit buffer that already holds records: hits are appended behind them


def capacities(count: int) -> List[int]:
    """0 (with ``hits = NULL``), the small ones, and the oracle's count - 1, the count, the count + 1."""
    return [0, *SMALL_CAPACITIES, count - 1, count, count + 1]


# ------------------------------------------------------------------------------------------------------ threshold grids
def low_threshold(g: tp.ProbeGrid) -> float:
    """The lowest threshold of the probe's own list: nearly every scored pair is a hit, so every wave appends."""
    return tp.probes_of(g)[0]


def hit_case(name: str) -> Tuple[float, list]:
    """(threshold, the oracle's hits at it) of a threshold-probe grid."""
    g = tp.grid(name)
    thr = low_threshold(g)
    return thr, tp.expectation(tp.all_scores(g), thr)


ANY_GRIDS = ["tails_indel_129", "tails_jaccard_129", "categories_indel_mode1", "categories_jaccard_nested_mode2",
             "categories_jaccard_independent_mode1"]


def any_case(name: str) -> Tuple[float, list]:
    """Threshold 0.0: every pair the category masks allow."""
    return 0.0, list(ao.oracle_all(ao.grid(name)))


# ---------------------------------------------------------------------------------------------------------- floor grids
FLOOR_GRIDS = {"nsm_indel_raw_floor_grid": "raw_indel_64", "nsm_jaccard_raw_floor_grid": "raw_jaccard_16",
               "nsm_indel_levels_floor_grid": "levels_indel_one_word-cat2_lanes",
               "nsm_jaccard_levels_floor_grid": "levels_jaccard-cat2_lanes"}


def caller_id(k):
    """Caller ids with gaps: item k reports 3 k + 2."""
    return 3 * k + 2


def floor_case(name: str):
    """(threshold, left floors, right floors, expected records) in CALLER ids ``caller_id(k)``: an item's floor is a quarter
    of its best score (NaN for every seventh left item: it admits nothing; -inf for an item without a hit)."""
    g = tp.grid(name)
    thr = low_threshold(g)
    hits = tp.expectation(tp.all_scores(g), thr)
    lf = np.full(caller_id(len(g.left) - 1) + 1, -np.inf)
    rf = np.full(caller_id(len(g.right) - 1) + 1, -np.inf)
    best_l: Dict[int, float] = {}
    best_r: Dict[int, float] = {}
    for s, i, j in hits:
        best_l[i] = max(best_l.get(i, -1.0), s)
        best_r[j] = max(best_r.get(j, -1.0), s)
    for i, s in best_l.items():
        lf[caller_id(i)] = np.nan if i % 7 == 3 else 0.25 * s
    for j, s in best_r.items():
        rf[caller_id(j)] = 0.25 * s
    want = [(s, caller_id(i), caller_id(j)) for s, i, j in hits if s >= lf[caller_id(i)] and s >= rf[caller_id(j)]]
    return thr, lf, rf, want


# -------------------------------------------------------------------------------------------------------------- profiles
PROFILE_GRIDS = {"nsm_indel_raw_profile": "raw_indel_128", "nsm_jaccard_raw_profile": "raw_jaccard_32",
                 "nsm_indel_levels_profile": "levels_indel_one_word-cat2_lanes",
                 "nsm_jaccard_levels_profile": "levels_jaccard-cat2_lanes"}


def profile_case(name: str):
    """(ladder, pairs [T], {left caller id: best}, {right caller id: best}) with caller ids ``caller_id(k)``; an item
    without a hit at ladder[0] has best -1.0."""
    g = tp.grid(name)
    scores = tp.probes_of(g)
    ladder = sorted({scores[(2 * len(scores)) // 3], scores[(5 * len(scores)) // 6], scores[-1]})  # (items without a hit on both sides)
    hits = tp.expectation(tp.all_scores(g), ladder[0])
    pairs = [sum(1 for h in hits if h[0] >= t) for t in ladder]
    left = {caller_id(i): -1.0 for i in range(len(g.left))}
    right = {caller_id(j): -1.0 for j in range(len(g.right))}
    for s, i, j in hits:
        left[caller_id(i)] = max(left[caller_id(i)], s)
        right[caller_id(j)] = max(right[caller_id(j)], s)
    return ladder, pairs, left, right


# ----------------------------------------------------------------------------------------------------------------- top-k
TOP_K = (1, 3, 300)  # (300: more than the 229 right items, the entry clamps it)
TOP_K_GRIDS = {"nsm_indel_raw_top_k": "raw_indel_64", "nsm_jaccard_raw_top_k": "raw_jaccard_16",
               "nsm_indel_raw_top_k_grouped": "raw_indel_128", "nsm_jaccard_raw_top_k_grouped": "raw_jaccard_32",
               "nsm_indel_levels_top_k": "levels_indel_one_word-cat2_lanes", "nsm_jaccard_levels_top_k": "levels_jaccard-cat1_partition"}


def row_counts(hits: Sequence[tuple], n_left: int) -> List[int]:
    count = [0] * n_left
    for _, i, _ in hits:
        count[i] += 1
    return count


def banned_pairs(name: str, hits: Sequence[tuple]) -> Optional[Tuple[List[int], List[int]]]:
    """The blacklist of a levels top-k case: every third hit of the oracle's list, and a pair that is no hit."""
    if not name.startswith("levels"):
        return None
    picked = list(hits[::3])
    return [h[1] for h in picked] + [0], [h[2] for h in picked] + [10 ** 6]


def top_k_case(name: str):
    """(threshold, allowed hits = the oracle's at the threshold without the banned pairs, banned): the first probe
    threshold, from the top, at which the allowed hits leave rows with no record, rows with fewer than 3 and rows with more."""
    g = tp.grid(name)
    all_hits = tp.all_scores(g)
    for thr in reversed(tp.probes_of(g)):
        hits = tp.expectation(all_hits, thr)
        banned = banned_pairs(name, hits)
        gone = set(zip(*banned)) if banned else set()
        allowed = [h for h in hits if (h[1], h[2]) not in gone]
        count = row_counts(allowed, len(g.left))
        if 0 in count and any(0 < c < 3 for c in count) and any(c > 3 for c in count):
            return thr, allowed, banned
    return None


# ---------------------------------------------------------------------------------------------------------- listed pairs
PAIR_COUNTS = (1, 63, 64, 65, 1000)
PAIRS_GRIDS = {"nsm_indel_raw_pairs": "raw_indel_256", "nsm_jaccard_raw_pairs": "raw_jaccard_64",
               "nsm_indel_levels_pairs": "levels_indel_multi_word_128", "nsm_jaccard_levels_pairs": "levels_jaccard"}
UNMAPPED_LEFT, UNMAPPED_RIGHT = (3, 40), (0, 100, 228)  # items the caller's id -> row maps give no row (-1)


def pair_list(g: tp.ProbeGrid, n_pairs: int):
    """``n_pairs`` (i, j) records in caller ids (item k is id k here): most name two items, a tenth repeat an earlier
    record, and some carry an id outside the maps (negative, or beyond the last) or one whose map entry is -1."""
    rng = random.Random(4100 + n_pairs)
    n, m = len(g.left), len(g.right)
    out: List[Tuple[int, int]] = []
    for p in range(n_pairs):
        roll = rng.random()
        if roll < 0.1 and out:
            out.append(out[rng.randrange(len(out))])
        elif roll < 0.15:
            out.append((rng.choice((-1, n, n + 7, 2 ** 31 - 1)), rng.randrange(m)))
        elif roll < 0.2:
            out.append((rng.randrange(n), rng.choice((-5, m, 2 ** 31 - 1))))
        elif roll < 0.25:
            out.append((rng.choice(UNMAPPED_LEFT), rng.choice(UNMAPPED_RIGHT)))
        else:
            out.append((rng.randrange(n), rng.randrange(m)))
    return out


def pair_scores(g: tp.ProbeGrid, pairs: Sequence[Tuple[int, int]]) -> List[float]:
    """``grid.lookup_pairs``' definition on the oracle's list: the pair's score, -1.0 when it has none or names no row."""
    by_pair = {(i, j): s for s, i, j in tp.all_scores(g)}
    return [-1.0 if (i in UNMAPPED_LEFT or j in UNMAPPED_RIGHT) else by_pair.get((i, j), -1.0) for i, j in pairs]


# ------------------------------------------------------------------------------------------------------------------ sort
SORT_SIZES = ((8191, 8191 + 300), (8193, 8193 + 300), (20011, 20011 + 77))  # (live records n, capacity C)


def sort_records(n_total: int, seed: int, id_limit: int) -> np.ndarray:
    """``n_total`` distinct records [score, i, j] as a float64 [n][2] array (the 16-byte layout): few distinct scores, so
    that the order of most neighbours is decided by i and j; ids below ``id_limit``."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n_total, 2), dtype=np.float64)
    rec[:, 0] = rng.integers(0, 50, size=n_total) / 49.0
    ij = rec.view(np.int32).reshape(n_total, 4)
    flat = rng.choice(id_limit * id_limit, size=n_total, replace=False)
    ij[:, 2], ij[:, 3] = flat // id_limit, flat % id_limit
    return rec


def sorted_records(rec: np.ndarray) -> np.ndarray:
    ij = rec.view(np.int32).reshape(-1, 4)
    return rec[np.lexsort((ij[:, 3], ij[:, 2], -rec[:, 0]))]
