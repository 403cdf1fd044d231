"""The cases of tests/test_gpu_memory_contract.py that do not need a GPU to state: which grid, which threshold, which
capacities, and what the oracle says must come out.  tests/test_cpu_memory_contract.py checks their premises with the
oracle alone (enough hits to overflow every "too small" buffer, caller ids with gaps, top-k rows of every fill).

Grids: tests/support/threshold_probes.py (70 .. 90 x 229 items: several row batches, three full right tiles and a partial
one), any_operands.py for the two general kernels.  The nsm_set_* and nsm_edit_* entries of the additive headers run the
cases of their nsm_jaccard_* / nsm_indel_* siblings on the same grids; what must come out is then stated by the
plain-Python definitions (measure_probes.py / set_measures.py, edit_distance.py), never by the native oracle.
"""
import random
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle.compare import compare_terms, level_index_pairs
from support import any_operands as ao
from support import edit_distance as ed
from support import measure_probes as mp
from support import threshold_probes as tp

SMALL_CAPACITIES = (1, 63, 64, 65)  # around a wavefront's 64 records
START_COUNT = 5                     # a hit buffer that already holds records: hits are appended behind them


def capacities(count: int) -> List[int]:
    """0 (with ``hits = NULL``), the small ones, and the oracle's count - 1, the count, the count + 1."""
    return [0, *SMALL_CAPACITIES, count - 1, count, count + 1]


# ------------------------------------------------------------------- the additive headers: one more argument, a code
# A VARIANT names the yardstick of a case: None -- the native oracle, for the entries of nsm_hip.h; a token-set measure
# (nsm_hip_measures.h) or a Levenshtein metric (nsm_hip_edit.h) -- the plain-Python definitions of set_measures.py /
# edit_distance.py, for the nsm_set_* / nsm_edit_* entry that takes the sibling's arguments and the variant's code.
MEASURES = mp.MEASURES  # mean, smaller, left (code 0, "union", only forwards)
METRICS = ed.METRICS    # edit, edit_within (code 0, "indel", only forwards)
CODE = {"mean": 1, "smaller": 2, "left": 3, "edit": 1, "edit_within": 2}


def additive(siblings) -> List[Tuple[str, str, str]]:
    """(entry, sibling, variant) for every nsm_set_* / nsm_edit_* entry beside the ``siblings`` and every code but 0."""
    out = []
    for sib in siblings:
        if sib.startswith("nsm_jaccard_"):
            out += [(sib.replace("nsm_jaccard_", "nsm_set_"), sib, v) for v in MEASURES]
        else:
            out += [(sib.replace("nsm_indel_", "nsm_edit_"), sib, v) for v in METRICS]
    return out


def grid_name(grids: Dict[str, str], sibling: str, variant: Optional[str] = None) -> str:
    """The sibling's grid of ``grids`` (TOP_K_GRIDS, PROFILE_GRIDS).  One exception: under "smaller" (overlap) every left
    row of the RAW grids of widths 16 and 32 has a right row that is a subset of it or holds it, so every row's best is
    1.0 -- no threshold leaves a row without a record; at width 64 there are such rows."""
    name = grids[sibling]
    return "raw_jaccard_64" if variant == "smaller" and name.startswith("raw_jaccard_") else name


def view(name: str, variant: Optional[str] = None) -> tp.ProbeGrid:
    """The probe grid as the variant's sweeps may see it ("smaller": a RAW grid without its empty right rows)."""
    return mp.grid_for(name, variant) if variant in MEASURES else tp.grid(name)


_TUPLES: Dict[str, tuple] = {}
_DW: Dict[str, dict] = {}
_EDIT: Dict[tuple, list] = {}


def _as_tuples(g: tp.ProbeGrid):
    """(left, right) with every string a tuple of code units (hashable): RAW item -> string, levels item -> [strings]."""
    if g.name not in _TUPLES:
        one = (lambda it: tuple(it)) if g.raw else (lambda it: [tuple(lv) for lv in it])
        _TUPLES[g.name] = ([one(it) for it in g.left], [one(it) for it in g.right])
    return _TUPLES[g.name]


def _distances(g: tp.ProbeGrid, pairs: Sequence[Tuple[int, int]]) -> dict:
    """{(a, b): (d, w)} for every (left string, right string) that the definition compares for the item ``pairs``: one
    ``ed.distance_table`` call where the pairs are most of all pairs, else one per distinct left string with the right
    strings it meets; both distances from one pass; cached per grid."""
    left, right = _as_tuples(g)
    known = _DW.setdefault(g.name, {})
    wanted: Dict[tuple, set] = {}
    for i, j in pairs:
        if g.raw:
            steps = [(left[i], right[j])]
        else:
            steps = [(left[i][p], right[j][q]) for p, q in level_index_pairs(len(left[i]), len(right[j]))]
        for a, b in steps:
            if (a, b) not in known:
                wanted.setdefault(a, set()).add(b)
    texts = sorted(set().union(*wanted.values()))
    if 2 * sum(len(bs) for bs in wanted.values()) > len(wanted) * len(texts):  # (most of all pairs: one call for them all)
        return ed.distance_table(sorted(wanted), texts, known)
    for a, bs in wanted.items():
        ed.distance_table([a], sorted(bs), known)
    return known


def edit_pair_scores(g: tp.ProbeGrid, metric: str, pairs: Sequence[Tuple[int, int]]) -> List[float]:
    """The definition's score of the item ``pairs`` of an Indel probe grid under a Levenshtein metric: RAW
    ``ed.score`` of the pair's distance; levels ``compare_terms`` with that as score_func."""
    left, right = _as_tuples(g)
    known = _distances(g, pairs)
    f = lambda a, b: ed.plain_score(metric, len(a), len(b), *known[a, b])
    return [f(left[i], right[j]) if g.raw else compare_terms(left[i], right[j], f) for i, j in pairs]


def edit_scores(g: tp.ProbeGrid, metric: str) -> list:
    """``tp.all_scores`` under a Levenshtein metric: the definition's records of every pair the category predicate admits
    (no score is negative), canonical order.  Cached; never modified."""
    if (g.name, metric) not in _EDIT:
        keep = (lambda i, j: True) if g.mode == tp.CAT_NONE else \
            (lambda i, j: ed.category_match(int(g.cat_l[i]), int(g.cat_r[j]), g.mode))
        pairs = [(i, j) for i in range(len(g.left)) for j in range(len(g.right)) if keep(i, j)]
        hits = [(s, i, j) for s, (i, j) in zip(edit_pair_scores(g, metric, pairs), pairs)]
        _EDIT[g.name, metric] = sorted(hits, key=lambda h: (-h[0], h[1], h[2]))
    return _EDIT[g.name, metric]


def scores(g: tp.ProbeGrid, variant: Optional[str] = None) -> list:
    """Every pair's record in canonical order by the variant's yardstick."""
    if variant is None:
        return tp.all_scores(g)
    return mp.all_scores(g, variant) if variant in MEASURES else edit_scores(g, variant)


def probes_of(g: tp.ProbeGrid, variant: Optional[str] = None) -> List[float]:
    return tp.probes_of(g) if variant is None else tp.probes(scores(g, variant), 40, g.family_pairs())


# ------------------------------------------------------------------------------------------------------ threshold grids
def low_threshold(g: tp.ProbeGrid, variant: Optional[str] = None) -> float:
    """The lowest threshold of the probe's own list: nearly every scored pair is a hit, so every wave appends."""
    return probes_of(g, variant)[0]


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


caller_id = ed.caller_id  # caller ids with gaps: item k reports 3 k + 2 (one definition for both files)


def floor_case(name: str, variant: Optional[str] = None):
    """(threshold, left floors, right floors, expected records) in CALLER ids ``caller_id(k)``: an item's floor is a quarter
    of its best score (NaN for every seventh left item: it admits nothing; -inf for an item without a hit)."""
    g = view(name, variant)
    thr = low_threshold(g, variant)
    hits = tp.expectation(scores(g, variant), thr)
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


def profile_case(name: str, variant: Optional[str] = None):
    """(ladder, pairs [T], {left caller id: best}, {right caller id: best}) with caller ids ``caller_id(k)``; an item
    without a hit at ladder[0] has best -1.0."""
    g = view(name, variant)
    cuts = probes_of(g, variant)
    low, mid = (2 * len(cuts)) // 3, (5 * len(cuts)) // 6
    if variant is not None:  # (overlap scores high: the lowest rung moves up the probe list until an item has no hit at it)
        best_l, best_r = {}, {}
        for s, i, j in scores(g, variant):
            best_l[i], best_r[j] = max(best_l.get(i, 0.0), s), max(best_r.get(j, 0.0), s)
        weakest = min(list(best_l.values()) + list(best_r.values()) + ([0.0] if len(best_l) < len(g.left) or len(best_r) < len(g.right) else []))
        while cuts[low] <= weakest and low < len(cuts) - 3:
            low += 1
        mid = max(mid, low + 1)
    ladder = sorted({cuts[low], cuts[mid], cuts[-1]})  # (items without a hit on both sides)
    hits = tp.expectation(scores(g, variant), ladder[0])
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


def top_k_case(name: str, variant: Optional[str] = None):
    """(threshold, allowed hits = the oracle's at the threshold without the banned pairs, banned): the first probe
    threshold, from the top, at which the allowed hits leave rows with no record, rows with fewer than 3 and rows with more."""
    g = view(name, variant)
    all_hits = scores(g, variant)
    for thr in reversed(probes_of(g, variant)):
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


def pair_scores(g: tp.ProbeGrid, pairs: Sequence[Tuple[int, int]], variant: Optional[str] = None) -> List[float]:
    """``grid.lookup_pairs``' definition on the oracle's list: the pair's score, -1.0 when it has none or names no row.
    With a variant: the definition's score of the two items (a measure that divides by zero: -1.0, as its header says)."""
    n, m = len(g.left), len(g.right)
    named = lambda i, j: 0 <= i < n and 0 <= j < m and i not in UNMAPPED_LEFT and j not in UNMAPPED_RIGHT
    if variant is None:
        by_pair = {(i, j): s for s, i, j in tp.all_scores(g)}
    elif variant in MEASURES:
        every = mp.pair_scores(g, variant)
        by_pair = {(i, j): every[i * m + j] for i, j in set(pairs) if named(i, j)}
    else:
        listed = sorted({p for p in pairs if named(*p)})
        by_pair = dict(zip(listed, edit_pair_scores(g, variant, listed)))
    return [by_pair.get((i, j), -1.0) if named(i, j) else -1.0 for i, j in pairs]


# ---------------------------------------------------------------------------------------------------------- edge support
SUPPORT_STATS_START = (11, 12, 13, 14, 15)  # what ``stats`` holds before the call: it is added to
SUPPORT_MIN_SCORE = 0.4                     # (edge_support.SCORES: 0.2 is below it, NaN scores never count)


def support_case():
    """(lists, nodes, min_score) of the ``nsm_support_hits`` case: ``edge_support.seeded_lists`` thinned to about 250
    records -- three cohorts pairwise and a self-join over the whole node space, with duplicates, both orientations,
    self-loops, NaN scores and scores below ``min_score`` -- and, in the middle, a list without records."""
    from napkon_string_matching_amd import grid
    from support import edge_support as es

    lists, nodes = es.seeded_lists(5, density=0.4)
    empty = grid.Hits(np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    return lists[:2] + [(empty, 0, 0)] + lists[2:], nodes, SUPPORT_MIN_SCORE


def support_case_with_bad_id(lists, nodes: int, side: str):
    """The lists with ONE id outside its list's range -- in a record whose score is below ``min_score``, so that only the
    range check can see it: ``i = left_ids`` ("i"), ``j = right_ids`` ("j") or ``i = -1`` ("negative"), in the last list."""
    from napkon_string_matching_amd import grid

    hits, left_base, right_base = lists[-1]
    score, i, j = hits.score.copy(), hits.i.copy(), hits.j.copy()
    at = len(score) // 2
    score[at] = 0.2
    if side == "j":
        j[at] = nodes - right_base
    else:
        i[at] = nodes - left_base if side == "i" else -1
    return lists[:-1] + [(grid.Hits(score, i, j), left_base, right_base)]


def support_records(hits) -> np.ndarray:
    """The 16-byte records [score, i, j] of a ``grid.Hits`` as a float64 [n][2] array."""
    rec = np.zeros((len(hits.score), 2), dtype=np.float64)
    rec[:, 0] = hits.score
    ij = rec.view(np.int32).reshape(-1, 4)
    ij[:, 2], ij[:, 3] = hits.i, hits.j
    return rec


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
