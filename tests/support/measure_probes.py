"""The probe grids of tests/support/threshold_probes.py as the token-set measures beside Jaccard see them (mean = Dice,
smaller = overlap, left = containment): a thin layer over ``threshold_probes`` (the grids, the probe classes) and
``set_measures`` (the definitions in plain Python, which are the yardstick here).  It generates one kind of grid of its
own, ``sharp_grid``: pairs at whose score ``need`` of csrc/set_measure.hpp starts with no slack, which the seeded grids lack.

Shared by tests/test_cpu_measure_probes.py (do the grids hold, under every measure, the ties, ulp twins and tight families
that a threshold probe needs? -- no device) and tests/test_gpu_measure_probes.py (the kernels at those probes)."""
import dataclasses
from typing import Callable, Dict, List

import numpy as np

from support import probe_tables
from support import set_measures as sm
from support import threshold_probes as tp

MEASURES = sm.MEASURES
RAW = tp.RAW_JACCARD
LEVELS = tp.LEVELS_JACCARD
LEVELS_WIDTHS = (32, 64)  # the levels items hold at most 40 ids: both widths hold them
PROBE_CAP = 40            # probes per grid and measure; holds every family score, twin member, shared score and landmark

_VIEWS: Dict[str, tp.ProbeGrid] = {}


def _view(name: str, make: Callable[[], tp.ProbeGrid]) -> tp.ProbeGrid:
    if name not in _VIEWS:
        _VIEWS[name] = make()
    return _VIEWS[name]


def without_empty_rows(g: tp.ProbeGrid) -> tp.ProbeGrid:
    """A RAW grid without its empty right rows; a record's j is the index in the filtered list."""
    assert g.raw and all(g.left)

    def make():
        kept = [j for j, row in enumerate(g.right) if row]
        new_j = {j: q for q, j in enumerate(kept)}
        return dataclasses.replace(g, name=f"{g.name}-no_empty", right=[g.right[j] for j in kept],
                                   subset=[(i, new_j[j]) for i, j in g.subset if j in new_j])

    return _view(f"{g.name}-no_empty", make)


def grid_for(name: str, measure: str) -> tp.ProbeGrid:
    """The probe grid ``name`` as ``measure`` may see it: as it is for "mean" and "left" (an empty right row scores 0.0;
    no left row is empty); for "smaller" a RAW grid loses its empty right rows (the wrappers raise the whole-grid
    ZeroDivisionError otherwise).  The levels grids hold no empty level."""
    g = tp.grid(name)
    return without_empty_rows(g) if measure == "smaller" and g.raw else g


def swapped(g: tp.ProbeGrid) -> tp.ProbeGrid:
    """The RAW grid without empty rows, left and right exchanged."""
    base = without_empty_rows(g) if not all(g.right) else g
    return _view(f"{base.name}-swapped", lambda: dataclasses.replace(
        base, name=f"{base.name}-swapped", left=base.right, right=base.left, subset=[(j, i) for i, j in base.subset]))


# --------------------------------------------------------------------------------------------------------- yardstick
_ALL: Dict[tuple, list] = {}


def all_scores(g: tp.ProbeGrid, measure: str) -> list:
    """The definition's records ``(score, i, j)`` at threshold 0.0 in canonical order: no measure is negative, so every
    defined pair that the category predicate admits.  ``measure`` may be "union".  Cached; never modified."""
    key = (g.name, measure)
    if key not in _ALL:
        if g.raw:
            _ALL[key] = sm.raw_hits(measure, g.left, g.right, 0.0)
        else:
            keep = (lambda i, j: True) if g.mode == tp.CAT_NONE else \
                (lambda i, j: sm.category_match(int(g.cat_l[i]), int(g.cat_r[j]), g.mode))
            _ALL[key] = sm.levels_hits(measure, g.left, g.right, 0.0, keep)
    return _ALL[key]


def probes_of(g: tp.ProbeGrid, measure: str, cap: int = PROBE_CAP) -> List[float]:
    return tp.probes(all_scores(g, measure), cap, g.family_pairs())


_PAIRS: Dict[tuple, list] = {}


def pair_scores(g: tp.ProbeGrid, measure: str) -> List[float]:
    """The definition's score of EVERY pair, (i, j) row-major, as a listed-pairs query gives it: no category predicate, and
    -1.0 where the measure divides by zero."""
    key = (g.name, measure)
    if key not in _PAIRS:
        from oracle.compare import compare_terms

        f = sm.DEFINITIONS[measure]
        score = f if g.raw else (lambda a, b: compare_terms(a, b, f))
        out = []
        for a in g.left:
            for b in g.right:
                try:
                    out.append(score(a, b))
                except ZeroDivisionError:
                    out.append(-1.0)
        _PAIRS[key] = out
    return _PAIRS[key]


_BOUND: Dict[tuple, Callable] = {}


def scorer(measure: str) -> Callable:
    """``all_scores`` of one measure as the one-argument callable that ``probe_checks`` takes (one object per measure)."""
    return _BOUND.setdefault(("scores", measure), lambda g: all_scores(g, measure))


def prober(measure: str) -> Callable:
    return _BOUND.setdefault(("probes", measure), lambda g: probes_of(g, measure))


# -------------------------------------------------------------------------------------------- floors that leave need() no slack
GUESS = {"mean": lambda a, b, eff: eff * float(a + b) * 0.5, "smaller": lambda a, b, eff: eff * float(min(a, b)),
         "left": lambda a, b, eff: eff * float(a)}
NUM = {"mean": lambda k: 2 * k, "smaller": lambda k: k, "left": lambda k: k}
DEN = {"mean": lambda a, b: a + b, "smaller": lambda a, b: min(a, b), "left": lambda a, b: a}
SHARP_WIDTH = 32


def sharp_sizes(measure: str, limit: int = SHARP_WIDTH, count: int = 6) -> List[tuple]:
    """(a, b, k) with ``ceil(guess(a, b, s)) == k + 1`` for the pair's own score ``s = num(k) / den(a, b)``: the product
    ``s * den`` rounds above k, so ``QuotientMeasure::need`` (csrc/set_measure.hpp), which starts at ``ceil(guess) - 1``,
    starts exactly ON the answer k -- a start one higher skips it.  The ``count`` cases with the fewest ids (the smallest
    denominator at which the product rounds up is 25)."""
    import math

    cases = [(a, b, k) for a in range(1, limit + 1) for b in range(1, limit + 1) for k in range(1, min(a, b) + 1)
             if a + b - k <= 50 and math.ceil(GUESS[measure](a, b, NUM[measure](k) / DEN[measure](a, b))) == k + 1]
    out, per_score = [], {}
    for a, b, k in sorted(cases, key=lambda c: (c[0] + c[1], c)):  # (at most two cases per score: several scores)
        s = NUM[measure](k) / DEN[measure](a, b)
        if per_score.get(s, 0) < 2 and len(out) < count:
            per_score[s] = per_score.get(s, 0) + 1
            out.append((a, b, k))
    return out


def _ids_of_distinct_signature_bits(n: int) -> List[int]:
    """``n`` ids whose hash bits in the rows' signature words differ pairwise (found with ``tables.signatures`` itself): for
    rows over them the signature bound of an intersection is the intersection's size, so that ``need`` alone decides."""
    from napkon_string_matching_amd import tables

    ids = np.arange(4096, dtype=np.int32).reshape(-1, 1)
    bits = tables.signatures(ids, np.ones(len(ids), dtype=np.int32))
    seen, out = set(), []
    for v, bit in zip(ids[:, 0].tolist(), bits.tolist()):
        if bit not in seen and bin(bit).count("1") == 1:
            seen.add(bit)
            out.append(v)
    assert len(out) >= n, len(out)
    return out[:n]


def sharp_grid(measure: str) -> tp.ProbeGrid:
    """A RAW grid of width 32 with one left and one right row per ``sharp_sizes`` case -- a ids against b ids that share k,
    all over 50 ids of distinct signature bits -- and a few small rows around them.  ``subset`` lists the planted pairs."""
    def make():
        pool = _ids_of_distinct_signature_bits(50)
        left, right, planted = [], [], []
        for a, b, k in sharp_sizes(measure):
            planted.append((len(left), len(right)))
            left.append(pool[:a])
            right.append(pool[:k] + pool[a: a + b - k])
        for q in range(9):  # (fillers: more than one row group on the left, other classes on the right)
            left.append(pool[q: q + 1 + q % 4])
            right.append(pool[2 * q: 2 * q + 1 + q % 5])
        return tp.ProbeGrid(f"sharp_need-{measure}", "jaccard", True, left, right, size=SHARP_WIDTH, subset=planted)

    return _view(f"sharp_need-{measure}", make)


def sharp_scores(measure: str) -> List[float]:
    g = sharp_grid(measure)
    by_pair = {(i, j): s for s, i, j in all_scores(g, measure)}
    return sorted({by_pair[p] for p in g.subset})


# ------------------------------------------------------------------------------------------------------------ tables
def raw_tables(g: tp.ProbeGrid, dev):
    """(left table, right table) of a RAW grid or one of its views."""
    if g.name in tp.RAW_JACCARD:
        return probe_tables.raw_jaccard_tables(g, dev)
    from napkon_string_matching_amd import tables

    def make():
        def padded(rows):
            ids = np.full((len(rows), g.size), -1, dtype=np.int32)
            for r, row in enumerate(rows):
                ids[r, : len(row)] = row
            return ids

        lt = tables.SetTable.from_padded(padded(g.left), "left", dev, width=g.size)
        rt = tables.SetTable.from_padded(padded(g.right), "right", dev, width=g.size)
        assert lt.width == rt.width == g.size and lt.n == len(g.left) and rt.n == len(g.right)
        assert not lt.has_empty and not rt.has_empty
        return lt, rt

    return probe_tables.cached(g.name, make)


def levels_tables(g: tp.ProbeGrid, dev, width: int):
    """(left table, right table) of a levels grid at ``width``, without a partition (the per-item sweeps ask for that)."""
    from napkon_string_matching_amd import tables

    def make():
        vocabulary = tables.Vocabulary()
        lt = tables.SetTable.from_levels(g.left, "left", dev, vocabulary, width=width, categories=g.cat_l, category_mode=g.mode,
                                         partition=False)
        rt = tables.SetTable.from_levels(g.right, "right", dev, vocabulary, width=width, categories=g.cat_r,
                                         category_mode=g.mode, partition=False)
        assert lt.width == rt.width == width and lt.seg is None and rt.seg is None
        return lt, rt

    return probe_tables.cached((g.name, "measures", width), make)
