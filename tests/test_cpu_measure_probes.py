"""The probe grids under the token-set measures beside Jaccard, through the definitions alone (no GPU): are they worth
running?

tests/test_gpu_measure_probes.py puts thresholds and per-item floors exactly on scores of intersection_vs_mean (Dice),
intersection_vs_smaller (overlap) and intersection_vs_left (containment), and one ulp to either side.  That pins the
measures' pruning decisions (``need``, ``bound``, ``up_first``, ``part`` / ``later`` of csrc/set_measure.hpp) only if the
grids of tests/support/threshold_probes.py hold, under each measure, what those decisions are weakest against: scores
shared by many pairs (1.0 above all: whole classes of pairs under overlap and containment), distinct scores a few ulps
apart, and tight families -- pairs whose bound is met with equality.  This file checks those premises, and that the
yardstick itself (the definitions of tests/support/set_measures.py through ``oracle.compare.compare_terms``) is the native
oracle's where the two overlap: under Jaccard.

The counts below are properties of the definitions on seeded grids, measured once and written down; a change of a generator
or of a definition shows here before it lets the GPU file pass vacuously.
"""
import math

import numpy as np
import pytest

from support import best_matches as bm
from support import measure_probes as mp
from support import threshold_probes as tp
from support.probe_checks import ban_unique_bests

CASES = [(n, m) for n in mp.RAW + mp.LEVELS for m in mp.MEASURES]

# (grid, measure) -> (records, distinct probes, pairs at exactly 1.0, pairs at 0.0, most records at 1.0 in one left row)
RAW_COUNTS = {
    ("raw_jaccard_16", "mean"): (18320, 15, 273, 8470, 13),
    ("raw_jaccard_16", "smaller"): (17760, 15, 3531, 7910, 78),
    ("raw_jaccard_16", "left"): (18320, 14, 1669, 8470, 78),
    ("raw_jaccard_32", "mean"): (18320, 15, 290, 9081, 13),
    ("raw_jaccard_32", "smaller"): (17600, 15, 3421, 8361, 131),
    ("raw_jaccard_32", "left"): (18320, 14, 1815, 9081, 67),
    ("raw_jaccard_64", "mean"): (18320, 16, 198, 8792, 12),
    ("raw_jaccard_64", "smaller"): (17600, 15, 3069, 8072, 92),
    ("raw_jaccard_64", "left"): (18320, 14, 1400, 8792, 72),
}
# (grid, measure) -> (records, distinct probes, ulp twins in all, pairs at 0.0)
LEVELS_COUNTS = {
    ("levels_jaccard", "mean"): (19007, 38, 60, 6976),
    ("levels_jaccard", "smaller"): (19007, 31, 118, 6976),
    ("levels_jaccard", "left"): (19007, 34, 70, 6976),
    ("levels_jaccard-cat1_partition", "mean"): (9896, 38, 29, 2952),
    ("levels_jaccard-cat1_partition", "smaller"): (9896, 31, 65, 2952),
    ("levels_jaccard-cat1_partition", "left"): (9896, 34, 35, 2952),
    ("levels_jaccard-cat2_lanes", "mean"): (10312, 38, 32, 3149),
    ("levels_jaccard-cat2_lanes", "smaller"): (10312, 31, 74, 3149),
    ("levels_jaccard-cat2_lanes", "left"): (10312, 32, 38, 3149),
}
EMPTY_RIGHT_ROWS = {"raw_jaccard_16": 7, "raw_jaccard_32": 9, "raw_jaccard_64": 9}


def _by_pair(records):
    return {(i, j): s for s, i, j in records}


@pytest.mark.parametrize("name", mp.RAW + mp.LEVELS)
def test_union_through_the_yardstick_is_the_native_oracle(name):
    """Same records, same order, same bits: the plain-Python definitions, ``compare_terms`` and the category predicate of
    this yardstick against ``oracle.native`` on the grids both can score."""
    g = tp.grid(name)
    got = mp.all_scores(g, "union")
    assert got == tp.all_scores(g) and len(got) == (RAW_COUNTS[(name, "mean")] if g.raw else LEVELS_COUNTS[(name, "mean")])[0]
    assert mp.probes_of(g, "union") == tp.probes_of(g)


@pytest.mark.parametrize("name,measure", CASES)
def test_probe_classes(name, measure):
    g = mp.grid_for(name, measure)
    records = mp.all_scores(g, measure)
    assert records == sorted(records, key=lambda h: (-h[0], h[1], h[2]))
    scores = mp.probes_of(g, measure)
    assert scores == sorted(set(scores)) and scores[0] > 0.0 and scores[-1] <= 1.0
    # the cap cuts nothing: every family score, twin member, shared score and landmark is a probe
    assert scores == tp.probes(records, 10 ** 6, g.family_pairs()) and len(scores) <= mp.PROBE_CAP
    count = {}
    for s, _, _ in records:
        count[s] = count.get(s, 0) + 1
    shared = tp.shared_scores(records)
    assert len(shared) == 8 and count[shared[0]] >= 20 and set(shared) <= set(scores)
    assert set(tp.landmark_scores(records)) <= set(scores)
    lb, _ = bm.bests(records)
    assert any(s in set(lb.values()) for s in scores), "no probe is a left item's best score"
    assert bm.row_gap(records) > 0.0
    ranks = tp.RowRanks(records)
    assert all(ranks.kth_tie(k) is not None for k in (1, 3, 64))
    ones_in_row = {}
    for s, i, _ in records:
        if s == 1.0:
            ones_in_row[i] = ones_in_row.get(i, 0) + 1
    if g.raw:
        n_records, n_probes, ones, zeros, most_ones = RAW_COUNTS[(name, measure)]
        assert (len(records), len(scores), count.get(1.0, 0), count.get(0.0, 0), max(ones_in_row.values())) == \
            (n_records, n_probes, ones, zeros, most_ones)
        assert len(records) == g.pairs and 1.0 in scores
        # a RAW score is one quotient of integers up to 128: no ulp twins, and no later step for a family to be tight in
        assert not tp.ulp_twins(records) and not g.tight
        if measure in ("smaller", "left"):
            assert ones > 1000  # whole classes of pairs sit on the threshold 1.0
            # ... and some left row holds more than 64 of them: k = 64 ends inside a tie, at every width
            assert most_ones > 64
            row = next(lst for lst, _ in ranks.rows.values() if len(lst) > 64 and lst[64][0] == 1.0)
            kept = [h for h in ranks.cut(1.0, 64) if h[1] == row[0][1]]
            assert kept == sorted(row[:64], key=lambda t: (-t[0], t[1], t[2])) and row[64] not in kept and row[63][2] < row[64][2]
        return
    n_records, n_probes, twins_in_all, zeros = LEVELS_COUNTS[(name, measure)]
    assert (len(records), len(scores), len(tp.ulp_twins(records, n=1000)), count.get(0.0, 0)) == \
        (n_records, n_probes, twins_in_all, zeros)
    assert (len(records) == g.pairs) == (g.mode == tp.CAT_NONE)
    chosen = tp.ulp_twins(records)
    assert len(chosen) == 8 and all(a in scores and b in scores and 0 < tp._ulps_apart(a, b) <= 4 for a, b in chosen)
    # every tight family: 12 pairs of ONE score, and that score is a probe
    by_pair = _by_pair(records)
    assert len(g.tight) == 7
    for fam, pairs in g.tight.items():
        at = {by_pair[p] for p in pairs}
        assert len(pairs) == tp.FAMILY_SIZE and len(at) == 1 and at <= set(scores), (fam, at)
    # best matches with a blacklist: enough items whose best is unique, so that banning it moves the best
    assert len(ban_unique_bests(records)[0]) >= 3


@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name", mp.LEVELS)
def test_tight_families_are_tight_under_the_measures(name, measure):
    """Only the level that step 1 compares differs and every later level is identical, so every later step scores exactly
    1.0 and meets the step bound ``later(a1, b1, k)`` of the levels sweep with equality where that bound is 1.0.  A
    ``drop1`` copy is a subset at step 1: ``part(a1, b1, min(a1, b1))``, the class bound, is its exact step-1 score.  An
    ``add1`` copy contains the left set at step 1: containment and overlap score it 1.0 there."""
    from support import set_measures as sm

    g = mp.grid_for(name, measure)
    by_pair = _by_pair(mp.all_scores(g, measure))
    f = sm.DEFINITIONS[measure]
    for fam, pairs in g.tight.items():
        for i, j in pairs:
            a, b = g.left[i], g.right[j]
            depth, lv = len(a), tp.step1_level(a)
            assert len(b) == depth and all(set(a[q]) == set(b[q]) for q in range(lv + 1, depth)), fam
            sa, sb = set(a[lv]), set(b[lv])
            r1 = f(a[lv], b[lv])
            if fam.startswith("drop1"):
                assert sb < sa and len(sb) == len(sa) - 1
                assert r1 == {"mean": 2 * len(sb) / (len(sa) + len(sb)), "smaller": 1.0, "left": len(sb) / len(sa)}[measure]
            else:
                assert sa < sb and len(sb) == len(sa) + 1
                assert r1 == {"mean": 2 * len(sa) / (len(sa) + len(sb)), "smaller": 1.0, "left": 1.0}[measure]
            score, factor = 0.0, 1.0
            for step in range(1, depth + 1):
                factor /= 2
                score += (r1 if step == 1 else 1.0) * factor
            assert by_pair[(i, j)] == score, (fam, i, j)


@pytest.mark.parametrize("name", mp.RAW)
def test_grid_views(name):
    """The grid without its empty right rows (what "smaller" may see) and the swapped grid."""
    g = tp.grid(name)
    empty = [j for j, row in enumerate(g.right) if not row]
    assert len(empty) == EMPTY_RIGHT_ROWS[name] and all(g.left)
    assert mp.grid_for(name, "mean") is g and mp.grid_for(name, "left") is g
    f = mp.grid_for(name, "smaller")
    assert f.left == g.left and f.right == [row for row in g.right if row] and len(f.right) == len(g.right) - len(empty)
    assert f.subset and all(set(f.right[j]) <= set(f.left[i]) for i, j in f.subset)
    s = mp.swapped(g)
    assert s is mp.swapped(f) and s.left == f.right and s.right == f.left and s.size == g.size
    assert len(s.left) in (220, 222) and len(s.right) == 80
    # under "mean" and "left" the empty right rows score 0.0 against every left row
    for measure in ("mean", "left"):
        by_pair = _by_pair(mp.all_scores(g, measure))
        assert all(by_pair[(i, j)] == 0.0 for i in range(len(g.left)) for j in empty)


@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name", mp.RAW)
def test_swapped_grid_is_the_transpose_for_symmetric_measures_only(name, measure):
    """Dice and overlap are symmetric: the swapped grid's records are the transposed records.  Containment is not: the
    swapped grid divides by the other set's size."""
    g = mp.without_empty_rows(tp.grid(name))
    s = mp.swapped(g)
    transposed = sorted(((x, j, i) for x, i, j in mp.all_scores(g, measure)), key=lambda h: (-h[0], h[1], h[2]))
    swapped = mp.all_scores(s, measure)
    assert len(swapped) == len(transposed) == g.pairs
    if measure == "left":
        assert swapped != transposed
        differ = sum(1 for a, b in zip(sorted(swapped, key=lambda h: h[1:]), sorted(transposed, key=lambda h: h[1:])) if a != b)
        assert differ > 1000
    else:
        assert swapped == transposed
    assert len(mp.probes_of(s, measure)) >= 10


# ------------------------------------------------------------------------------------------------------------- need()
GUESS, NUM, DEN = mp.GUESS, mp.NUM, mp.DEN  # the start guess, numerator and denominator of the three measures, restated


def test_need_starts_at_or_below_the_least_intersection():
    """A host restatement of ``QuotientMeasure::need`` of csrc/set_measure.hpp (the same double operations in the same
    order, in numpy) -- it guards the arithmetic of the start guess, not the compiled kernel.  ``need(a, b, eff)`` starts at
    ``ceil(guess) - 1`` clamped to [0, min(a, b) + 1] and walks up on the exact score, so it returns the least k with
    ``score(a, b, k) >= eff`` iff the start is at most that k.  Every a, b <= 64 with a non-zero denominator, every
    attainable score as ``eff`` and one ulp to either side of it."""
    cases = 0
    for measure in mp.MEASURES:
        for a in range(65):
            for b in range(65):
                den = DEN[measure](a, b)
                if den == 0:
                    continue
                top = min(a, b)
                score = np.array([NUM[measure](k) for k in range(top + 1)], dtype=np.float64) / np.float64(den)
                assert (np.diff(score) > 0).all()
                eff = np.concatenate([np.nextafter(score, 0.0), score, np.nextafter(score, 2.0)])
                eff = eff[eff > 0.0]  # (eff <= 0 returns 0 before any guess)
                least = np.searchsorted(score, eff, side="left")  # the scores below eff: the least k that reaches it
                start = np.minimum(np.ceil(GUESS[measure](a, b, eff)), float(top + 2)).astype(np.int64) - 1
                start = np.clip(start, 0, top + 1)
                assert (start <= least).all(), (measure, a, b, eff[start > least][:3])
                # (and it is a useful start: never more than two below the answer)
                assert (least - start <= 2).all(), (measure, a, b)
                cases += len(eff)
    assert cases > 800000
    # the scalar form, on one case by hand: Dice of 3 and 5 ids at eff = 0.5 needs 2 (2 * 2 / 8)
    assert math.ceil(GUESS["mean"](3, 5, 0.5)) - 1 == 1 and 2 * 1 / 8 < 0.5 <= 2 * 2 / 8


@pytest.mark.parametrize("measure", mp.MEASURES)
def test_grids_whose_floors_leave_need_no_slack(measure):
    """The probe grids hold almost no pair on which a ``need`` that starts one too high could show on the device: the
    product ``score * den`` has to round above the intersection k (no denominator below 25 does that), and the signature
    bound has to be exactly k, or the pair passes it anyway.  ``measure_probes.sharp_grid`` plants such pairs: checked here
    with the arithmetic of the guess and with ``tables.signatures``."""
    from napkon_string_matching_amd import tables

    sizes = mp.sharp_sizes(measure)
    assert len(sizes) == 6 and all(max(a, b) <= mp.SHARP_WIDTH and 25 <= mp.DEN[measure](a, b) for a, b, _ in sizes)
    assert all(mp.DEN[measure](a, b) >= 25 for a, b, _ in mp.sharp_sizes(measure, count=10 ** 6))
    g = mp.sharp_grid(measure)
    assert len(g.subset) == 6 and len(g.left) > 8 and all(g.left) and all(g.right)
    by_pair = _by_pair(mp.all_scores(g, measure))

    def signature(rows):
        ids = np.full((len(rows), g.size), -1, dtype=np.int32)
        for r, row in enumerate(rows):
            ids[r, : len(row)] = sorted(row)
        return tables.signatures(ids, np.array([len(r) for r in rows], dtype=np.int32))

    sig_l, sig_r = signature(g.left), signature(g.right)
    for (i, j), (a, b, k) in zip(g.subset, sizes):
        assert (len(g.left[i]), len(g.right[j]), len(set(g.left[i]) & set(g.right[j]))) == (a, b, k)
        s = by_pair[(i, j)]
        assert s == mp.NUM[measure](k) / mp.DEN[measure](a, b) and 0.0 < s < 1.0
        # the start ceil(guess) - 1 is the answer itself ...
        assert math.ceil(mp.GUESS[measure](a, b, s)) - 1 == k
        assert mp.NUM[measure](k - 1) / mp.DEN[measure](a, b) < s
        # ... and the signature bound says k, not more: one more needed and the pair is dropped
        assert bin(int(sig_l[i]) & int(sig_r[j])).count("1") == k and int(sig_l[i]) >> 58 == 0
    assert len(mp.sharp_scores(measure)) >= 2
