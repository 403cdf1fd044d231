"""The grids of tests/support/threshold_probes.py through the oracle alone (no GPU): are they worth running?

tests/test_gpu_threshold_probes.py puts thresholds exactly on oracle scores, and one ulp to either side, for every route of
the fast-path kernels.  That only pins the kernels' pruning bounds if the grids hold what the bounds are weakest against:
scores shared by many pairs, distinct scores a few ulps apart, and tight families -- pairs whose every later step scores
exactly 1.0, so that the bound a kernel derives from the threshold is met with equality.  This file checks those premises,
the cut of the cached oracle list against real oracle calls, and the fast top-k cuts against their definitions.
"""
import math
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import pytest

from support import threshold_probes as tp
from support.grouped import group_cut


def _lcs(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0
        for y in range(1, len(b) + 1):
            up = row[y]
            row[y] = diag + 1 if x == b[y - 1] else max(up, row[y - 1])
            diag = up
    return row[-1]


def _indel_ratio(a, b):
    """The reference's operation order (normalized distance -> similarity -> percent -> / 100), in plain Python."""
    if not a or not b:
        return 0.0
    total = len(a) + len(b)
    return (1.0 - (total - 2 * _lcs(a, b)) / total) * 100.0 / 100.0


def _jaccard(a, b):
    return len(set(a) & set(b)) / len(set(a) | set(b))


def _by_pair(all_hits):
    return {(i, j): s for s, i, j in all_hits}


@pytest.mark.parametrize("name", tp.EVERY)
def test_cut_of_the_cached_list_is_a_real_oracle_call(name):
    """For three probes (the lowest, the middle and the highest) and a threshold on, below or above each."""
    g = tp.grid(name)
    all_hits = tp.all_scores(g)
    assert all_hits == sorted(all_hits, key=lambda h: (-h[0], h[1], h[2]))
    assert (len(all_hits) == g.pairs) == (g.mode == tp.CAT_NONE)
    scores = tp.probes_of(g)
    picks = [scores[0], math.nextafter(scores[len(scores) // 2], 0.0), math.nextafter(scores[-1], 2.0)]
    with ThreadPoolExecutor(3) as pool:  # (the C oracle runs without the interpreter lock)
        real = list(pool.map(lambda thr: tp.oracle_call(g, thr), picks))
    for thr, want in zip(picks, real):
        got = tp.expectation(all_hits, thr)
        assert got == want and got == [h for h in all_hits if h[0] >= thr], thr
    assert real[0] and len(real[1]) < len(real[0]) and not any(h[0] <= scores[-1] for h in real[2])


@pytest.mark.parametrize("name", tp.EVERY)
def test_probe_classes(name):
    g = tp.grid(name)
    all_hits = tp.all_scores(g)
    scores = tp.probes_of(g)
    assert (10 if g.raw else 16) <= len(scores) <= 40 and scores == sorted(set(scores)) and scores[0] > 0.0
    count = {}
    for s, _, _ in all_hits:
        count[s] = count.get(s, 0) + 1
    shared = tp.shared_scores(all_hits)
    assert len(shared) == 8 and count[shared[0]] >= 20 and set(shared) <= set(scores)
    assert len(tp.landmark_scores(all_hits)) == 8 and set(tp.landmark_scores(all_hits)) <= set(scores)  # none dropped by the cap
    thresholds = tp.thresholds_around(scores)
    assert all({math.nextafter(s, 0.0), s, math.nextafter(s, 2.0)} <= set(thresholds) for s in scores)
    if g.raw:
        # A RAW score is one correctly rounded quotient of two integers below 1025: distinct ones lie at least 2^-20 apart,
        # so ulp twins cannot exist here, and nothing is planted as a tight family (there is no later step).
        assert not tp.ulp_twins(all_hits) and not g.tight
        return
    twins = tp.ulp_twins(all_hits, n=1000)
    assert len(twins) >= 4
    chosen = tp.ulp_twins(all_hits)
    assert 4 <= len(chosen) <= 8 and all(a in scores and b in scores for a, b in chosen)
    assert all(0 < tp._ulps_apart(a, b) <= 4 for a, b in chosen)
    # every family: at least 10 pairs, all of ONE score, and that score is a probe
    by_pair = _by_pair(all_hits)
    assert len(g.tight) >= 4
    for fam, pairs in g.tight.items():
        at = {by_pair[p] for p in pairs}
        assert len(pairs) >= 10 and len(at) == 1 and at <= set(scores), (fam, at)
    for p in g.anagram:
        assert by_pair[p] in scores


@pytest.mark.parametrize("name", tp.LEVELS)
def test_tight_families_are_tight(name):
    """Recomputed in plain Python, not by the oracle.  Only the level that step 1 compares differs between the two items,
    both have S levels, so steps 2 .. S score exactly 1.0 and the oracle's sum is ``ratio_1 / 2 + 1/4 + ... + 2^-S`` in its
    own order of additions, bit for bit.  Exactly, that is ``score - ratio_1 / 2 == 1/2 - 2^-S``; in doubles each of the
    oracle's S - 1 additions below 1.0 may round by half an ulp (2^-54), which is all the identity is allowed to miss by."""
    g = tp.grid(name)
    by_pair = _by_pair(tp.all_scores(g))
    ratio = _indel_ratio if g.kind == "indel" else _jaccard
    exact = 0
    for fam, pairs in g.tight.items():
        for i, j in pairs:
            a, b = g.left[i], g.right[j]
            depth = len(a)
            lv = tp.step1_level(a)
            assert len(b) == depth != 2, fam
            if g.kind == "indel":
                assert a[lv] != b[lv] and all(a[q] == b[q] for q in range(depth) if q != lv), fam
            else:
                assert set(a[lv]) != set(b[lv]) and all(set(a[q]) == set(b[q]) for q in range(lv + 1, depth)), fam
            r1 = ratio(a[lv], b[lv])
            assert 0.0 < r1 < 1.0
            score, factor = 0.0, 1.0
            for step in range(1, depth + 1):
                factor /= 2
                score += (r1 if step == 1 else 1.0) * factor
            assert by_pair[(i, j)] == score, (fam, i, j)
            tail = 0.5 - 2.0 ** -depth
            miss = abs(Fraction(score) - Fraction(0.5 * r1) - Fraction(tail))
            assert miss <= (depth - 1) * Fraction(1, 2 ** 54), (fam, i, j)
            exact += score - 0.5 * r1 == tail
    assert exact >= 10  # (and for many pairs the doubles themselves satisfy it)
    for i, j in g.anagram:  # the histogram of level 2 is its partner's, the string is not
        a, b = g.left[i], g.right[j]
        assert sorted(a[2]) == sorted(b[2]) and a[2] != b[2] and _indel_ratio(a[2], b[2]) < 1.0
        assert all(a[q] == b[q] for q in range(len(a)) if q != 2) and len(a) == len(b) >= 3


def test_one_word_probes_lie_on_both_sides_of_the_routing_thresholds():
    """The library routes one-word grids by 0.55 (the probe's threshold) and 0.7 (the split path)."""
    for name in tp.ONE_WORD:
        scores = tp.probes_of(tp.grid(name))
        for cut in (0.55, 0.7):
            assert any(s < cut for s in scores) and any(s > cut for s in scores), (name, cut)
        by_pair = _by_pair(tp.all_scores(tp.grid(name)))
        g = tp.grid(name)
        fam = [by_pair[pairs[0]] for pairs in g.tight.values()]
        assert any(s >= 0.7 for s in fam)
        # ... and a family WITH later steps (their bounds met with equality) lies between the two: the default route there
        later = [by_pair[pairs[0]] for pairs in g.tight.values() if len(g.left[pairs[0][0]]) >= 3]
        assert any(0.55 < s < 0.7 for s in later), later


@pytest.mark.parametrize("name", tp.EVERY)
def test_edges_the_grid_was_built_for(name):
    g = tp.grid(name)
    assert 70 <= len(g.left) <= 90 and len(g.right) == 64 * 3 + 37
    rows = lambda items: items if g.raw else [lv for it in items for lv in it]
    for side in (g.left, g.right):
        lens = {len(r) for r in rows(side)}
        if name.startswith("levels_indel_one_word"):  # 33 .. 64 units: the finish kernel's two-sweep LCS
            assert 48 < max(lens) <= 64
        else:
            assert max(lens) == g.size if g.kind == "indel" or g.raw else max(lens) <= g.size
        if name.startswith("raw_indel"):
            edges = [64] if g.size == 64 else [e for e in (65, 128, 129, 256, 257, 512) if e <= g.size]
            assert set(edges) <= lens and 0 in lens
    if name.startswith("raw_jaccard"):
        assert all(g.left) and not all(g.right) and len(g.subset) > 20
        by_pair = _by_pair(tp.all_scores(g))
        for i, j in g.subset:
            assert set(g.right[j]) <= set(g.left[i]) and by_pair[(i, j)] == len(set(g.right[j])) / len(g.left[i])
        count = {}
        for s, _, _ in tp.all_scores(g):
            count[s] = count.get(s, 0) + 1
        assert all(count[s] >= 100 for s in (1 / 2, 1 / 3, 2 / 3))
    if name.startswith("levels_indel_one_word"):
        assert g.size == 64 and {len(it) for it in g.left} >= {1, 2, 3, 4, 5, 6}
    if name.startswith("levels_indel_multi_word"):
        # a substituted copy of a step-1 string that fills the row: n1 = 2 * stride (1024 at stride 512)
        n1 = {len(g.left[i][1]) + len(g.right[j][1]) for pairs in g.tight.values() for i, j in pairs}
        assert 2 * g.size in n1 and 2 * g.size - 1 in n1
        assert len(g.duplicates) == 24 and all(g.right[j] == g.right[0] for j in g.duplicates)
    if name.startswith("levels_jaccard"):
        assert g.size == 32 and len(g.subset) == 10
        for i, j in g.subset:
            assert len(g.left[i]) == len(g.right[j]) and all(set(b) <= set(a) for a, b in zip(g.left[i], g.right[j]))
        for it in g.left + g.right:
            assert all(set(lo) <= set(hi) for lo, hi in zip(it, it[1:])) and it[0]
    if g.mode != tp.CAT_NONE:
        assert (g.cat_l == 0).any() and (g.cat_r == 0).any()
        assert g.partition == (g.mode == tp.CAT_INTERSECT)


@pytest.mark.parametrize("name", ["raw_indel_64", "raw_jaccard_32", "levels_indel_one_word-cat2_lanes", "levels_jaccard"])
def test_row_ranks_are_the_definitions(name):
    """``RowRanks.cut`` against the rank cut of the top-k tests and ``group_cut`` of tests/support/grouped.py."""
    g = tp.grid(name)
    all_hits = tp.all_scores(g)
    groups = tp.groups_of(g).tolist()
    assert 10 < len(set(groups)) < len(groups)
    plain, grouped = tp.RowRanks(all_hits), tp.RowRanks(all_hits, groups)

    def rank_cut(hits, k):
        rows = {}
        for h in hits:
            rows.setdefault(h[1], []).append(h)
        kept = [r for lst in rows.values() for r in sorted(lst, key=lambda t: (-t[0], t[2]))[:k]]
        return sorted(kept, key=lambda t: (-t[0], t[1], t[2]))

    scores = tp.probes_of(g)
    tie = plain.kth_tie(3)
    assert tie is not None
    for thr in tp.thresholds_around([scores[0], scores[len(scores) // 2], scores[-1], tie]):
        hits = tp.expectation(all_hits, thr)
        for k in (1, 3, 64):
            assert plain.cut(thr, k) == rank_cut(hits, k), (thr, k)
            assert grouped.cut(thr, k) == group_cut(hits, groups, k), (thr, k)
    # at the k-th record's own score the (k + 1)-th of the same score is cut: the tie goes to the lower j
    row = next(lst for lst, _ in plain.rows.values() if len(lst) > 3 and lst[2][0] == lst[3][0] == tie)
    kept = [h for h in plain.cut(tie, 3) if h[1] == row[0][1]]
    assert len(kept) == 3 and row[3] not in kept and row[2] in kept and row[2][2] < row[3][2]
