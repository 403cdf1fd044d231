"""The checks that the probe files share: tests/test_gpu_threshold_probes.py and tests/test_gpu_best.py (Jaccard and Indel
against the native oracle) and tests/test_gpu_measure_probes.py (the token-set measures against their definitions).

``check`` and ``check_top_k`` take the yardstick as two callables, ``all_scores(g)`` (the canonical list of every pair) and
``probes_of(g)`` (the scores to cut at); their defaults are the native oracle's, tests/support/threshold_probes.py.  The
floor and best-match helpers work on a record list that the caller brings."""
import math

import numpy as np

from support import best_matches as bm
from support import probe_tables
from support import threshold_probes as tp

_AT = {}


def _pairs_at(g, all_scores=tp.all_scores):
    """score -> the pairs that score exactly that."""
    key = (g.name, all_scores)
    if key not in _AT:
        at = {}
        for s, i, j in all_scores(g):
            at.setdefault(s, set()).add((i, j))
        _AT[key] = at
    return _AT[key]


def check(g, route, run, all_scores=tp.all_scores, probes_of=tp.probes_of):
    """``run(thr)`` -> the kernel's (score, i, j) list."""
    all_hits = all_scores(g)
    scores = probes_of(g)
    seen = {}
    for thr in tp.thresholds_around(scores):
        want = tp.expectation(all_hits, thr)
        got = seen[thr] = run(thr)
        assert got == want, f"{g.name} / {route} at threshold {thr!r}: {probe_tables.first_difference(got, want)}"
    at = _pairs_at(g, all_scores)
    for s in scores:  # (implied by the equalities above; spelled out, since it is what these thresholds are for)
        here, below, above = ({(i, j) for _, i, j in seen[t]} for t in (s, math.nextafter(s, 0.0), math.nextafter(s, 2.0)))
        assert at[s] and at[s] <= here and at[s] <= below and not at[s] & above, \
            f"{g.name} / {route}: pairs scoring exactly {s!r}: {sorted(at[s] - here)[:4]} lost at it, " \
            f"{sorted(at[s] - below)[:4]} lost one ulp below, {sorted(at[s] & above)[:4]} kept one ulp above"


def check_top_k(g, route, run, groups=None, all_scores=tp.all_scores, probes_of=tp.probes_of):
    """``run(k, thr)`` -> the kernel's list.  The expectation: the oracle's list cut at the threshold, per left item the
    first k in (score descending, j ascending) -- of the groups' representatives when ``groups`` is given."""
    all_hits = all_scores(g)
    ranks = tp.RowRanks(all_hits, None if groups is None else groups.tolist())
    thresholds = tp.thresholds_around(probes_of(g))
    for k in (1, 3, 64):
        # a threshold on the score of some row's k-th record: floor and threshold coincide, the tie goes to the lower j
        tie = ranks.kth_tie(k)
        assert tie is not None or k == 64  # (with categories a row may hold fewer than 64 records)
        for thr in sorted(set(thresholds) | set(tp.thresholds_around([] if tie is None else [tie]))):
            want = ranks.cut(thr, k)
            got = run(k, thr)
            assert got == want, f"{g.name} / {route} k={k} at threshold {thr!r}: {probe_tables.first_difference(got, want)}"


# ------------------------------------------------------------------------------------------- floors and best matches
def same(got, want, what):
    """Records and doubles equal, bit for bit (scores are never NaN or -0.0)."""
    assert len(got) == len(want), f"{what}: {len(got)} records, expected {len(want)}"
    assert np.array_equal(got.i, want.i) and np.array_equal(got.j, want.j), f"{what}: pairs differ"
    assert np.array_equal(got.score.view(np.int64), want.score.view(np.int64)), f"{what}: scores differ"


def ban_unique_bests(records):
    """The best pair of every third left item, where it is the item's only pair at that score: banning it moves the best."""
    rows = {}
    for s, i, j in records:  # (score descending: a row's first record is its best)
        rows.setdefault(i, []).append((s, j))
    banned = {(i, r[0][1]) for i, r in rows.items() if i % 3 == 0 and r[0][0] > 0.0 and (len(r) == 1 or r[1][0] < r[0][0])}
    return banned, {i: r[0][0] for i, r in rows.items()}


def floor_cases(records, n, m):
    """Floors of a small grid: every item's own best; left floors one ulp above it (admits nothing for the item); a mix."""
    lb, rb = bm.bests(records)
    own_l, own_r = [lb.get(i, 0.0) for i in range(n)], [rb.get(j, 0.0) for j in range(m)]
    above = [math.nextafter(x, 2.0) if i % 2 else x for i, x in enumerate(own_l)]
    mixed = [math.nan if j % 5 == 1 else -math.inf if j % 5 == 2 else x for j, x in enumerate(own_r)]
    return [(own_l, None), (None, own_r), (own_l, own_r), (above, mixed), (None, None)]


def check_small(records, n, m, floor_grid, best, what):
    from napkon_string_matching_amd import grid

    hits = bm.to_hits(records)
    for prune in (True, False):
        for lf, rf in floor_cases(records, n, m):
            arr = lambda f: None if f is None else np.array(f, dtype=np.float64)
            same(floor_grid(0.0, arr(lf), arr(rf), prune), bm.to_hits(bm.floors_plain(records, lf, rf)), f"{what} prune={prune}")
        for margin, mutual in ((0.0, False), (0.0, True), (0.25, False), (0.25, True), (2.0, True)):
            same(best(margin, 0.0, mutual, prune), grid.best_of_hits(hits, margin, mutual, n, m),
                 f"{what} margin {margin} mutual {mutual} prune={prune}")
