"""The token-set measures beside Jaccard -- intersection_vs_mean (Dice, "mean"), intersection_vs_smaller (overlap,
"smaller"), intersection_vs_left (containment, "left") -- with thresholds and per-item floors put exactly on scores of the
definitions, and one ulp to either side.

Under a measure every query is an instantiation of the per-item sweep kernels (``jaccard_top_k_kernel``,
``jaccard_levels_top_k_kernel`` with the sinks TopLists, ScoreTally and FloorGate) or of the listed-pair kernels with
``RuntimeMeasure`` of csrc/set_measure.hpp in place of the Jaccard quotient, and every pruning decision is the measure's
own: ``need`` (the least intersection that reaches a floor), ``bound`` and ``up_first`` (the class walk), ``part`` /
``later`` (the step bound ``0.5 part + tail * later + 1e-6`` of the levels sweep and its ``score + factor + 1e-9`` exit).
The rule: a bound may drop a pair only when the pair is strictly below ``max(threshold, floor)``.  A ``need`` that starts
one too high, a ``later`` that is too tight or a walk that ends a class early shows only on a pair that sits exactly on its
floor; the grids here hold such pairs for every measure (tests/test_cpu_measure_probes.py checks that without a device):
1.0 shared by whole size classes under overlap and containment, ulp twins, and tight families whose bounds are met with
equality; for ``need`` itself a grid of its own (``test_need_without_slack``).

The yardstick is tests/support/measure_probes.py: the plain-Python definitions of tests/support/set_measures.py, for levels
through ``oracle.compare.compare_terms``.  Records are compared as canonical ``(score, i, j)`` tuples, scores bit for bit.
Every query runs pruned and unpruned; the levels grids at widths 32 and 64 (the ``W = 64`` instantiation of the levels
sweep); at most ``measure_probes.PROBE_CAP`` = 40 probes x 3 thresholds per route, every family score and ulp twin among
them.
"""
import math
import random

import numpy as np
import pytest

from support import best_matches as bm
from support import measure_probes as mp
from support import probe_tables
from support import set_measures as sm
from support import threshold_probes as tp
from support.probe_checks import ban_unique_bests, check, check_small, check_top_k, same

pytestmark = pytest.mark.gpu
PRUNE = {"prune": True, "no_prune": False}
ABOVE_ONE = math.nextafter(1.0, 2.0)


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _case(dev, name, measure, width=None):
    """(grid, left table, right table, keyword arguments of the levels wrappers) of a probe grid under a measure."""
    g = mp.grid_for(name, measure)
    if g.raw:
        return (g, *mp.raw_tables(g, dev), {})
    return (g, *mp.levels_tables(g, dev, width), dict(category_mode=g.mode))


def _yardstick(measure):
    return dict(all_scores=mp.scorer(measure), probes_of=mp.prober(measure))


# --------------------------------------------------------------------------------------------------- threshold grids
@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name", mp.RAW)
def test_raw_grid(dev, name, measure, route):
    """``need`` and the class walk of the RAW sweep through FloorGate without floors: 1.0 shared by every subset pair
    (overlap) and every pair whose right row holds the left row (containment), 0.0 by every disjoint pair."""
    from napkon_string_matching_amd import grid

    g, lt, rt, _ = _case(dev, name, measure)
    run = lambda thr: grid.jaccard_raw_grid(lt, rt, thr, prune=PRUNE[route], capacity=g.pairs + 1, measure=measure).as_tuples()
    check(g, route, run, **_yardstick(measure))
    assert run(0.0) == mp.all_scores(g, measure)
    assert run(ABOVE_ONE) == []  # (no measure exceeds 1.0)


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("width", mp.LEVELS_WIDTHS)
@pytest.mark.parametrize("name", mp.LEVELS)
def test_levels_grid(dev, name, width, measure, route):
    """The step bound of the levels sweep on tight families: every step after the first scores exactly 1.0."""
    from napkon_string_matching_amd import grid

    g, lt, rt, kw = _case(dev, name, measure, width)
    run = lambda thr: grid.jaccard_levels_grid(lt, rt, thr, prune=PRUNE[route], capacity=g.pairs + 1, measure=measure,
                                               **kw).as_tuples()
    check(g, route, run, **_yardstick(measure))
    assert run(0.0) == mp.all_scores(g, measure)
    assert run(ABOVE_ONE) == []


@pytest.mark.parametrize("measure", mp.MEASURES)
def test_capacity_one_grows_and_retries(dev, measure):
    """A mid probe with room for one record: the wrapper's second launch at the counted size gives the same list."""
    from napkon_string_matching_amd import grid

    for name, width in (("raw_jaccard_32", None), ("levels_jaccard-cat2_lanes", 64)):
        g, lt, rt, kw = _case(dev, name, measure, width)
        probes = mp.probes_of(g, measure)
        thr = probes[len(probes) // 2]
        want = tp.expectation(mp.all_scores(g, measure), thr)
        assert len(want) > 1
        call = grid.jaccard_raw_grid if g.raw else grid.jaccard_levels_grid
        for prune in (True, False):
            assert call(lt, rt, thr, prune=prune, capacity=1, measure=measure, **kw).as_tuples() == want, (name, prune)


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
def test_need_without_slack(dev, measure, route):
    """``need`` gates the signature bound of the RAW sweep (``ub < need``: the pair is dropped unscored).  On the seeded
    grids that bound is almost never as small as the intersection where it matters, so a ``need`` one too high passes them.
    ``measure_probes.sharp_grid`` plants pairs over ids of distinct signature bits -- the bound IS the intersection k -- at
    sizes where ``score * den`` rounds above k, so that the start ``ceil(guess) - 1`` is k itself: a threshold, a left floor
    or a right floor on such a pair's score must keep it."""
    from napkon_string_matching_amd import grid

    g = mp.sharp_grid(measure)
    lt, rt = mp.raw_tables(g, dev)
    records = mp.all_scores(g, measure)
    everything = bm.to_hits(records)
    run = lambda thr, lf=None, rf=None: grid.jaccard_raw_floor_grid(lt, rt, thr, lf, rf, prune=PRUNE[route], capacity=g.pairs + 1,
                                                                    measure=measure)
    check(g, route, lambda thr: run(thr).as_tuples(), all_scores=mp.scorer(measure), probes_of=lambda _: mp.sharp_scores(measure))
    n, m = len(g.left), len(g.right)
    by_pair = {(i, j): s for s, i, j in records}
    for i, j in g.subset:
        s = by_pair[(i, j)]
        for floor, kept in ((math.nextafter(s, 0.0), True), (s, True), (math.nextafter(s, 2.0), False)):
            for lf, rf in ((np.full(n, floor), None), (None, np.full(m, floor)), (np.full(n, floor), np.full(m, floor))):
                got = run(0.0, lf, rf)
                same(got, grid.filter_by_floors(everything, lf, rf), f"{g.name} / {route} floors {floor!r}")
                assert ((s, i, j) in got.as_tuples()) == kept
        top = grid.jaccard_raw_top_k(lt, rt, 64, s, prune=PRUNE[route], measure=measure).as_tuples()
        assert (s, i, j) in top and top == tp.RowRanks(records).cut(s, 64)


# -------------------------------------------------------------------------------------------------------------- top-k
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name", mp.RAW)
def test_raw_top_k(dev, name, measure, route, grouped):
    """TopLists under a measure with k in 1, 3, 64: the list's floor rises to scores that whole classes share."""
    from napkon_string_matching_amd import grid

    g, lt, rt, _ = _case(dev, name, measure)
    groups = tp.groups_of(g) if grouped else None
    check_top_k(g, f"top_k-{route}-{'grouped' if grouped else 'plain'}",
                lambda k, thr: grid.jaccard_raw_top_k(lt, rt, k, thr, prune=PRUNE[route], groups=groups, measure=measure).as_tuples(),
                groups, **_yardstick(measure))


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", ["smaller", "left"])
@pytest.mark.parametrize("name", mp.RAW)
def test_raw_top_64_ends_inside_a_run_of_ones(dev, name, measure, route):
    """Some left row has more than 64 right rows at exactly 1.0: its list is full of ties with the floor, and a later 1.0
    enters only with a lower j."""
    from napkon_string_matching_amd import grid

    g, lt, rt, _ = _case(dev, name, measure)
    ones = {}
    for s, i, j in mp.all_scores(g, measure):
        if s == 1.0:
            ones.setdefault(i, []).append(j)
    full = {i: sorted(js)[:64] for i, js in ones.items() if len(js) > 64}
    assert full
    for thr in (0.0, 1.0):
        got = grid.jaccard_raw_top_k(lt, rt, 64, thr, prune=PRUNE[route], measure=measure).as_tuples()
        for i, js in full.items():
            assert [(s, j) for s, gi, j in got if gi == i] == [(1.0, j) for j in js], (name, measure, route, thr, i)


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("width", mp.LEVELS_WIDTHS)
@pytest.mark.parametrize("name", mp.LEVELS)
def test_levels_top_k(dev, name, width, measure, route):
    """The ``score + factor + 1e-9`` exit of the levels sweep against a rising list floor."""
    from napkon_string_matching_amd import grid

    g, lt, rt, kw = _case(dev, name, measure, width)
    check_top_k(g, f"top_k-{route}",
                lambda k, thr: grid.jaccard_levels_top_k(lt, rt, k, thr, prune=PRUNE[route], measure=measure, **kw).as_tuples(),
                **_yardstick(measure))


# ------------------------------------------------------------------------------------------- floors and best matches
def _calls(dev, name, measure, width):
    """(grid, floor grid, best) through the grid-level wrappers: ``floors(thr, left_floor, right_floor, prune, banned=None,
    stats=None)``, ``best(margin, thr, mutual, prune, banned=None, stats=None)``; ``banned`` only on levels grids."""
    from napkon_string_matching_amd import grid

    g, lt, rt, kw = _case(dev, name, measure, width)
    cap = g.pairs  # (room for every pair: no retry)
    if g.raw:
        return (g, lambda thr, lf, rf, prune, banned=None, stats=None: grid.jaccard_raw_floor_grid(
                    lt, rt, thr, lf, rf, prune=prune, stats=stats, capacity=cap, measure=measure),
                lambda m, thr, mutual, prune, banned=None, stats=None: grid.jaccard_raw_best(
                    lt, rt, m, thr, mutual, prune=prune, stats=stats, measure=measure))
    return (g, lambda thr, lf, rf, prune, banned=None, stats=None: grid.jaccard_levels_floor_grid(
                lt, rt, thr, lf, rf, prune=prune, banned=banned, stats=stats, capacity=cap, measure=measure, **kw),
            lambda m, thr, mutual, prune, banned=None, stats=None: grid.jaccard_levels_best(
                lt, rt, m, thr, mutual, prune=prune, banned=banned, stats=stats, measure=measure, **kw))


GRIDS = [(n, None) for n in mp.RAW] + [(n, w) for n in mp.LEVELS for w in mp.LEVELS_WIDTHS]
GRID_IDS = [n if w is None else f"{n}@{w}" for n, w in GRIDS]


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name,width", GRIDS, ids=GRID_IDS)
def test_floor_grids(dev, name, width, measure, route):
    """FloorGate with real floors: for every probe s the left items whose best is s get a floor one ulp below s, on s and
    one ulp above it, every other item its own best (and one NaN and one -inf floor per side) -- as left floors only, right
    floors only, and both."""
    from napkon_string_matching_amd import grid

    g, floors, _ = _calls(dev, name, measure, width)
    records = mp.all_scores(g, measure)
    everything = bm.to_hits(records)
    n, m = len(g.left), len(g.right)
    probes = mp.probes_of(g, measure)
    lb, _ = bm.bests(records)
    assert any(s in set(lb.values()) for s in probes), "no probe is a left item's best score"
    for s in probes:
        for floor in (math.nextafter(s, 0.0), s, math.nextafter(s, 2.0)):
            left, right = (np.array(f) for f in bm.probe_floors(records, s, floor, n, m))
            for lf, rf in ((left, None), (None, right), (left, right)):
                got = floors(0.0, lf, rf, PRUNE[route])
                same(got, grid.filter_by_floors(everything, lf, rf), f"{g.name} / {measure} / {route} floor {floor!r} "
                     f"{'left' if rf is None else 'right' if lf is None else 'both'}")
    # neither: the threshold grid
    for thr in (probes[0], probes[len(probes) // 2], math.nextafter(probes[-1], 2.0)):
        same(floors(thr, None, None, PRUNE[route]), bm.to_hits(tp.expectation(records, thr)),
             f"{g.name} / {measure} / {route} no floors at {thr!r}")


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name,width", GRIDS, ids=GRID_IDS)
def test_best_matches(dev, name, width, measure, route):
    """Best matches (a profile sweep, then a floor grid at ``best - margin``) with margin 0, a margin that splits a row's
    runners-up, and one that keeps everything; on the levels grids with the unique bests of every third item banned."""
    from napkon_string_matching_amd import grid

    g, _, best = _calls(dev, name, measure, width)
    records = mp.all_scores(g, measure)
    ban = None
    if not g.raw:
        banned, old_best = ban_unique_bests(records)
        assert len(banned) >= 3
        records = [r for r in records if (r[1], r[2]) not in banned]
        ban = (np.array([p[0] for p in sorted(banned)]), np.array([p[1] for p in sorted(banned)]))
    gap = bm.row_gap(records)
    probes = mp.probes_of(g, measure)
    for thr in (0.0, probes[len(probes) // 2]):
        want_from = bm.to_hits(tp.expectation(records, thr))
        for margin in (0.0, gap, 2.0):
            for mutual in (False, True):
                got = best(margin, thr, mutual, PRUNE[route], ban)
                same(got, grid.best_of_hits(want_from, margin, mutual, len(g.left), len(g.right)),
                     f"{g.name} / {measure} / {route} margin {margin!r} mutual {mutual} at {thr!r}")
                if ban is not None and margin == 0.0 and thr == 0.0 and not mutual:
                    new_best = dict(zip(got.i.tolist(), got.score.tolist()))
                    # (every banned pair was its item's only pair at that score: each of those bests must have moved)
                    assert all(new_best.get(i, -1.0) < old_best[i] for i, _ in banned), "a banned item's best did not move"
                    assert sum(1 for i, _ in banned if i in new_best) >= 3


@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name,width", GRIDS, ids=GRID_IDS)
def test_pruning_is_monotone(dev, name, width, measure):
    """The floor sweep's bounds are compared against max(threshold, floor) >= the profile's threshold: every counter of
    the floor grid is at most the profile sweep's.  Without pruning a RAW sweep scores every pair (each is defined: no left
    row is empty, and "smaller" sees no empty right row)."""
    g, floors, best = _calls(dev, name, measure, width)
    probes = mp.probes_of(g, measure)
    for thr in (0.0, probes[len(probes) // 2]):
        for mutual in (False, True):
            stats = []
            best(0.0, thr, mutual, True, None, stats)
            profile, floor = stats
            assert len(profile) == len(floor) == 4 and all(f <= p for f, p in zip(floor, profile)), (g.name, thr, mutual, stats)
    if g.raw:
        stats = []
        floors(0.0, None, None, False, None, stats)
        assert stats[3] == g.pairs, (g.name, stats)


# ------------------------------------------------------------------------------------------------------ small shapes
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_small_shapes(dev, n, m, measure):
    """Fewer left rows than a wave's 8, exactly 8, one more (a last row group of one); every right row of ONE size, so that
    one size class holds exactly m rows: one short of a 64-lane batch, a full one, one more.  Six tokens: ties abound."""
    from napkon_string_matching_amd import grid, tables

    rng = random.Random(n * 1000 + m)
    size = 1 + (n + m) % 4
    left = [rng.sample(range(6), rng.randint(1, 5)) for _ in range(n)]
    right = [rng.sample(range(6), size) for _ in range(m)]
    records = sm.raw_hits(measure, left, right, 0.0)
    assert len(records) == n * m and {len(r) for r in right} == {size}

    def padded(side):
        ids = np.full((len(side), 16), -1, dtype=np.int32)
        for r, row in enumerate(side):
            ids[r, : len(row)] = row
        return ids

    lt = tables.SetTable.from_padded(padded(left), "left", dev, width=16)
    rt = tables.SetTable.from_padded(padded(right), "right", dev, width=16)
    check_small(records, n, m,
                lambda thr, lf, rf, prune: grid.jaccard_raw_floor_grid(lt, rt, thr, lf, rf, prune=prune, measure=measure),
                lambda margin, thr, mutual, prune: grid.jaccard_raw_best(lt, rt, margin, thr, mutual, prune=prune, measure=measure),
                f"{measure} {n} x {m} of size {size}")


# ----------------------------------------------------------------------------------------------------------- profiles
@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name,width", GRIDS, ids=GRID_IDS)
def test_profiles(dev, name, width, measure, route):
    """ScoreTally under a measure: one call with a ladder of 64 rungs, each on a probe or one ulp beside it."""
    from napkon_string_matching_amd import grid

    g, lt, rt, kw = _case(dev, name, measure, width)
    ladder = tp.thresholds_around(mp.probes_of(g, measure))[:64]
    assert 30 <= len(ladder) <= 64
    want = grid.profile_of_hits(bm.to_hits(tp.expectation(mp.all_scores(g, measure), ladder[0])), ladder, len(g.left), len(g.right))
    call = grid.jaccard_raw_profile if g.raw else grid.jaccard_levels_profile
    got = call(lt, rt, ladder, prune=PRUNE[route], measure=measure, **kw)
    assert got.pairs.tolist() == want.pairs.tolist() and len(set(got.pairs.tolist())) > 10
    assert got.left_best.tolist() == want.left_best.tolist() and got.right_best.tolist() == want.right_best.tolist()


# -------------------------------------------------------------------------------------------------------- listed pairs
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name,width", GRIDS, ids=GRID_IDS)
def test_listed_pairs(dev, name, width, measure):
    """Every pair of the grid through the listed-pair kernels (no pruning there, no category predicate): the definition bit
    for bit."""
    from napkon_string_matching_amd import grid

    g, lt, rt, _ = _case(dev, name, measure, width)
    n, m = len(g.left), len(g.right)
    pi, pj = np.arange(n).repeat(m), np.tile(np.arange(m), n)
    call = grid.jaccard_raw_pairs if g.raw else grid.jaccard_levels_pairs
    want = mp.pair_scores(g, measure)
    assert call(lt, rt, pi, pj, measure=measure).tolist() == want and min(want) >= 0.0


@pytest.mark.parametrize("name", mp.RAW)
def test_listed_pairs_with_empty_right_rows_under_smaller(dev, name):
    """The unfiltered grid: the threshold queries refuse it (ZeroDivisionError for the whole grid), a listed pair with an
    empty right row is -1.0."""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    lt, rt = mp.raw_tables(g, dev)
    n, m = len(g.left), len(g.right)
    pi, pj = np.arange(n).repeat(m), np.tile(np.arange(m), n)
    want = mp.pair_scores(g, "smaller")
    empty = [j for j, row in enumerate(g.right) if not row]
    assert empty and all(want[i * m + j] == -1.0 for i in range(n) for j in empty) and want.count(-1.0) == n * len(empty)
    assert grid.jaccard_raw_pairs(lt, rt, pi, pj, measure="smaller").tolist() == want
    with pytest.raises(ZeroDivisionError):
        grid.jaccard_raw_grid(lt, rt, 0.5, measure="smaller")


# -------------------------------------------------------------------------------------------------- swapped orientation
@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("measure", mp.MEASURES)
@pytest.mark.parametrize("name", mp.RAW)
def test_swapped_orientation(dev, name, measure, route):
    """Left and right exchanged (220 or 222 left rows against 80 right rows): Dice and overlap give the transposed records,
    containment -- which divides by the LEFT set -- does not."""
    from napkon_string_matching_amd import grid

    plain = mp.without_empty_rows(tp.grid(name))
    g = mp.swapped(plain)
    lt, rt = mp.raw_tables(g, dev)
    run = lambda thr: grid.jaccard_raw_grid(lt, rt, thr, prune=PRUNE[route], capacity=g.pairs + 1, measure=measure).as_tuples()
    check(g, route, run, **_yardstick(measure))
    ranks = tp.RowRanks(mp.all_scores(g, measure))
    for thr in tp.thresholds_around(mp.probes_of(g, measure)):
        got = grid.jaccard_raw_top_k(lt, rt, 3, thr, prune=PRUNE[route], measure=measure).as_tuples()
        want = ranks.cut(thr, 3)
        assert got == want, f"{g.name} / {measure} / {route} k=3 at {thr!r}: {probe_tables.first_difference(got, want)}"
    pl, pr = mp.raw_tables(plain, dev)
    unswapped = grid.jaccard_raw_grid(pl, pr, 0.0, prune=PRUNE[route], capacity=g.pairs + 1, measure=measure).as_tuples()
    transposed = sorted(((s, j, i) for s, i, j in unswapped), key=lambda h: (-h[0], h[1], h[2]))
    assert len(transposed) == g.pairs
    assert (run(0.0) == transposed) == (measure != "left")
