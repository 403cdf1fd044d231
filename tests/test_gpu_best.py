"""Floor grids (``nsm_*_floor_grid``: the top-k kernels with the gate sink of csrc/floor_gate.hpp) and best matches on the
GPU against the definitions: ``grid.filter_by_floors`` / ``grid.best_of_hits`` of the oracle's hit list -- the same records
and the same doubles after the canonical sort (tests/test_cpu_best.py checks those two against plain Python).

The probe grids (tests/support/threshold_probes.py) put a floor exactly on a best score shared by several right items, one
ulp below and one ulp above it: a comparison with a margin, or a bound that prunes a pair sitting on its floor, shows
there.  Tables are built as the probe tests of the threshold grids build them (imported, not copied)."""
import math
import random

import numpy as np
import pandas as pd
import pytest

from support import probe_tables
from support import best_matches as bm
from support import threshold_probes as tp
from support.probe_checks import ban_unique_bests as _ban_unique_bests, check_small as _check_small, same as _same

pytestmark = pytest.mark.gpu
PRUNE = {"prune": True, "no_prune": False}


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _calls(g, dev):
    """(floor grid, best) of a probe grid through the grid-level wrappers of its mode:
    ``floors(thr, left_floor, right_floor, prune, banned=None, stats=None)``, ``best(margin, thr, mutual, prune, banned=None,
    stats=None)``.  ``banned`` only on levels grids."""
    from napkon_string_matching_amd import grid

    cap = g.pairs  # (room for every pair: no retry)
    if g.raw:
        lt, rt = probe_tables.raw_indel_tables(g, dev) if g.kind == "indel" else probe_tables.raw_jaccard_tables(g, dev)
        fg, best = (grid.indel_raw_floor_grid, grid.indel_raw_best) if g.kind == "indel" else \
            (grid.jaccard_raw_floor_grid, grid.jaccard_raw_best)
        return (lambda thr, lf, rf, prune, banned=None, stats=None: fg(lt, rt, thr, lf, rf, prune=prune, stats=stats, capacity=cap),
                lambda m, thr, mutual, prune, banned=None, stats=None: best(lt, rt, m, thr, mutual, prune=prune, stats=stats))
    tabs = probe_tables.levels_indel_tables(g, dev, False) if g.kind == "indel" else probe_tables.levels_jaccard_tables(g, dev, False)
    fg, best = (grid.indel_levels_floor_grid, grid.indel_levels_best) if g.kind == "indel" else \
        (grid.jaccard_levels_floor_grid, grid.jaccard_levels_best)
    return (lambda thr, lf, rf, prune, banned=None, stats=None: fg(*tabs, thr, lf, rf, category_mode=g.mode, prune=prune,
                                                                   banned=banned, stats=stats, capacity=cap),
            lambda m, thr, mutual, prune, banned=None, stats=None: best(*tabs, m, thr, mutual, category_mode=g.mode, prune=prune,
                                                                        banned=banned, stats=stats))


# ------------------------------------------------------------------------------------------------------- probe grids
@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("name", tp.EVERY)
def test_floor_grids_on_probe_grids(dev, name, route):
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    floors, _ = _calls(g, dev)
    records = tp.all_scores(g)
    everything = bm.to_hits(records)
    n, m = len(g.left), len(g.right)
    probes = tp.probes_of(g)
    lb, _ = bm.bests(records)
    assert any(s in set(lb.values()) for s in probes), "no probe is a left item's best score"
    for s in probes:
        for floor in (math.nextafter(s, 0.0), s, math.nextafter(s, 2.0)):
            left, right = (np.array(f) for f in bm.probe_floors(records, s, floor, n, m))
            for lf, rf in ((left, None), (None, right), (left, right)):
                got = floors(0.0, lf, rf, PRUNE[route])
                _same(got, grid.filter_by_floors(everything, lf, rf), f"{name} / {route} floor {floor!r} "
                      f"{'left' if rf is None else 'right' if lf is None else 'both'}")
    # neither: the threshold grid
    for thr in (probes[0], probes[len(probes) // 2], math.nextafter(probes[-1], 2.0)):
        _same(floors(thr, None, None, PRUNE[route]), bm.to_hits(tp.expectation(records, thr)), f"{name} / {route} no floors at {thr!r}")


@pytest.mark.parametrize("name", tp.EVERY)
def test_best_matches_end_to_end(dev, name):
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    _, best = _calls(g, dev)
    records = tp.all_scores(g)
    ban = None
    if not g.raw:
        banned, old_best = _ban_unique_bests(records)
        assert len(banned) >= 3
        records = [r for r in records if (r[1], r[2]) not in banned]
        ban = (np.array([p[0] for p in sorted(banned)]), np.array([p[1] for p in sorted(banned)]))
    gap = bm.row_gap(records)
    probes = tp.probes_of(g)
    for thr in (0.0, probes[len(probes) // 2]):
        want_from = bm.to_hits(tp.expectation(records, thr))
        for margin in (0.0, gap, 2.0):
            for mutual in (False, True):
                got = best(margin, thr, mutual, True, ban)
                _same(got, grid.best_of_hits(want_from, margin, mutual, len(g.left), len(g.right)),
                      f"{name} margin {margin!r} mutual {mutual} at {thr!r}")
                if ban is not None and margin == 0.0 and thr == 0.0 and not mutual:
                    new_best = dict(zip(got.i.tolist(), got.score.tolist()))
                    # (every banned pair was its item's only pair at that score: each of those bests must have moved)
                    assert all(new_best.get(i, -1.0) < old_best[i] for i, _ in banned), "a banned item's best did not move"
                    assert sum(1 for i, _ in banned if i in new_best) >= 3
    _same(best(0.0, 0.0, True, False, ban), grid.best_of_hits(bm.to_hits(records), 0.0, True), f"{name} without pruning")


@pytest.mark.parametrize("name", tp.EVERY)
def test_pruning_is_monotone(dev, name):
    """The floor sweep's bounds are compared against max(threshold, floor) >= the profile's threshold: every counter of
    the floor grid is at most the profile sweep's.  Without pruning a RAW sweep scores every pair."""
    g = tp.grid(name)
    floors, best = _calls(g, dev)
    probes = tp.probes_of(g)
    for thr in (0.0, probes[len(probes) // 2]):
        for mutual in (False, True):
            stats = []
            best(0.0, thr, mutual, True, None, stats)
            profile, floor = stats
            assert len(profile) == len(floor) == 4 and all(f <= p for f, p in zip(floor, profile)), (name, thr, mutual, stats)
    if g.raw:
        stats = []
        floors(0.0, None, None, False, None, stats)
        # (a RAW Jaccard pair of two empty sets is never scored; the probe grids have no empty left row)
        assert stats[3] == g.pairs, (name, stats)


# ------------------------------------------------------------------------------------------------------ small shapes
def _small_strings(rng, n):
    return ["".join(rng.choice("abcd") for _ in range(rng.choice((0, 1, 3, 9, 20)))) for _ in range(n)]


@pytest.mark.parametrize("stride", [64, 128])
@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_small_fuzzy(dev, n, m, stride):
    """Fewer rows than a wave's 8, exactly 8, one more; right sides around one chunk of 64; empty strings on both sides."""
    from napkon_string_matching_amd import grid, tables
    from oracle import native

    rng = random.Random(n * 100 + m)
    left, right = _small_strings(rng, n), _small_strings(rng, m)
    left[0] = right[-1] = ""
    units = lambda rows: native.csr([[ord(c) for c in s] for s in rows])
    records = native.indel_raw(units(left), units(right), 0.0, cap=n * m + 1)
    assert len(records) == n * m
    alpha = tables.Alphabet(left + right)
    lt, rt = (tables.StrTable.from_strings(side, alpha, dev, stride=stride) for side in (left, right))
    assert lt.stride == rt.stride == stride
    _check_small(records, n, m, lambda thr, lf, rf, prune: grid.indel_raw_floor_grid(lt, rt, thr, lf, rf, prune=prune),
                 lambda margin, thr, mutual, prune: grid.indel_raw_best(lt, rt, margin, thr, mutual, prune=prune), f"{n} x {m} @ {stride}")


@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_small_jaccard(dev, n, m):
    from napkon_string_matching_amd import grid, tables
    from oracle import native

    rng = random.Random(n * 1000 + m)
    rows = lambda k, low: [rng.sample(range(8), rng.randint(low, 5)) for _ in range(k)]
    left, right = rows(n, 1), rows(m, 0)
    right[0] = []
    records = native.jaccard_raw(native.csr(left), native.csr(right), 0.0, cap=n * m + 1)
    assert len(records) == n * m

    def padded(side):
        ids = np.full((len(side), 16), -1, dtype=np.int32)
        for r, row in enumerate(side):
            ids[r, : len(row)] = row
        return ids

    lt = tables.SetTable.from_padded(padded(left), "left", dev, width=16)
    rt = tables.SetTable.from_padded(padded(right), "right", dev, width=16)
    _check_small(records, n, m, lambda thr, lf, rf, prune: grid.jaccard_raw_floor_grid(lt, rt, thr, lf, rf, prune=prune),
                 lambda margin, thr, mutual, prune: grid.jaccard_raw_best(lt, rt, margin, thr, mutual, prune=prune), f"{n} x {m}")


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_identical_right_rows_every_pair_ties(dev, n):
    """A right table of identical rows: every left item's best is shared by all of them -- N M best records, which no
    fixed k returns.  Every right item's best is the largest score of the grid, so the mutual best matches are the rows of
    the one left item that reaches it."""
    from napkon_string_matching_amd import grid, tables
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    m = 65
    left = ["abca", "abcd ab", "", "dcba", "ab", "abcabc", "a", "bcd", "abcd"][:n]
    lt, rt = tables.encode_strings(left, ["abcd"] * m, dev)
    got = grid.indel_raw_best(lt, rt, 0.0, 0.0, False)
    assert len(got) == n * m and sorted(zip(got.i.tolist(), got.j.tolist())) == [(i, j) for i in range(n) for j in range(m)]
    assert all(len(set(got.score[got.i == i].tolist())) == 1 for i in range(n))
    top = int(got.i[0])  # (canonical order: the first record holds the largest score; no two of these items share it)
    both = grid.indel_raw_best(lt, rt, 0.0, 0.0, True)
    assert list(zip(both.i.tolist(), both.j.tolist())) == [(top, j) for j in range(m)] and set(both.score.tolist()) == {got.score[0]}
    words = ["a b", "a b c", "c", "a", "b c d", "d", "a d", "b", "a b c d"][:n]
    for plugin in (fuzzy_match, intersection_vs_union):
        assert len(plugin.best(words, ["a b c"] * m, device=dev)) == n * m, plugin.__name__


@pytest.mark.parametrize("n,m", [(0, 5), (5, 0), (0, 0)])
def test_a_side_without_rows(dev, n, m):
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    for plugin in (fuzzy_match, intersection_vs_union):
        for mutual in (False, True):
            assert len(plugin.best(["ab cd"] * n, ["ab ef"] * m, mutual=mutual, device=dev)) == 0


@pytest.mark.parametrize("empty", ["left", "right", "both"])
def test_wrappers_on_a_table_without_rows(dev, empty):
    """The grid-level wrappers themselves with an empty table (the plugins return before they build one): no caller ids, so
    no floors to check or hand over; the entries return without a launch and the hit list is empty."""
    import dataclasses

    from napkon_string_matching_amd import grid, tables

    cut = lambda table, side: dataclasses.replace(table, n=0) if empty in (side, "both") else table
    lt, rt = tables.encode_strings(["ab", "cd", "ef"], ["ab", "xy"], dev)
    lt, rt = cut(lt, "left"), cut(rt, "right")
    floors = lambda table: np.zeros(table.n)
    for stats in (None, []):
        assert len(grid.indel_raw_floor_grid(lt, rt, 0.0, floors(lt), floors(rt), stats=stats)) == 0
        assert len(grid.indel_raw_floor_grid(lt, rt, 0.0, stats=stats)) == 0
        assert stats in (None, [0, 0, 0, 0])
    for mutual in (False, True):
        assert len(grid.indel_raw_best(lt, rt, 0.0, 0.0, mutual)) == 0

    def padded(rows):
        ids = np.full((len(rows), 16), -1, dtype=np.int32)
        for r, row in enumerate(rows):
            ids[r, : len(row)] = row
        return ids

    jl = cut(tables.SetTable.from_padded(padded([[1, 2], [3]]), "left", dev, width=16), "left")
    jr = cut(tables.SetTable.from_padded(padded([[1], [2, 3], [4]]), "right", dev, width=16), "right")
    assert len(grid.jaccard_raw_floor_grid(jl, jr, 0.0, floors(jl), floors(jr))) == 0
    for mutual in (False, True):
        assert len(grid.jaccard_raw_best(jl, jr, 0.0, 0.0, mutual)) == 0


def test_floors_shorter_than_the_caller_ids_are_refused(dev):
    from napkon_string_matching_amd import grid, tables

    lt, rt = tables.encode_strings(["ab", "cd", "ef"], ["ab", "xy"], dev)
    with pytest.raises(ValueError):
        grid.indel_raw_floor_grid(lt, rt, 0.0, left_floor=np.zeros(2))
    with pytest.raises(ValueError):
        grid.indel_raw_floor_grid(lt, rt, 0.0, right_floor=np.zeros(1))
    with pytest.raises(ValueError):
        grid.indel_raw_floor_grid(lt, rt, 0.0, left_floor=np.zeros(3, dtype=np.float32).reshape(3, 1))


# -------------------------------------------------------------------------------------------------- capacity protocol
def _entry_calls(dev):
    """name -> (call(threshold, left_floor ptr, right_floor ptr, hits ptr, capacity, count ptr), probe grid) for the four C
    entries, each on one probe grid."""
    import torch

    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    for name, entry in (("raw_indel_64", "nsm_indel_raw_floor_grid"), ("raw_jaccard_16", "nsm_jaccard_raw_floor_grid"),
                        ("levels_indel_one_word-cat2_lanes", "nsm_indel_levels_floor_grid"),
                        ("levels_jaccard-cat2_lanes", "nsm_jaccard_levels_floor_grid")):
        g = tp.grid(name)
        if g.raw:
            tabs = probe_tables.raw_indel_tables(g, dev) if g.kind == "indel" else probe_tables.raw_jaccard_tables(g, dev)
            middle = (_lib.FLAG_PRUNE,)
        else:
            tabs = probe_tables.levels_indel_tables(g, dev, False) if g.kind == "indel" else \
                probe_tables.levels_jaccard_tables(g, dev, False)
            middle = (g.mode, _lib.FLAG_PRUNE, 0, 0)
        fn = getattr(lib, entry)
        out[entry] = (lambda thr, lf, rf, hits, cap, cnt, fn=fn, tabs=tabs, middle=middle: fn(
            *[t.struct() for t in tabs], thr, lf, rf, *middle, hits, cap, cnt, 0, stream), g)
    return out


def _device_records(buf, n):
    host = buf[:n].cpu().numpy()
    ij = host.view(np.int32).reshape(n, 4)
    return list(zip(host[:, 0].tolist(), ij[:, 2].tolist(), ij[:, 3].tolist()))


def test_capacity_protocol(dev):
    """The threshold grids' protocol: the counter reports the true count at any capacity, what is stored are distinct
    members of the expected list, and records go behind what the counter already holds."""
    import torch

    for entry, (call, g) in _entry_calls(dev).items():
        records = tp.all_scores(g)
        n, m = len(g.left), len(g.right)
        lb, rb = bm.bests(records)
        lf = [math.nextafter(lb.get(i, 0.0), 0.0) for i in range(n)]
        rf = [rb.get(j, 0.0) * 0.5 for j in range(m)]
        want = bm.floors_plain(records, lf, rf)
        assert len(want) > 8, entry
        lfd, rfd = (torch.tensor(f, dtype=torch.float64, device=dev) for f in (lf, rf))
        for cap in (0, 1, len(want) // 2, len(want)):
            buf = torch.full((max(cap, 1) + 4, 2), -7.0, dtype=torch.float64, device=dev)
            cnt = torch.zeros(1, dtype=torch.int64, device=dev)
            assert call(0.0, lfd.data_ptr(), rfd.data_ptr(), buf.data_ptr() if cap else 0, cap, cnt.data_ptr()) == 0, entry
            torch.cuda.synchronize(dev)
            assert int(cnt.item()) == len(want), (entry, cap)
            stored = _device_records(buf, cap) if cap else []
            assert len(set((i, j) for _, i, j in stored)) == cap and set(stored) <= set(want), (entry, cap)
            assert (buf[cap:] == -7.0).all(), f"{entry}: wrote beyond capacity {cap}"
        # three records already counted: the new ones follow them
        cap = len(want) + 3
        buf = torch.full((cap + 4, 2), -7.0, dtype=torch.float64, device=dev)
        cnt = torch.full((1,), 3, dtype=torch.int64, device=dev)
        assert call(0.0, lfd.data_ptr(), rfd.data_ptr(), buf.data_ptr(), cap, cnt.data_ptr()) == 0, entry
        torch.cuda.synchronize(dev)
        assert int(cnt.item()) == cap and (buf[:3] == -7.0).all() and (buf[cap:] == -7.0).all(), entry
        assert sorted(_device_records(buf, cap)[3:], key=lambda r: (-r[0], r[1], r[2])) == want, entry


# ------------------------------------------------------------------------------------------------------ public surface
def test_fuzzy_match_best_with_a_wide_item(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match

    rng = random.Random(21)
    text = lambda k: " ".join("".join(rng.choice("abcde") for _ in range(rng.randint(2, 6))) for _ in range(k))
    left, right = [text(rng.randint(1, 4)) for _ in range(12)], [text(rng.randint(1, 4)) for _ in range(14)]
    left[3] = "x" * 513  # beyond the fast kernels: the general route
    right[5], right[9] = left[2], left[2]  # a tie at the top
    for thr in (0.0, 0.4):
        everything = fuzzy_match.raw_grid(left, right, thr, device=dev)
        for margin in (0.0, 0.1, 2.0):
            for mutual in (False, True):
                got = fuzzy_match.best(left, right, margin, thr, mutual, device=dev)
                _same(got, grid.best_of_hits(everything, margin, mutual, len(left), len(right)), f"margin {margin} mutual {mutual} at {thr}")
    exact = fuzzy_match.best(left, right, device=dev)
    assert {(2, 5), (2, 9)} <= set(zip(exact.i.tolist(), exact.j.tolist())) and 3 in exact.i


def test_intersection_vs_union_best_with_a_wide_item(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import intersection_vs_union

    rng = random.Random(22)
    words = [f"w{q}" for q in range(10)]
    row = lambda: rng.sample(words, rng.randint(1, 4))
    left, right = [row() for _ in range(12)], [row() for _ in range(14)]
    many = [f"x{q}" for q in range(70)]
    left[4], right[6] = many[:65], many[3:68] + words[:2]  # 65 distinct tokens and more: the general route
    for thr in (0.0, 0.3):
        everything = intersection_vs_union.raw_grid(left, right, thr, device=dev)
        for margin in (0.0, 0.1, 2.0):
            for mutual in (False, True):
                got = intersection_vs_union.best(left, right, margin, thr, mutual, device=dev)
                _same(got, grid.best_of_hits(everything, margin, mutual, len(left), len(right)), f"margin {margin} mutual {mutual} at {thr}")
    exact = intersection_vs_union.best(left, right, mutual=True, device=dev)
    assert (4, 6) in set(zip(exact.i.tolist(), exact.j.tolist()))


def test_empty_vs_empty_jaccard_raises(dev):
    from napkon_string_matching_amd.compare.score_functions import intersection_vs_union

    with pytest.raises(ZeroDivisionError):
        intersection_vs_union.best(["a b", ""], ["a", ""], device=dev)
    with pytest.raises(ValueError):  # the margin is checked first
        intersection_vs_union.best(["a b", ""], ["a", ""], margin=-1.0, device=dev)


def _frame(rows):
    return pd.DataFrame(rows, columns=["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"])


def _cohort(seed, n, words, zero_at):
    rng = random.Random(seed)
    rows = []
    for k in range(n):
        toks = [rng.choice(words) for _ in range(rng.randint(1, 6))]
        term = [" ".join(toks[q:q + 2]) for q in range(0, len(toks), 2)]
        cat = [f"c{k % 3}"]
        if k == zero_at:  # zero levels; a category of its own, so that it only meets the other side's zero-level item
            term, cat = [], ["none"]
        rows.append([f"{seed}-{k}", f"v{k}", "s", cat, term, toks, "p"])
    return _frame(rows)


def _rows(comparable):
    frame = comparable.dataframe()
    return [(s, a, b) for s, a, b in zip(frame["MatchScore"].tolist(), frame["HapIdentifier"].tolist(), frame["PopIdentifier"].tolist())]


@pytest.mark.parametrize("score_func", ["intersection_vs_union", "fuzzy_match"])
def test_compare_best_margin(score_func, tmp_path):
    """``compare(best_margin=)`` is ``best_of_hits`` of the rows of the plain ``compare()``: after categories and blacklist,
    the zero-level pair (score 0) a row like any other; the same with the bests taken at a cache threshold below
    ``score_threshold``."""
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    words = [f"word{q}" for q in range(12)]
    left, right = Questionnaire(_cohort(1, 30, words, 4)), Questionnaire(_cohort(2, 35, words, 7))
    kw = dict(score_func=score_func, compare_column="Term", left_name="hap", right_name="pop", filter_categories=True)
    plain = left.compare(right, None, None, score_threshold=0.0, cached=False, **kw)
    top = plain.dataframe().iloc[0]
    blacklist = {"b": {"hap": [top["HapIdentifier"]], "pop": [top["PopIdentifier"]]}}
    for thr in (0.0, 0.3):
        rows = _rows(left.compare(right, None, blacklist, score_threshold=thr, cached=False, **kw))
        assert (top["HapIdentifier"], top["PopIdentifier"]) not in {(a, b) for _, a, b in rows}
        for margin, mutual in ((0.0, False), (0.0, True), (0.05, False), (0.05, True), (2.0, True)):
            want = bm.best_plain(rows, margin, mutual)
            got = _rows(left.compare(right, None, blacklist, score_threshold=thr, cached=False, best_margin=margin,
                                     mutual_best=mutual, **kw))
            assert sorted(got) == sorted(want) and len(want) > 0, (score_func, thr, margin, mutual)
            if margin == 0.0 and thr == 0.0:
                # (the zero-level pair scores 0 and is the only row of both its items: a best match from either side)
                assert len(want) < len(rows) and (0.0, "1-4", "2-7") in want
    # the bests taken at cache_threshold 0.1, the rows filtered at 0.3 afterwards
    rows = _rows(left.compare(right, None, blacklist, score_threshold=0.3, cached=False, **kw))
    for mutual in (False, True):
        got = _rows(left.compare(right, None, blacklist, score_threshold=0.3, cache_threshold=0.1, cache_dir=tmp_path,
                                 best_margin=0.0, mutual_best=mutual, **kw))
        assert sorted(got) == sorted(bm.best_plain(rows, 0.0, mutual)) and len(got) > 0
        again = _rows(left.compare(right, None, blacklist, score_threshold=0.3, cache_threshold=0.1, cache_dir=tmp_path,
                                   best_margin=0.0, mutual_best=mutual, **kw))
        assert sorted(again) == sorted(got)  # (read back from its own cache file)
    assert len(list(tmp_path.iterdir())) == 2


def test_matcher_config_passes_best_margin(dev):
    """``matching.best_margin`` / ``matching.mutual_best`` of a ``Matcher`` config reach ``compare`` the way ``top_k`` does."""
    from napkon_string_matching_amd.matcher import Matcher
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    words = [f"word{q}" for q in range(12)]
    cohorts = {"hap": Questionnaire(_cohort(1, 20, words, -1)), "pop": Questionnaire(_cohort(2, 25, words, -1))}
    matching = dict(score_func="fuzzy_match", compare_column="Term", score_threshold=0.2, cached=False)
    want = bm.best_plain(_rows(cohorts["hap"].compare(cohorts["pop"], None, None, left_name="hap", right_name="pop", **matching)),
                         0.0, True)
    matcher = Matcher(None, {"matching": dict(matching, best_margin=0.0, mutual_best=True)}, questionnaires=cohorts)
    matcher.match_questionnaires()
    ((_, result),) = matcher.results.items()
    assert sorted(_rows(result)) == sorted(want) and len(want) > 0
