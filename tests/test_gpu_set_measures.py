"""GPU parity of the token-set measures beside Jaccard -- intersection_vs_mean (Dice), intersection_vs_smaller (overlap),
intersection_vs_left (containment) -- from the nsm_set_* entries up to ``ComparableData.compare`` and ``Matcher``.

The yardstick is the pure-Python definition in tests/support/set_measures.py (for levels and whole frames: the oracle's
``compare_terms`` / ``gen_comparable`` with that definition registered as score_func).  Records are compared as canonical
``(score, i, j)`` tuples, the scores as doubles bit for bit (``==`` on Python floats: every score here is finite).  The
inputs are checked in tests/test_cpu_set_measures.py: every threshold has a pair exactly on it and one below it.
The pruning bounds of the measures at exact thresholds and floors, at every width: tests/test_gpu_measure_probes.py.
"""
import math

import numpy as np
import pandas as pd
import pytest

from support import set_measures as sm

pytestmark = pytest.mark.gpu

RAW_THRESHOLDS = sm.thresholds_with_next(sm.RAW_THRESHOLDS) + (0.0,)
LEVELS_THRESHOLDS = sm.thresholds_with_next(sm.LEVELS_THRESHOLDS)


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _plugin(measure):
    from napkon_string_matching_amd.compare import score_functions as sf

    return getattr(sf, sm.NAMES[measure])


def _hits(records):
    from napkon_string_matching_amd import grid

    return grid.Hits(np.array([r[0] for r in records], dtype=np.float64), np.array([r[1] for r in records], dtype=np.int32),
                     np.array([r[2] for r in records], dtype=np.int32))


_RAW = {}


def _raw_case(dev, measure, width):
    """(left rows, right rows, left table, right table, every pair's record) of a RAW grid, built once per module."""
    from napkon_string_matching_amd import tables

    key = (measure, width)
    if key not in _RAW:
        left, right = sm.raw_grid(measure, width)
        vocab = tables.Vocabulary()
        lt = tables.SetTable.from_rows(left, "left", dev, vocab, width=width)
        rt = tables.SetTable.from_rows(right, "right", dev, vocab, width=width)
        assert lt.width == rt.width == width
        _RAW[key] = (left, right, lt, rt, sm.raw_hits(measure, left, right, float("-inf")))
    return _RAW[key]


def _at(records, threshold):
    return [r for r in records if r[0] >= threshold]


# =============================================================================================== 1, 2: RAW threshold grids
@pytest.mark.parametrize("width", [16, 32, 64])
@pytest.mark.parametrize("measure", sm.MEASURES)
def test_raw_grid_records(dev, measure, width):
    from napkon_string_matching_amd import grid

    left, right, lt, rt, full = _raw_case(dev, measure, width)
    for t in RAW_THRESHOLDS:
        want = _at(full, t)
        assert (len(want) > 0) == (t <= 1.0) and (t == 0.0 or len(want) < len(full))  # (nothing scores above 1.0)
        for prune in (True, False):
            got = grid.jaccard_raw_grid(lt, rt, t, prune=prune, measure=measure)
            assert got.as_tuples() == want, (measure, width, t, prune)
    # the pair on the threshold leaves with nextafter(t)
    for t in sm.RAW_THRESHOLDS:
        assert len(_at(full, t)) > len(_at(full, math.nextafter(t, 2.0)))
    # the plug-in encodes the same lists itself
    assert _plugin(measure).raw_grid(left, right, 0.5, device=dev).as_tuples() == _at(full, 0.5)
    assert _plugin(measure).raw_grid(left, right, 0.5, device=dev, prune=False).as_tuples() == _at(full, 0.5)


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_plugin_call_and_gewicht(dev, measure):
    plugin = _plugin(measure)
    left, right = ["Gewicht"], ["Gewicht", "Patient", "Aufnahme", "kg"]
    assert plugin(left, right) == {"left": 1.0, "smaller": 1.0, "mean": 0.4}[measure]
    assert plugin(right, left) == {"left": 0.25, "smaller": 1.0, "mean": 0.4}[measure]
    assert plugin("a b c", "b c d e f") == sm.DEFINITIONS[measure]("a b c", "b c d e f")


# ================================================================================================ 3: the other RAW queries
@pytest.mark.parametrize("measure", sm.MEASURES)
def test_raw_top_k(dev, measure):
    from napkon_string_matching_amd import grid

    left, right, lt, rt, full = _raw_case(dev, measure, 16)
    groups = [j % 7 for j in range(len(right))]
    for t in (0.0, 0.5):
        for k in (1, 3):
            for g in (None, groups):
                want = grid.select_top_k(_hits(_at(full, t)), k, None if g is None else np.array(g, dtype=np.int32)).as_tuples()
                assert len(want) > 0
                for prune in (True, False):
                    got = _plugin(measure).top_k(left, right, k, t, device=dev, prune=prune, groups=g)
                    assert got.as_tuples() == want, (measure, t, k, g is not None, prune)
                got = grid.jaccard_raw_top_k(lt, rt, k, t, groups=None if g is None else np.array(g, dtype=np.int32),
                                             measure=measure)
                assert got.as_tuples() == want


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_raw_profile_and_best(dev, measure):
    from napkon_string_matching_amd import grid

    left, right, lt, rt, full = _raw_case(dev, measure, 16)
    ladder = [0.0, 0.25, 0.5, 2 / 3, 1.0]
    want = grid.profile_of_hits(_hits(_at(full, ladder[0])), ladder, len(left), len(right))
    for prune in (True, False):
        got = _plugin(measure).profile(left, right, ladder, device=dev, prune=prune)
        assert got.pairs.tolist() == want.pairs.tolist() and got.pairs[0] > got.pairs[-1] > 0
        assert got.left_best.tolist() == want.left_best.tolist() and got.right_best.tolist() == want.right_best.tolist()
    for mutual in (True, False):
        want = grid.best_of_hits(_hits(_at(full, 0.0)), 0.0, mutual, len(left), len(right)).as_tuples()
        got = _plugin(measure).best(left, right, margin=0.0, threshold=0.0, mutual=mutual, device=dev)
        assert got.as_tuples() == want and len(want) >= (1 if mutual else len(left)), (measure, mutual)


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_raw_pairs(dev, measure):
    """Listed pairs at the grid.*_pairs level: duplicates, an id no table holds, and zero-denominator pairs (-1.0)."""
    from napkon_string_matching_amd import grid, tables

    left, right = sm.raw_grid(measure, 16)
    left, right = left + [[]], [r for r in right if r] + [[]]  # an empty set on both sides: the tables may hold them
    vocab = tables.Vocabulary()
    lt = tables.SetTable.from_rows(left, "left", dev, vocab, width=16)
    rt = tables.SetTable.from_rows(right, "right", dev, vocab, width=16)
    n_l, n_r = len(left), len(right)
    pi = [k % n_l for k in range(0, 5 * n_l, 3)] + [n_l - 1, n_l - 1, 0, 5, 5, n_l + 3, 2]
    pj = [(7 * k + 1) % n_r for k in range(len(pi) - 7)] + [n_r - 1, 4, n_r - 1, 9, 9, 1, n_r]
    want = []
    for a, b in zip(pi, pj):
        if a >= n_l or b >= n_r or sm.DIVIDES_BY_ZERO[measure](len(set(left[a])), len(set(right[b]))):
            want.append(-1.0)
        else:
            want.append(sm.DEFINITIONS[measure](left[a], right[b]))
    assert want.count(-1.0) >= 3 and len(set(zip(pi, pj))) < len(pi)
    got = grid.jaccard_raw_pairs(lt, rt, np.array(pi), np.array(pj), measure=measure)
    assert got.tolist() == want
    # the plug-in: positions in the lists, ZeroDivisionError for a listed pair that divides by zero (the CPU tests), else
    # the definition
    ok = [(a, b) for a, b, w in zip(pi, pj, want) if w != -1.0]
    assert _plugin(measure).pairs(left, right, ok, device=dev).tolist() == [w for w in want if w != -1.0]


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_raw_assign_groups_forest(dev, measure):
    from napkon_string_matching_amd import grid

    left, right, lt, rt, full = _raw_case(dev, measure, 16)
    n_l, n_r = len(left), len(right)
    plugin = _plugin(measure)
    for t in (2 / 3, 1.0):
        hits = _hits(_at(full, t))
        assert plugin.assign(left, right, t, device=dev).as_tuples() == grid.assign_of_hits(hits).as_tuples()
        groups = plugin.groups(left, right, t, device=dev)
        want_label = grid.groups_of_hits([(hits, 0, n_l)], n_l + n_r)
        assert groups.label.tolist() == want_label.tolist() and len(groups.members()) > 0
        forest = plugin.forest(left, right, t, device=dev)
        want_forest = grid.forest_of_hits([(hits, 0, n_l)], n_l + n_r, t)
        assert forest.as_tuples() == want_forest.as_tuples() and len(forest) > 0
        assert forest.cut(t).label.tolist() == want_label.tolist()
    # the self-join
    items = left[:20]
    self_hits = _hits(sm.raw_hits(measure, items, items, 1.0))
    want = grid.groups_of_hits([(self_hits, 0, 0)], len(items))
    assert plugin.groups(items, items, 1.0, device=dev, same=True).label.tolist() == want.tolist()
    assert plugin.cluster_tree(items, 1.0, device=dev).cut(1.0).label.tolist() == want.tolist()
    assert [c.tolist() for c in plugin.clusters(items, 1.0, device=dev)] == \
        [m[0].tolist() for m in grid.MatchGroups(want, (0,), (len(items),)).members(2)]


# ============================================================================================ 4: NSM_MEASURE_UNION differential
def test_union_through_the_new_entries(dev, monkeypatch):
    """NSM_MEASURE_UNION through nsm_set_* gives the nsm_jaccard_* entry's records, record for record, on the same tables."""
    from napkon_string_matching_amd import _lib, grid, tables

    left, right, lt, rt, _ = _raw_case(dev, "mean", 16)  # (a grid with an empty right row: fine for Jaccard too)
    items_l, items_r = sm.levels_grid("mean")
    vocab = tables.Vocabulary()
    cl, cr = sm.levels_categories(len(items_l), len(items_r))
    ll = tables.SetTable.from_levels(items_l, "left", dev, vocab, width=16, categories=cl, category_mode=2, partition=False, index=False)
    lr = tables.SetTable.from_levels(items_r, "right", dev, vocab, width=16, categories=cr, category_mode=2, partition=False,
                                     index=False)
    pi, pj = np.arange(len(left)).repeat(3), (np.arange(3 * len(left)) * 5) % len(right)
    ladder = [0.0, 0.3, 0.5, 1.0]

    def run():
        return {
            "top_k": grid.jaccard_raw_top_k(lt, rt, 3, 0.2).as_tuples(),
            "grouped": grid.jaccard_raw_top_k(lt, rt, 2, 0.0, groups=np.arange(len(right), dtype=np.int32) % 5).as_tuples(),
            "profile": [a.tolist() for a in (lambda p: (p.pairs, p.left_best, p.right_best))(grid.jaccard_raw_profile(lt, rt, ladder))],
            "floor": grid.jaccard_raw_floor_grid(lt, rt, 0.4).as_tuples(),
            "pairs": grid.jaccard_raw_pairs(lt, rt, pi, pj).tolist(),
            "levels floor": grid.jaccard_levels_floor_grid(ll, lr, 0.3, category_mode=2).as_tuples(),
            "levels top_k": grid.jaccard_levels_top_k(ll, lr, 2, 0.1, category_mode=2).as_tuples(),
            "levels profile": grid.jaccard_levels_profile(ll, lr, ladder, category_mode=2).pairs.tolist(),
            "levels pairs": grid.jaccard_levels_pairs(ll, lr, np.arange(len(items_l)), np.arange(len(items_l)) % len(items_r)).tolist(),
        }

    want = run()
    used = []

    def through_set(entry, measure):
        assert measure == "union"
        used.append(entry.replace("nsm_jaccard_", "nsm_set_"))
        return used[-1], (_lib.MEASURE_UNION,)

    monkeypatch.setattr(grid, "_set_entry", through_set)
    got = run()
    assert set(used) | {"nsm_set_raw_top_k_grouped"} == set(_lib.MEASURE_EXPORTS)
    assert got == want and all(len(v) > 0 for v in want.values())


# ======================================================================================================== 5: levels
_LEVELS = {}


def _levels_case(dev, measure, mode):
    from napkon_string_matching_amd import tables

    key = (measure, mode)
    if key not in _LEVELS:
        left, right = sm.levels_grid(measure)
        cl, cr = sm.levels_categories(len(left), len(right)) if mode else (None, None)
        vocab = tables.Vocabulary()
        lt = tables.SetTable.from_levels(left, "left", dev, vocab, width=16, categories=cl, category_mode=mode, partition=False,
                                         index=False)
        rt = tables.SetTable.from_levels(right, "right", dev, vocab, width=16, categories=cr, category_mode=mode, partition=False,
                                         index=False)
        keep = (lambda i, j: True) if not mode else (lambda i, j: sm.category_match(int(cl[i]), int(cr[j]), mode))
        _LEVELS[key] = (left, right, lt, rt, keep)
    return _LEVELS[key]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("measure", sm.MEASURES)
def test_levels_queries(dev, measure, mode, monkeypatch):
    from napkon_string_matching_amd import grid
    from oracle import score_functions as osf

    left, right, lt, rt, keep = _levels_case(dev, measure, mode)
    with sm.registered(monkeypatch):
        f = osf.get(sm.NAMES[measure])  # the registered callable, as the oracle's compare_terms gets it
        full = sm.levels_hits(measure, left, right, float("-inf"), keep, f)
    assert 0 < len(full) and (mode == 0) == (len(full) == len(left) * len(right))
    best_of_row = {}
    for s, i, j in full:
        best_of_row.setdefault(i, (i, j))
    banned = set(list(best_of_row.values())[::2]) | {(1, j) for j in range(len(right))}
    as_arrays = lambda ban: None if not ban else (np.array([p[0] for p in sorted(ban)]), np.array([p[1] for p in sorted(ban)]))
    for ban in (set(), banned):
        allowed = [h for h in full if (h[1], h[2]) not in ban]
        for t in LEVELS_THRESHOLDS:
            want = _at(allowed, t)
            assert 0 < len(want) < len(allowed)
            for prune in (True, False):
                got = grid.jaccard_levels_grid(lt, rt, t, category_mode=mode, prune=prune, measure=measure, banned=as_arrays(ban))
                assert got.as_tuples() == want, (measure, mode, t, prune, len(ban))
        for k in (1, 2):
            want = grid.select_top_k(_hits(_at(allowed, 0.5)), k).as_tuples()
            for prune in (True, False):
                got = grid.jaccard_levels_top_k(lt, rt, k, 0.5, category_mode=mode, prune=prune, banned=as_arrays(ban), measure=measure)
                assert got.as_tuples() == want, (measure, mode, k, prune, len(ban))
        ladder = [0.25, 0.5, 0.75, math.nextafter(0.75, 2.0)]
        want = grid.profile_of_hits(_hits(_at(allowed, ladder[0])), ladder, len(left), len(right))
        got = grid.jaccard_levels_profile(lt, rt, ladder, category_mode=mode, banned=as_arrays(ban), measure=measure)
        assert got.pairs.tolist() == want.pairs.tolist() and got.pairs[2] > got.pairs[3]
        assert got.left_best.tolist() == want.left_best.tolist() and got.right_best.tolist() == want.right_best.tolist()
        if ban:
            assert got.left_best[1] == -1.0  # every pair of left item 1 is banned
        want = grid.best_of_hits(_hits(_at(allowed, 0.25)), 0.0, True, len(left), len(right)).as_tuples()
        got = grid.jaccard_levels_best(lt, rt, 0.0, 0.25, mutual=True, category_mode=mode, banned=as_arrays(ban), measure=measure)
        assert got.as_tuples() == want and len(want) > 0


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_levels_pairs(dev, measure, monkeypatch):
    """No category predicate, no blacklist: the listed pairs' compare_terms; -1.0 where a visited step divides by zero."""
    from napkon_string_matching_amd import grid, tables
    from oracle import compare as oc
    from oracle import score_functions as osf

    left, right = sm.levels_grid(measure)
    left, right = left + [sm.nested(0, 0, 2), sm.nested(0)], right + [sm.nested(0, 0, 2), sm.nested(0)]
    vocab = tables.Vocabulary()
    lt = tables.SetTable.from_levels(left, "left", dev, vocab, width=16, partition=False, index=False)
    rt = tables.SetTable.from_levels(right, "right", dev, vocab, width=16, partition=False, index=False)
    pi = np.array([i for i in range(len(left)) for _ in range(len(right))] + [0, 0, len(left)])
    pj = np.array([j for _ in range(len(left)) for j in range(len(right))] + [3, 3, 0])
    want = []
    with sm.registered(monkeypatch):
        f = osf.get(sm.NAMES[measure])
        for a, b in zip(pi.tolist(), pj.tolist()):
            try:
                want.append(oc.compare_terms(left[a], right[b], f) if a < len(left) else -1.0)
            except ZeroDivisionError:
                want.append(-1.0)
    assert want.count(-1.0) > 2 and sum(w >= 0 for w in want) > len(want) // 2
    assert grid.jaccard_levels_pairs(lt, rt, pi, pj, measure=measure).tolist() == want


# ================================================================================================= 6: the public surface
WORDS = [f"word{q}" for q in range(10)]
COLUMNS = ["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"]


def _cohort(seed, n, n_cats=3):
    import random

    rng = random.Random(seed)
    rows = []
    for k in range(n):
        toks = [rng.choice(WORDS) for _ in range(rng.randint(1, 6))]
        term = [" ".join(toks[q:q + 2]) for q in range(0, len(toks), 2)]
        rows.append([f"{seed}-{k}", f"v{k}", "s", [f"c{k % n_cats}"] if k % 7 else [], term, toks, "p"])
    return pd.DataFrame(rows, columns=COLUMNS)


def _with_term(frame: pd.DataFrame, row: int, term) -> pd.DataFrame:
    terms = list(frame["Term"])
    terms[row] = term
    return frame.assign(Term=pd.Series(terms, dtype=object, index=frame.index))


def _same_frame(got: pd.DataFrame, want: pd.DataFrame):
    assert list(got.index) == list(want.index) and list(got.columns) == list(want.columns)
    assert list(got["MatchScore"]) == list(want["MatchScore"])  # bit-exact doubles
    assert got.drop(columns=["MatchScore"]).to_dict(orient="records") == want.drop(columns=["MatchScore"]).to_dict(orient="records")


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_compare_against_the_oracle(dev, measure, monkeypatch):
    from napkon_string_matching_amd.types.questionnaire import Questionnaire
    from oracle import compare as oc

    name = sm.NAMES[measure]
    left, right = _cohort(1, 26), _cohort(2, 31)
    ql, qr = Questionnaire(left), Questionnaire(right)
    blacklist = {"b": {"hap": [left["Identifier"][3], left["Identifier"][8]], "pop": list(right["Identifier"][:12])}}
    with sm.registered(monkeypatch):
        for bl, filt in ((blacklist, False), ({}, True), (blacklist, True)):
            kw = dict(score_func=name, compare_column="Term", left_name="hap", right_name="pop", filter_categories=filt,
                      score_threshold=0.3)
            want = oc.gen_comparable(left, right, {}, bl, **kw)
            assert 3 < len(want) < len(left) * len(right)
            _same_frame(ql.gen_comparable(qr, {}, bl, **kw).dataframe(), want)
            # compare(): the same rows ordered by score (ties: the reference leaves them unspecified)
            kw.pop("score_threshold")
            comp = ql.compare(qr, None, bl, score_threshold=0.3, cached=False, **kw).dataframe()
            ordered = oc.compare(left, right, {}, bl, score_threshold=0.3, **kw)
            assert list(comp["MatchScore"]) == list(ordered["MatchScore"]) and list(comp.columns) == list(ordered.columns)
            assert sorted(comp.index) == sorted(ordered.index)
            rows = sorted(zip((-ordered["MatchScore"]).tolist(), ordered.index.tolist()))
            # top_k=2: per left item the first two rows (score descending, label ascending)
            seen, cut = {}, []
            for neg, lab in rows:
                i = lab // len(right)
                if seen.setdefault(i, 0) < 2:
                    seen[i] += 1
                    cut.append((neg, lab))
            top = ql.compare(qr, None, bl, score_threshold=0.3, cached=False, top_k=2, **kw).dataframe()
            assert sorted(zip((-top["MatchScore"]).tolist(), top.index.tolist())) == cut and len(cut) < len(rows)
            # best_margin=0, mutual: rows that are the best of their left and of their right item
            best_l, best_r = {}, {}
            for neg, lab in rows:
                best_l[lab // len(right)] = min(best_l.get(lab // len(right), 0.0), neg)
                best_r[lab % len(right)] = min(best_r.get(lab % len(right), 0.0), neg)
            mutual = [(neg, lab) for neg, lab in rows if neg == best_l[lab // len(right)] == best_r[lab % len(right)]]
            best = ql.compare(qr, None, bl, score_threshold=0.3, cached=False, best_margin=0.0, mutual_best=True, **kw).dataframe()
            assert sorted(zip((-best["MatchScore"]).tolist(), best.index.tolist())) == mutual and 0 < len(mutual) < len(rows)
            # one_to_one: greedy over the ordered rows
            taken_l, taken_r, greedy = set(), set(), []
            for neg, lab in rows:
                if lab // len(right) not in taken_l and lab % len(right) not in taken_r:
                    taken_l.add(lab // len(right)), taken_r.add(lab % len(right)), greedy.append((neg, lab))
            one = ql.compare(qr, None, bl, score_threshold=0.3, cached=False, one_to_one=True, **kw).dataframe()
            assert sorted(zip((-one["MatchScore"]).tolist(), one.index.tolist())) == greedy
            # compare_profile: the length of the frame at every threshold
            ladder = [0.3, 0.5, 0.75, 1.0]
            prof = ql.compare_profile(qr, ladder, None, bl, **kw)
            assert prof.pairs.tolist() == [int((ordered["MatchScore"] >= t).sum()) for t in ladder]
        # score_pairs: these pairs, whatever blacklist and categories say
        listed = [(left["Identifier"][i], right["Identifier"][(3 * i + 1) % len(right)]) for i in range(len(left))]
        listed += [listed[0], (left["Identifier"][3], right["Identifier"][0])]
        got = ql.score_pairs(qr, listed, compare_column="Term", score_func=name, left_name="hap", right_name="pop")
        pos_l = {v: k for k, v in enumerate(left["Identifier"])}
        pos_r = {v: k for k, v in enumerate(right["Identifier"])}
        f = sm.DEFINITIONS[measure]
        want = [oc.compare_terms(oc.gen_comp_value(left["Term"][pos_l[a]]), oc.gen_comp_value(right["Term"][pos_r[b]]), f)
                for a, b in listed]
        assert got.dataframe()["MatchScore"].tolist() == want


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_compare_raises_what_the_oracle_raises(dev, measure, monkeypatch):
    """The exception is that of the FIRST offending pair in pair order: a step that divides by zero (ZeroDivisionError) or
    a level-less item against one with levels (IndexError), whichever pair comes first."""
    from napkon_string_matching_amd.types.questionnaire import Questionnaire
    from oracle import compare as oc

    name = sm.NAMES[measure]
    kw = dict(score_func=name, compare_column="Term", left_name="hap", right_name="pop", score_threshold=0.2)
    hollow = ["word1 word2", "", ""]  # levels [], [], [word1, word2]: step 1 meets an empty set
    seen = set()
    with sm.registered(monkeypatch):
        for side in ("left", "right", "both"):
            for level_less_first in (False, True):
                left, right = _cohort(3, 9), _cohort(4, 11)
                if side in ("left", "both"):
                    left = _with_term(left, 4, hollow)
                if side in ("right", "both"):
                    right = _with_term(right, 6, hollow)
                left = _with_term(left, 2 if level_less_first else 7, [])
                try:
                    oc.gen_comparable(left, right, {}, {}, **kw)
                    want = None
                except (ZeroDivisionError, IndexError) as err:
                    want = type(err)
                seen.add(want)
                if want is None:  # (containment does not mind an empty right set)
                    got = Questionnaire(left).gen_comparable(Questionnaire(right), {}, {}, **kw).dataframe()
                    _same_frame(got, oc.gen_comparable(left, right, {}, {}, **kw))
                else:
                    with pytest.raises(want):
                        Questionnaire(left).gen_comparable(Questionnaire(right), {}, {}, **kw)
    assert {ZeroDivisionError, IndexError} <= seen


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_compare_refuses_what_only_the_general_kernels_take(dev, measure):
    """Items beyond 64 tokens and levels that are not suffix-nested are NotImplementedError with a new measure (the general
    kernels score Jaccard alone), in ``compare``, ``compare_terms`` and ``score_pairs``; Jaccard still takes them."""
    from napkon_string_matching_amd.compare import score_functions as sf
    from napkon_string_matching_amd.types.comparable_data import ComparableData
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    name = sm.NAMES[measure]
    kw = dict(compare_column="Term", left_name="hap", right_name="pop", score_threshold=0.2)
    wide = " ".join(f"tok{q}" for q in range(70))
    left, right = _cohort(5, 8), _with_term(_cohort(6, 9), 4, ["word1 word2", wide])
    with pytest.raises(NotImplementedError) as err:
        Questionnaire(left).gen_comparable(Questionnaire(right), {}, {}, score_func=name, **kw)
    assert measure in str(err.value) and name in str(err.value)
    assert len(Questionnaire(left).gen_comparable(Questionnaire(right), {}, {}, score_func="intersection_vs_union", **kw).dataframe()) > 0
    with pytest.raises(NotImplementedError):
        Questionnaire(left).score_pairs(Questionnaire(right), [(left["Identifier"][0], right["Identifier"][4])], score_func=name,
                                        compare_column="Term", left_name="hap", right_name="pop")
    irregular = [["a", "b"], ["c"]]  # level 1 does not contain level 0
    with pytest.raises(NotImplementedError) as err:
        ComparableData.compare_terms(irregular, [["a"], ["a", "c"]], getattr(sf, name))
    assert "nested" in str(err.value)
    assert ComparableData.compare_terms(irregular, [["a"], ["a", "c"]], sf.intersection_vs_union) == 0.5 * 0.5 + 0.25 * 0.5


def test_matcher_gecco_with_intersection_vs_left(dev):
    """The motivating example: a short GECCO definition against long questionnaire items.  Contained in the item it scores
    as a full match under intersection_vs_left; Jaccard leaves it far below the threshold."""
    from napkon_string_matching_amd.matcher import Matcher
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    frame = lambda rows: pd.DataFrame([[ident, f"v{k}", "s", [], [term], term.split(), "p"] for k, (ident, term) in enumerate(rows)],
                                      columns=COLUMNS)
    gecco = Questionnaire(frame([("g-weight", "Gewicht"), ("g-height", "Groesse"), ("g-age", "Alter Jahre")]))
    hap = Questionnaire(frame([("h-1", "Gewicht Patient Aufnahme kg"), ("h-2", "Groesse Patient cm"), ("h-3", "Blutdruck systolisch"),
                               ("h-4", "Alter Patient")]))
    matching = dict(compare_column="Term", score_threshold=0.5, cached=False)
    pairs = {}
    for func in ("intersection_vs_left", "intersection_vs_union"):
        matcher = Matcher(None, {"matching": dict(matching, score_func=func)}, questionnaires={"hap": hap}, gecco=gecco)
        matcher.match_gecco_with_questionnaires()
        ((key, result),) = matcher.results.items()
        assert key == "gecco vs hap"
        df = result.dataframe()
        pairs[func] = {(a, b): s for a, b, s in zip(df["GeccoIdentifier"], df["HapIdentifier"], df["MatchScore"])}
    # one level each: the score is 2^-1 * m(A, B)
    assert pairs["intersection_vs_left"] == {("g-weight", "h-1"): 0.5, ("g-height", "h-2"): 0.5}
    assert pairs["intersection_vs_union"] == {}
