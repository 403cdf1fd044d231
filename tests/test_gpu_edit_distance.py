"""GPU parity of the Levenshtein score functions -- levenshtein_match (normalised Levenshtein similarity) and
levenshtein_within (best approximate occurrence of left inside right) -- from the nsm_edit_* entries up to
``ComparableData.compare`` and ``Matcher``.

The yardstick is the two-row DP and the pure-Python definitions in tests/support/edit_distance.py (for levels and whole
frames: the oracle's ``compare_terms`` / ``gen_comparable`` with that definition registered as score_func).  Records are
compared as canonical ``(score, i, j)`` tuples, the scores as doubles bit for bit (``==`` on Python floats: every score
here is finite).  The inputs are checked in tests/test_cpu_edit_distance.py: every threshold has a pair exactly on it and
one below it.
"""
import math

import numpy as np
import pandas as pd
import pytest

from support import edit_distance as ed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _plugin(metric):
    from napkon_string_matching_amd.compare import score_functions as sf

    return getattr(sf, ed.NAMES[metric])


def _hits(records):
    from napkon_string_matching_amd import grid

    return grid.Hits(np.array([r[0] for r in records], dtype=np.float64), np.array([r[1] for r in records], dtype=np.int32),
                     np.array([r[2] for r in records], dtype=np.int32))


def _at(records, threshold):
    return [r for r in records if r[0] >= threshold]


_RAW = {}


def _raw_case(dev, metric, stride):
    """(left strings, right strings, left table, right table, every pair's record) of a RAW grid, built once per module."""
    from napkon_string_matching_amd import tables

    if ("tables", stride) not in _RAW:
        left, right = ed.raw_corpus(stride)
        lt, rt = tables.encode_strings(left, right, dev)
        assert lt.stride == rt.stride == stride
        _RAW["tables", stride] = (left, right, lt, rt)
    left, right, lt, rt = _RAW["tables", stride]
    if (metric, stride) not in _RAW:
        _RAW[metric, stride] = ed.raw_hits(metric, left, right)
    return left, right, lt, rt, _RAW[metric, stride]


# =============================================================================================== 1: RAW threshold grids
@pytest.mark.parametrize("stride", ed.STRIDES)
@pytest.mark.parametrize("metric", ed.METRICS)
def test_raw_grid_records(dev, metric, stride):
    from napkon_string_matching_amd import grid

    left, right, lt, rt, full = _raw_case(dev, metric, stride)
    assert len(full) == len(left) * len(right) and len(left) % 8 != 0
    for t in ed.thresholds_around(ed.RAW_THRESHOLDS[metric]):
        want = _at(full, t)
        assert 0 < len(want) and (t == 0.0) == (len(want) == len(full))
        for prune in (True, False):
            got = grid.indel_raw_grid(lt, rt, t, prune=prune, metric=metric)
            assert got.as_tuples() == want, (metric, stride, t, prune)
    for t in ed.RAW_THRESHOLDS[metric]:  # the pair on the threshold leaves with nextafter(t)
        assert len(_at(full, math.nextafter(t, -1.0))) == len(_at(full, t)) > len(_at(full, math.nextafter(t, 2.0)))
    if stride == 64:  # the plug-in encodes the same lists itself
        t = ed.RAW_THRESHOLDS[metric][1]
        assert _plugin(metric).raw_grid(left, right, t, device=dev).as_tuples() == _at(full, t)
        assert _plugin(metric).raw_grid(left, right, t, device=dev, prune=False).as_tuples() == _at(full, t)


def test_greatest_distance_without_slack(dev):
    """Pairs whose histogram bound is attained, at thresholds where the start guess of ``edit_most`` has no slack: a start
    one lower drops them from the pruned sweep (tests/test_cpu_edit_distance.py checks the inputs)."""
    from napkon_string_matching_amd import grid, tables

    left, right = ed.sharp_corpus()
    lt, rt = tables.encode_strings(left, right, dev)
    for metric in ed.METRICS:
        full = ed.raw_hits(metric, left, right)
        for k, (n, x) in enumerate(ed.SHARP):
            base = ed.score(metric, n, n, x)
            assert (base, k, k) in full
            for t in (math.nextafter(base, -1.0), base, math.nextafter(base, 2.0)):
                for prune in (True, False):
                    assert grid.indel_raw_grid(lt, rt, t, prune=prune, metric=metric).as_tuples() == _at(full, t), (metric, k, t, prune)
                assert grid.indel_raw_top_k(lt, rt, 1, t, metric=metric).as_tuples() == grid.select_top_k(_hits(_at(full, t)), 1).as_tuples()
                prof = grid.indel_raw_profile(lt, rt, [t], metric=metric)
                assert prof.pairs.tolist() == [len(_at(full, t))]


def test_saturated_histogram_buckets(dev):
    """Stride 512 with rows of more than 255 copies of one symbol: their histogram bucket saturates, and the
    NSM_METRIC_EDIT filter runs on it all the same.  Every distinct score of the grid is a threshold in turn, with its two
    neighbours, pruned against unpruned against the DP."""
    from napkon_string_matching_amd import grid, tables

    left, right = ed.saturated_corpus()
    lt, rt = tables.encode_strings(left, right, dev)
    assert lt.stride == 512 and int(lt.hist.max().item()) == 255 and int(rt.hist.max().item()) == 255
    for metric in ed.METRICS:
        full = ed.raw_hits(metric, left, right)
        for base in sorted({h[0] for h in full}):
            for t in (math.nextafter(base, -1.0), base, math.nextafter(base, 2.0)):
                for prune in (True, False):
                    assert grid.indel_raw_grid(lt, rt, t, prune=prune, metric=metric).as_tuples() == _at(full, t), (metric, t, prune)
            want = grid.select_top_k(_hits(_at(full, base)), 2).as_tuples()
            assert grid.indel_raw_top_k(lt, rt, 2, base, metric=metric).as_tuples() == want
        pi, pj = np.repeat(np.arange(len(left)), len(right)), np.tile(np.arange(len(right)), len(left))
        score = {(i, j): v for v, i, j in full}
        assert grid.indel_raw_pairs(lt, rt, pi, pj, metric=metric).tolist() == [score[p] for p in zip(pi.tolist(), pj.tolist())]


def test_plugin_call_by_hand(dev):
    match, inside = _plugin("edit"), _plugin("edit_within")
    assert match("kitten", "sitting") == 1 - 3 / 7
    assert match("lewenstein", "levenshtein") == 1 - 2 / 11
    assert match("gewicht", "gewicht des patienten bei aufnahme") == 1 - 27 / 34
    assert inside("gewicht", "gewicht des patienten bei aufnahme") == 1.0
    assert inside("gewischt", "das gewicht bei aufnahme") == 0.875
    assert inside("gewicht des patienten bei aufnahme", "gewicht") == 1 - 27 / 34  # the left string stays the pattern
    assert match("", "abc") == match("abc", "") == inside("", "abc") == inside("abc", "") == inside("", "") == 0.0
    assert match(["Bei", "aufnahme", "Gewicht"], "aufnahme bei gewicht!") == 1.0  # join_sorted, then default_process
    for a, b in (("a b c", "b c d e f"), (ed.text(130, 1), ed.text(200, 2)), (ed.text(300, 1), ed.text(300, 1)[5:250])):
        assert match(a, b) == ed.levenshtein_match(a, b) and inside(a, b) == ed.levenshtein_within(a, b)


# ================================================================================================ 2: the other RAW queries
@pytest.mark.parametrize("stride", [64, 256])
@pytest.mark.parametrize("metric", ed.METRICS)
def test_raw_top_k(dev, metric, stride):
    from napkon_string_matching_amd import grid

    left, right, lt, rt, full = _raw_case(dev, metric, stride)
    groups = [j % 7 for j in range(len(right))]
    for t in (0.0, ed.RAW_THRESHOLDS[metric][0]):
        for k in (1, 3, 64):
            for g in (None, groups):
                gcol = None if g is None else np.array(g, dtype=np.int32)
                want = grid.select_top_k(_hits(_at(full, t)), k, gcol).as_tuples()
                assert len(want) > 0
                for prune in (True, False):
                    got = grid.indel_raw_top_k(lt, rt, k, t, prune=prune, groups=gcol, metric=metric)
                    assert got.as_tuples() == want, (metric, stride, t, k, g is not None, prune)
                if stride == 64 and k == 3:
                    assert _plugin(metric).top_k(left, right, k, t, device=dev, groups=g).as_tuples() == want


@pytest.mark.parametrize("metric", ed.METRICS)
def test_raw_profile_and_best(dev, metric):
    from napkon_string_matching_amd import grid

    left, right, lt, rt, full = _raw_case(dev, metric, 128)
    rungs = set(ed.thresholds_around(ed.RAW_THRESHOLDS[metric]))  # 64 rungs: the exact thresholds, then an even spread
    for v in np.linspace(0.0, 1.0, 90).tolist():
        if len(rungs) < 64:
            rungs.add(v)
    ladder = sorted(rungs)
    assert len(ladder) == 64 and ladder[0] == 0.0
    want = grid.profile_of_hits(_hits(_at(full, ladder[0])), ladder, len(left), len(right))
    for prune in (True, False):
        got = _plugin(metric).profile(left, right, ladder, device=dev, prune=prune)
        assert got.pairs.tolist() == want.pairs.tolist() and got.pairs[0] > got.pairs[-1] > 0
        assert got.left_best.tolist() == want.left_best.tolist() and got.right_best.tolist() == want.right_best.tolist()
    for mutual in (True, False):
        for margin in (0.0, 0.125):
            want = grid.best_of_hits(_hits(_at(full, 0.0)), margin, mutual, len(left), len(right)).as_tuples()
            got = _plugin(metric).best(left, right, margin=margin, threshold=0.0, mutual=mutual, device=dev)
            assert got.as_tuples() == want and len(want) >= (1 if mutual else len(left)), (metric, mutual, margin)


@pytest.mark.parametrize("stride", ed.STRIDES)
@pytest.mark.parametrize("metric", ed.METRICS)
def test_raw_pairs(dev, metric, stride):
    """Listed pairs: duplicates, an id no table holds, empty strings (0.0), and both orders of the same two strings -- the
    wave-per-pair kernel must keep the LEFT string as the pattern whichever is shorter."""
    from napkon_string_matching_amd import grid, tables

    left, right, _, _, full = _raw_case(dev, metric, stride)
    score = {(i, j): s for s, i, j in full}
    n_l, n_r = len(left), len(right)
    pi = [k % n_l for k in range(0, 5 * n_l, 3)] + [n_l - 1, n_l - 1, 0, 5, 5, n_l + 3, 2]
    pj = [(7 * k + 1) % n_r for k in range(len(pi) - 7)] + [n_r - 1, 4, n_r - 1, 9, 9, 1, n_r]
    want = [score.get((a, b), -1.0) for a, b in zip(pi, pj)]
    assert want.count(-1.0) == 2 and want.count(0.0) >= 1 and len(set(zip(pi, pj))) < len(pi)
    lt, rt = _RAW["tables", stride][2:]
    assert grid.indel_raw_pairs(lt, rt, np.array(pi), np.array(pj), metric=metric).tolist() == want
    # the swap: every (a, b) beside (b, a), the longer string on the left and on the right
    both = left + right
    lt2, rt2 = tables.encode_strings(both, both, dev)
    qi = list(range(len(left))) * 2
    qj = [len(left) + (3 * k) % n_r for k in range(len(left))] * 2
    qi, qj = qi + qj, qj + qi
    want = [ed.FAST[metric](both[a], both[b]) for a, b in zip(qi, qj)]
    got = grid.indel_raw_pairs(lt2, rt2, np.array(qi), np.array(qj), metric=metric).tolist()
    assert got == want
    half = len(qi) // 2
    assert (metric == "edit") == (want[:half] == want[half:])  # the distance is symmetric, the occurrence is not
    if stride == 128:
        ok = [(a, b) for a, b in zip(pi, pj) if a < n_l and b < n_r]
        assert _plugin(metric).pairs(left, right, ok, device=dev).tolist() == [score[p] for p in ok]


@pytest.mark.parametrize("metric", ed.METRICS)
def test_raw_assign_groups_forest(dev, metric):
    from napkon_string_matching_amd import grid

    left, right, lt, rt, full = _raw_case(dev, metric, 64)
    n_l, n_r = len(left), len(right)
    plugin = _plugin(metric)
    for t in ed.RAW_THRESHOLDS[metric]:
        hits = _hits(_at(full, t))
        assert plugin.assign(left, right, t, device=dev).as_tuples() == grid.assign_of_hits(hits).as_tuples()
        groups = plugin.groups(left, right, t, device=dev)
        want_label = grid.groups_of_hits([(hits, 0, n_l)], n_l + n_r)
        assert groups.label.tolist() == want_label.tolist() and len(groups.members()) > 0
        forest = plugin.forest(left, right, t, device=dev)
        want_forest = grid.forest_of_hits([(hits, 0, n_l)], n_l + n_r, t)
        assert forest.as_tuples() == want_forest.as_tuples() and len(forest) > 0
        assert forest.cut(t).label.tolist() == want_label.tolist()
    items = right[:40]  # the self-join
    self_hits = _hits(ed.raw_hits(metric, items, items, 0.8))
    want = grid.groups_of_hits([(self_hits, 0, 0)], len(items))
    assert plugin.groups(items, items, 0.8, device=dev, same=True).label.tolist() == want.tolist()
    assert plugin.cluster_tree(items, 0.8, device=dev).cut(0.8).label.tolist() == want.tolist()
    assert [c.tolist() for c in plugin.clusters(items, 0.8, device=dev)] == \
        [m[0].tolist() for m in grid.MatchGroups(want, (0,), (len(items),)).members(2)]


# ============================================================================================ 3: NSM_METRIC_INDEL forwarding
def test_indel_through_the_new_entries(dev, monkeypatch):
    """NSM_METRIC_INDEL through nsm_edit_* gives the nsm_indel_* entry's records, record for record, on the same tables."""
    from napkon_string_matching_amd import _lib, grid, tables

    left, right, lt, rt = _raw_case(dev, "edit", 128)[:4]
    items_l, items_r = ed.levels_corpus(True)
    cl, cr = ed.levels_categories(len(items_l), len(items_r))
    li, ls, ri, rs = tables.encode_level_strings(items_l, items_r, dev, cl, cr, 2, partition=False)
    pi, pj = np.arange(len(left)).repeat(3), (np.arange(3 * len(left)) * 5) % len(right)
    ladder = [0.0, 0.3, 0.5, 1.0]

    def run():
        return {
            "top_k": grid.indel_raw_top_k(lt, rt, 3, 0.2).as_tuples(),
            "grouped": grid.indel_raw_top_k(lt, rt, 2, 0.0, groups=np.arange(len(right), dtype=np.int32) % 5).as_tuples(),
            "profile": [a.tolist() for a in (lambda p: (p.pairs, p.left_best, p.right_best))(grid.indel_raw_profile(lt, rt, ladder))],
            "floor": grid.indel_raw_floor_grid(lt, rt, 0.4).as_tuples(),
            "pairs": grid.indel_raw_pairs(lt, rt, pi, pj).tolist(),
            "levels floor": grid.indel_levels_floor_grid(li, ls, ri, rs, 0.3, category_mode=2).as_tuples(),
            "levels top_k": grid.indel_levels_top_k(li, ls, ri, rs, 2, 0.1, category_mode=2).as_tuples(),
            "levels profile": grid.indel_levels_profile(li, ls, ri, rs, ladder, category_mode=2).pairs.tolist(),
            "levels pairs": grid.indel_levels_pairs(li, ls, ri, rs, np.arange(len(items_l)),
                                                    np.arange(len(items_l)) % len(items_r)).tolist(),
        }

    want = run()
    used = []

    def through_edit(entry, metric):
        assert metric == "indel"
        used.append(entry.replace("nsm_indel_", "nsm_edit_"))
        return used[-1], (_lib.METRIC_INDEL,)

    monkeypatch.setattr(grid, "_edit_entry", through_edit)
    got = run()
    assert set(used) | {"nsm_edit_raw_top_k_grouped"} == set(_lib.EDIT_EXPORTS)
    assert got == want and all(len(v) > 0 for v in want.values())


# ======================================================================================================== 4: levels
_LEVELS = {}


def _levels_case(dev, wide, mode):
    from napkon_string_matching_amd import tables

    key = (wide, mode)
    if key not in _LEVELS:
        left, right = ed.levels_corpus(wide)
        cl, cr = ed.levels_categories(len(left), len(right)) if mode else (None, None)
        li, ls, ri, rs = tables.encode_level_strings(left, right, dev, cl, cr, mode, partition=False)
        assert ls.stride == (256 if wide else 64)
        keep = (lambda i, j: True) if not mode else (lambda i, j: ed.category_match(int(cl[i]), int(cr[j]), mode))
        _LEVELS[key] = (left, right, (li, ls, ri, rs), keep)
    return _LEVELS[key]


def _levels_full(metric, wide, monkeypatch):
    """Every pair's ``compare_terms`` with the registered definition, once per (metric, corpus)."""
    from oracle import score_functions as osf

    if ("full", metric, wide) not in _LEVELS:
        left, right = ed.levels_corpus(wide)
        with ed.registered(monkeypatch, fast=True):
            f = osf.get(ed.NAMES[metric])  # the registered callable, as the oracle's compare_terms gets it
            _LEVELS["full", metric, wide] = ed.levels_hits(metric, left, right, f=f)
    return _LEVELS["full", metric, wide]


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("metric", ed.METRICS)
def test_levels_padding_trap(dev, metric, wide, monkeypatch):
    """Right level strings of lengths 1, 5, 63, 64 (and 65, 127, 128, 129) in ONE 64-lane batch against the same left
    level: the wave walks to the longest text, each lane must stop at its own."""
    from napkon_string_matching_amd import grid

    left, right, tabs, _ = _levels_case(dev, wide, 0)
    assert len(right) <= 64
    lens = sorted({len(r[0]) for r in right if len(r) == 1})
    assert set(lens) >= ({1, 5, 63, 64, 65, 127, 128, 129} if wide else {1, 5, 63, 64})
    full = _levels_full(metric, wide, monkeypatch)
    assert len(full) == len(left) * len(right)
    for prune in (True, False):
        assert grid.indel_levels_grid(*tabs, float("-inf"), prune=prune, metric=metric).as_tuples() == full
    pi = np.array([i for i in range(len(left)) for _ in range(len(right))])
    pj = np.array([j for _ in range(len(left)) for j in range(len(right))])
    score = {(i, j): s for s, i, j in full}
    assert grid.indel_levels_pairs(*tabs, pi, pj, metric=metric).tolist() == [score[p] for p in zip(pi.tolist(), pj.tolist())]


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("metric", ed.METRICS)
def test_levels_queries(dev, metric, wide, mode, monkeypatch):
    from napkon_string_matching_amd import grid

    left, right, tabs, keep = _levels_case(dev, wide, mode)
    full = [h for h in _levels_full(metric, wide, monkeypatch) if keep(h[1], h[2])]
    assert 0 < len(full) and (mode == 0) == (len(full) == len(left) * len(right))
    best_of_row = {}
    for s, i, j in full:
        best_of_row.setdefault(i, (i, j))
    banned = set(list(best_of_row.values())[::2]) | {(1, j) for j in range(len(right))}
    as_arrays = lambda ban: None if not ban else (np.array([p[0] for p in sorted(ban)]), np.array([p[1] for p in sorted(ban)]))
    for ban in (set(), banned):
        allowed = [h for h in full if (h[1], h[2]) not in ban]
        for base in ed.levels_thresholds(allowed):
            assert len(_at(allowed, math.nextafter(base, 2.0))) < len(_at(allowed, base)) < len(allowed)
            for t in (math.nextafter(base, -1.0), base, math.nextafter(base, 2.0)):
                want = _at(allowed, t)
                for prune in (True, False):
                    got = grid.indel_levels_grid(*tabs, t, category_mode=mode, prune=prune, metric=metric, banned=as_arrays(ban))
                    assert got.as_tuples() == want, (metric, wide, mode, t, prune, len(ban))
        for k in (1, 2):
            want = grid.select_top_k(_hits(_at(allowed, 0.25)), k).as_tuples()
            for prune in (True, False):
                got = grid.indel_levels_top_k(*tabs, k, 0.25, category_mode=mode, prune=prune, banned=as_arrays(ban), metric=metric)
                assert got.as_tuples() == want, (metric, wide, mode, k, prune, len(ban))
        ladder = [0.125, 0.25, 0.5, math.nextafter(0.5, 2.0), 0.75]
        want = grid.profile_of_hits(_hits(_at(allowed, ladder[0])), ladder, len(left), len(right))
        got = grid.indel_levels_profile(*tabs, ladder, category_mode=mode, banned=as_arrays(ban), metric=metric)
        assert got.pairs.tolist() == want.pairs.tolist() and got.pairs[0] > got.pairs[-1]
        assert got.left_best.tolist() == want.left_best.tolist() and got.right_best.tolist() == want.right_best.tolist()
        if ban:
            assert got.left_best[1] == -1.0  # every pair of left item 1 is banned
        want = grid.best_of_hits(_hits(_at(allowed, 0.25)), 0.0, True, len(left), len(right)).as_tuples()
        got = grid.indel_levels_best(*tabs, 0.0, 0.25, mutual=True, category_mode=mode, banned=as_arrays(ban), metric=metric)
        assert got.as_tuples() == want and len(want) > 0


# ================================================================================================== 5: explicit floors
def _with_caller_ids(table):
    """The table reporting caller ids with gaps: row r reports ``ed.caller_id`` of what it reported."""
    import copy

    out = copy.copy(table)
    out.orig = table.orig * 3 + 2
    return out


@pytest.mark.parametrize("shift", ed.FLOOR_SHIFTS)
@pytest.mark.parametrize("kind", ed.FLOOR_CORPORA)
@pytest.mark.parametrize("metric", ed.METRICS)
def test_explicit_floors(dev, metric, kind, shift, monkeypatch):
    """``nsm_edit_raw_floor_grid`` / ``nsm_edit_levels_floor_grid`` with ``left_floor`` / ``right_floor`` arrays of the
    caller's own (``best`` only ever derives them from a profile): indexed by caller ids with gaps, on the left side only,
    on the right side only and on both, sitting on every item's best and second-best score ("on"), one double below and
    one above; one left item's floor lies above all of its scores.  Expected: ``grid.filter_by_floors`` of every pair's
    record.  tests/test_cpu_edit_distance.py checks that every "on" floor has a pair exactly on it."""
    from napkon_string_matching_amd import grid

    if kind.startswith("raw_"):
        left, right, lt, rt, full = _raw_case(dev, metric, int(kind[4:]))
        tabs = (_with_caller_ids(lt), _with_caller_ids(rt))
        run = lambda lf, rf, prune: grid.indel_raw_floor_grid(*tabs, 0.0, lf, rf, prune=prune, metric=metric)
    else:
        wide = kind == "levels_wide"
        left, right, (li, ls, ri, rs), _ = _levels_case(dev, wide, 0)
        full = _levels_full(metric, wide, monkeypatch)
        tabs = (_with_caller_ids(li), ls, _with_caller_ids(ri), rs)
        run = lambda lf, rf, prune: grid.indel_levels_floor_grid(*tabs, 0.0, lf, rf, prune=prune, metric=metric)
    assert len(full) == len(left) * len(right)
    hits = _hits([(s, ed.caller_id(i), ed.caller_id(j)) for s, i, j in full])
    for label, lf, rf in ed.floor_cases(full, len(left), len(right), ed.FLOOR_SHIFTS[shift]):
        lf, rf = (None if f is None else ed.by_caller_id(f) for f in (lf, rf))
        want = grid.filter_by_floors(hits, lf, rf).as_tuples()
        assert not any(i == ed.caller_id(ed.ABOVE_ALL) for _, i, _ in want) or lf is None
        for prune in (True, False):
            got = run(lf, rf, prune).as_tuples()
            assert got == want, f"{metric} {kind} floors {shift} their scores, {label}, prune={prune}: " \
                                f"{len(got)} records, expected {len(want)}; only in got {sorted(set(got) - set(want))[:4]}, " \
                                f"lost {sorted(set(want) - set(got))[:4]}"


# ================================================================================================= 6: the public surface
WORDS = ["gewicht", "groesse", "alter", "patient", "aufnahme", "blutdruck", "systolisch", "diastolisch", "kg", "cm"]
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


@pytest.mark.parametrize("metric", ed.METRICS)
def test_compare_against_the_oracle(dev, metric, monkeypatch):
    from napkon_string_matching_amd.types.questionnaire import Questionnaire
    from oracle import compare as oc

    name = ed.NAMES[metric]
    left, right = _cohort(1, 26), _cohort(2, 31)
    ql, qr = Questionnaire(left), Questionnaire(right)
    blacklist = {"b": {"hap": [left["Identifier"][3], left["Identifier"][8]], "pop": list(right["Identifier"][:12])}}
    with ed.registered(monkeypatch):
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
        f = ed.DEFINITIONS[metric]
        want = [oc.compare_terms(oc.gen_comp_value(left["Term"][pos_l[a]]), oc.gen_comp_value(right["Term"][pos_r[b]]), f)
                for a, b in listed]
        assert got.dataframe()["MatchScore"].tolist() == want


@pytest.mark.parametrize("metric", ed.METRICS)
def test_compare_refuses_what_only_the_general_kernels_take(dev, metric):
    """A level string beyond 512 code units is NotImplementedError with a new metric (the general kernels score the Indel
    ratio alone), in ``compare`` and ``score_pairs``; ``fuzzy_match`` still takes it."""
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    name = ed.NAMES[metric]
    kw = dict(compare_column="Term", left_name="hap", right_name="pop", score_threshold=0.2)
    long = " ".join(f"wort{q}" for q in range(90))  # (a level is the sorted SET of its tokens: distinct ones)
    assert len(long) > 512
    left, right = _cohort(5, 8), _with_term(_cohort(6, 9), 4, ["gewicht kg", long])
    with pytest.raises(NotImplementedError) as err:
        Questionnaire(left).gen_comparable(Questionnaire(right), {}, {}, score_func=name, **kw)
    assert metric in str(err.value) and name in str(err.value)
    assert len(Questionnaire(left).gen_comparable(Questionnaire(right), {}, {}, score_func="fuzzy_match", **kw).dataframe()) > 0
    with pytest.raises(NotImplementedError):
        Questionnaire(left).score_pairs(Questionnaire(right), [(left["Identifier"][0], right["Identifier"][4])], score_func=name,
                                        compare_column="Term", left_name="hap", right_name="pop")


def test_matcher_gecco_with_levenshtein_within(dev, monkeypatch):
    """The motivating example: a short GECCO definition against long questionnaire items.  Occurring verbatim in the item
    it scores as a full match under levenshtein_within; the Indel ratio leaves it below the threshold.  The frame is the
    oracle's ``gen_comparable`` with the definition registered."""
    from napkon_string_matching_amd.matcher import Matcher
    from napkon_string_matching_amd.types.questionnaire import Questionnaire
    from oracle import compare as oc

    frame = lambda rows: pd.DataFrame([[ident, f"v{k}", "s", [], [term], term.split(), "p"] for k, (ident, term) in enumerate(rows)],
                                      columns=COLUMNS)
    gecco_df = frame([("g-weight", "Gewicht"), ("g-height", "Groesse"), ("g-age", "Alter Jahre")])
    hap_df = frame([("h-1", "Gewicht des Patienten bei Aufnahme"), ("h-2", "Groesse Patient cm"), ("h-3", "Blutdruck systolisch"),
                    ("h-4", "Alter Patient")])
    gecco, hap = Questionnaire(gecco_df), Questionnaire(hap_df)
    matching = dict(compare_column="Term", score_threshold=0.45, cached=False)
    pairs = {}
    for func in ("levenshtein_within", "fuzzy_match"):
        matcher = Matcher(None, {"matching": dict(matching, score_func=func)}, questionnaires={"hap": hap}, gecco=gecco)
        matcher.match_gecco_with_questionnaires()
        ((key, result),) = matcher.results.items()
        assert key == "gecco vs hap"
        df = result.dataframe()
        pairs[func] = {(a, b): s for a, b, s in zip(df["GeccoIdentifier"], df["HapIdentifier"], df["MatchScore"])}
    # one level each: the score is 2^-1 * m(a, b)
    assert pairs["levenshtein_within"] == {("g-weight", "h-1"): 0.5, ("g-height", "h-2"): 0.5}
    assert ("g-weight", "h-1") not in pairs["fuzzy_match"]
    with ed.registered(monkeypatch):
        want = oc.gen_comparable(gecco_df, hap_df, {}, {}, score_func="levenshtein_within", compare_column="Term",
                                 left_name="gecco", right_name="hap", score_threshold=0.45)
    assert sorted(want["MatchScore"].tolist()) == sorted(pairs["levenshtein_within"].values())
