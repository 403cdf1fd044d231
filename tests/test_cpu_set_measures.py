"""The token-set measures beside Jaccard (intersection_vs_mean / _smaller / _left), as far as no device is needed: the
definitions the GPU tests are measured against, the C header and its bindings, the argument checks that end before the first
HIP call, the host errors the plug-ins raise before they ask for a device, and a self-check of the GPU tests' inputs."""
import ctypes
import re
from pathlib import Path

import pytest

from support import set_measures as sm

ROOT = Path(__file__).resolve().parent.parent
BADARG = 10001


# ------------------------------------------------------------------------------------------------------- definitions
def test_definitions_by_hand():
    a, b = ["x", "y", "z"], ["y", "z", "w", "v", "u"]  # 2 in common
    assert sm.intersection_vs_mean(a, b) == 2 * 2 / 8 == 0.5
    assert sm.intersection_vs_smaller(a, b) == 2 / 3
    assert sm.intersection_vs_left(a, b) == 2 / 3 and sm.intersection_vs_left(b, a) == 2 / 5  # asymmetric
    assert sm.intersection_vs_mean(b, a) == 0.5 and sm.intersection_vs_smaller(b, a) == 2 / 3
    assert sm.intersection_vs_left("x y", "y x q") == 1.0 and sm.intersection_vs_left("y x q", "x y") == 2 / 3
    assert sm.intersection_vs_mean(["x", "x"], ["x"]) == 1.0  # duplicates collapse, as in set()
    assert sm.intersection_vs_mean([], ["x"]) == 0.0 and sm.intersection_vs_left(["x"], []) == 0.0
    for f, left, right in ((sm.intersection_vs_mean, [], []), (sm.intersection_vs_smaller, [], ["x"]),
                           (sm.intersection_vs_smaller, ["x"], []), (sm.intersection_vs_left, [], ["x"])):
        with pytest.raises(ZeroDivisionError):
            f(left, right)
    for measure, pred in sm.DIVIDES_BY_ZERO.items():
        for na in range(3):
            for nb in range(3):
                raised = False
                try:
                    sm.DEFINITIONS[measure](sm.VOCAB[:na], sm.VOCAB[5:5 + nb])
                except ZeroDivisionError:
                    raised = True
                assert raised == pred(na, nb), (measure, na, nb)


def test_gewicht_example():
    """The GECCO definition {"Gewicht"} is contained in the questionnaire item: 1.0 / 1.0 / 0.4 / 0.25."""
    left, right = ["Gewicht"], ["Gewicht", "Patient", "Aufnahme", "kg"]
    assert sm.intersection_vs_left(left, right) == 1.0
    assert sm.intersection_vs_smaller(left, right) == 1.0
    assert sm.intersection_vs_mean(left, right) == 0.4
    assert sm.intersection_vs_union(left, right) == 0.25
    assert sm.intersection_vs_left(right, left) == 0.25


# ------------------------------------------------------------------------------------------------ header and bindings
def test_symbol_header_and_binding():
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    assert len(_lib.MEASURE_EXPORTS) == 9 and all(name.startswith("nsm_set_") for name in _lib.MEASURE_EXPORTS)
    others = set(_lib.EXPORTS) | set(_lib.ASSIGN_EXPORTS) | set(_lib.GROUP_EXPORTS) | set(_lib.SPAN_EXPORTS)
    assert not set(_lib.MEASURE_EXPORTS) & others
    assert (_lib.MEASURE_UNION, _lib.MEASURE_MEAN, _lib.MEASURE_SMALLER, _lib.MEASURE_LEFT) == (0, 1, 2, 3)
    assert _lib.MEASURES == {"union": 0, "mean": 1, "smaller": 2, "left": 3}
    for name in _lib.MEASURE_EXPORTS:
        fn, twin = _lib.entry(name), getattr(lib, name.replace("nsm_set_", "nsm_jaccard_"))
        assert fn.restype is ctypes.c_int
        # the Jaccard entry's arguments with the measure (int32) after `right`
        assert list(fn.argtypes) == list(twin.argtypes[:2]) + [ctypes.c_int32] + list(twin.argtypes[2:]), name
    assert lib.nsm_abi_version() == 5 == _lib.ABI_VERSION
    text = (ROOT / "include" / "nsm_hip_measures.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|uint64_t|const char\*)\s+(nsm_\w+)\s*\(", text, flags=re.M))
    assert declared == set(_lib.MEASURE_EXPORTS)
    assert '#include "nsm_hip.h"' in text
    for name, code in (("UNION", 0), ("MEAN", 1), ("SMALLER", 2), ("LEFT", 3)):
        assert re.search(rf"#define NSM_MEASURE_{name}\s+{code}\b", text)
    assert "#define NSM_ABI_VERSION 5" in (ROOT / "include" / "nsm_hip.h").read_text()
    assert "nsm_hip_measures.h" in (ROOT / "napkon-string-matching_amd" / "csrc" / "Makefile").read_text()


def _calls(measure, left, right):
    """Every nsm_set_* entry with non-null pointers that are never dereferenced (each case ends before the first HIP call)."""
    from napkon_string_matching_amd import _lib

    p = 0x1000
    e = _lib.entry
    return {
        "nsm_set_raw_top_k": lambda: e("nsm_set_raw_top_k")(left, right, measure, 0.5, 1, 0, p, p, None, None),
        "nsm_set_raw_top_k_grouped": lambda: e("nsm_set_raw_top_k_grouped")(left, right, measure, p, 0.5, 1, 0, p, p, None, None),
        "nsm_set_raw_profile": lambda: e("nsm_set_raw_profile")(left, right, measure, p, 1, 0, p, p, p, None, None),
        "nsm_set_raw_floor_grid": lambda: e("nsm_set_raw_floor_grid")(left, right, measure, 0.5, None, None, 0, p, 16, p, None, None),
        "nsm_set_raw_pairs": lambda: e("nsm_set_raw_pairs")(left, right, measure, p, 1, p, 1, p, 1, None),
        "nsm_set_levels_top_k": lambda: e("nsm_set_levels_top_k")(left, right, measure, 0.5, 1, 0, 0, None, None, p, p, None, None),
        "nsm_set_levels_profile": lambda: e("nsm_set_levels_profile")(left, right, measure, p, 1, 0, 0, None, None, p, p, p, None,
                                                                      None),
        "nsm_set_levels_floor_grid": lambda: e("nsm_set_levels_floor_grid")(left, right, measure, 0.5, None, None, 0, 0, None, None,
                                                                            p, 16, p, None, None),
        "nsm_set_levels_pairs": lambda: e("nsm_set_levels_pairs")(left, right, measure, p, 1, p, 1, p, 1, None),
    }


def test_argument_checks_that_need_no_device():
    from napkon_string_matching_amd import _lib

    error = lambda: _lib.load().nsm_last_error().decode()
    table = _lib.NsmSetTable()  # (all zero: never read, the measure is checked first)
    for bad in (4, -1, 99):
        calls = _calls(bad, ctypes.byref(table), ctypes.byref(table))
        assert set(calls) == set(_lib.MEASURE_EXPORTS)
        for name, call in calls.items():
            assert call() == BADARG, name
            assert name + ":" in error() and "measure" in error() and str(bad) in error(), (name, error())
    for measure in (0, 1, 2, 3, 7):  # a null table is reported first, whatever the measure
        for left, right in ((None, ctypes.byref(table)), (ctypes.byref(table), None)):
            for name, call in _calls(measure, left, right).items():
                assert call() == BADARG, name
                assert name + ":" in error() and "null" in error(), (name, error())


# ------------------------------------------------------------------------------------- plug-ins: errors before the device
PLUGIN_RULES = {
    # measure: ((left items, right items) that raise, ...), ((left, right) that do not raise here, ...)
    "mean": ([(["a", ""], ["b", ""])], [(["a", ""], ["b"]), (["a"], ["b", ""])]),
    "smaller": ([(["a", ""], ["b"]), (["a"], ["b", ""]), ([""], ["b"])], [(["a"], ["b"]), (["a", ""], [])]),
    "left": ([(["a", ""], ["b"]), ([""], [""])], [(["a"], ["b", ""]), (["a", ""], [])]),
}


def _no_device(monkeypatch):
    """Make asking for the device an error of its own kind: a check that runs first never gets there."""
    from napkon_string_matching_amd.compare import score_functions as sf

    class Asked(Exception):
        pass

    def asked():
        raise Asked()

    monkeypatch.setattr(sf, "_device", asked)
    return Asked


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_plugin_resolves_and_describes_itself(measure):
    from napkon_string_matching_amd.compare import score_functions as sf

    plugin = getattr(sf, sm.NAMES[measure])
    assert plugin.kind == "sets" and plugin.measure == measure and plugin.__name__ == sm.NAMES[measure]
    assert plugin in sf.PLUGINS and sf.intersection_vs_union.measure == "union"
    for na in range(3):
        for nb in range(3):
            assert plugin.divides_by_zero(na, nb) == sm.DIVIDES_BY_ZERO[measure](na, nb)
            assert plugin.divides_by_zero(set(sm.VOCAB[:na]), set(sm.VOCAB[:nb])) == sm.DIVIDES_BY_ZERO[measure](na, nb)
    for method in ("raw_grid", "top_k", "pairs", "profile", "best", "assign", "groups", "clusters", "forest", "cluster_tree"):
        assert callable(getattr(plugin, method))
    common = {"Dice": "mean", "overlap": "smaller", "containment": "left"}
    assert any(word in type(plugin).__doc__ for word, m in common.items() if m == measure)


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_plugin_zero_division_before_the_device(measure, monkeypatch):
    from napkon_string_matching_amd.compare import score_functions as sf

    asked = _no_device(monkeypatch)
    plugin = getattr(sf, sm.NAMES[measure])
    raising, fine = PLUGIN_RULES[measure]
    queries = {
        "raw_grid": lambda l, r: plugin.raw_grid(l, r, 0.5),
        "top_k": lambda l, r: plugin.top_k(l, r, 2, 0.5),
        "profile": lambda l, r: plugin.profile(l, r, [0.5]),
        "best": lambda l, r: plugin.best(l, r),
        "assign": lambda l, r: plugin.assign(l, r, 0.5),
        "groups": lambda l, r: plugin.groups(l, r, 0.5),
        "forest": lambda l, r: plugin.forest(l, r, 0.5),
    }
    for name, query in queries.items():
        for left, right in raising:
            with pytest.raises(ZeroDivisionError):
                query(left, right)
        for left, right in fine:
            if left and right:
                with pytest.raises(asked):  # nothing to raise for: the query goes on to the device
                    query(left, right)
    # pairs: the rule holds per listed pair, not for the whole grid
    left, right = ["a b", "", "c"], ["a", "", "b c d"]
    bad = {"mean": (1, 1), "smaller": (0, 1), "left": (1, 0)}[measure]
    good = {"mean": [(0, 1), (1, 0)], "smaller": [(0, 0), (2, 2)], "left": [(0, 1), (2, 1)]}[measure]
    with pytest.raises(ZeroDivisionError):
        plugin.pairs(left, right, good + [bad])
    with pytest.raises(asked):
        plugin.pairs(left, right, good)
    # and the plug-in called on one pair
    with pytest.raises(ZeroDivisionError):
        plugin(left[bad[0]], right[bad[1]])


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_plugin_refuses_wide_items_before_the_device(measure, monkeypatch):
    from napkon_string_matching_amd.compare import score_functions as sf

    _no_device(monkeypatch)
    plugin = getattr(sf, sm.NAMES[measure])
    wide = " ".join(f"w{k}" for k in range(65))
    narrow = " ".join(f"w{k % 64}" for k in range(80))  # 80 tokens, 64 distinct: fits
    for query in (lambda l, r: plugin.raw_grid(l, r, 0.5), lambda l, r: plugin.top_k(l, r, 1), lambda l, r: plugin.profile(l, r, [0.5]),
                  lambda l, r: plugin.best(l, r), lambda l, r: plugin.assign(l, r, 0.5), lambda l, r: plugin.groups(l, r, 0.5),
                  lambda l, r: plugin.forest(l, r, 0.5), lambda l, r: plugin.pairs(l, r, [(0, 0)])):
        for left, right in (([wide], ["a"]), (["a"], [wide])):
            with pytest.raises(NotImplementedError) as err:
                query(left, right)
            assert "64" in str(err.value) and measure in str(err.value) and sm.NAMES[measure] in str(err.value)
        with pytest.raises(Exception) as err:
            query([narrow], ["w1"])
        assert not isinstance(err.value, NotImplementedError)


def test_grid_measure_argument():
    from napkon_string_matching_amd import grid

    assert [grid.check_measure(m) for m in ("union", "mean", "smaller", "left")] == [0, 1, 2, 3]
    for bad in ("dice", None, 1, ["mean"]):
        with pytest.raises(ValueError):
            grid.check_measure(bad)
    for measure in ("union",) + sm.MEASURES:
        for na in range(3):
            for nb in range(3):
                assert grid.measure_divides_by_zero(measure, na, nb) == sm.DIVIDES_BY_ZERO[measure](na, nb)
    # the whole-grid rule: (left has an empty set, left rows, right has an empty set, right rows)
    table = {("union", True, 2, True, 2): True, ("union", True, 2, False, 2): False, ("mean", True, 2, True, 2): True,
             ("mean", False, 2, True, 2): False, ("smaller", True, 2, False, 2): True, ("smaller", False, 2, True, 2): True,
             ("smaller", True, 2, False, 0): False, ("smaller", False, 2, False, 2): False, ("left", True, 2, False, 2): True,
             ("left", False, 2, True, 2): False, ("left", True, 2, False, 0): False}
    for args, bad in table.items():
        if bad:
            with pytest.raises(ZeroDivisionError):
                grid.check_measure_grid(*args)
        else:
            grid.check_measure_grid(*args)


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_compare_terms_raises_before_the_device(measure):
    """``compare_terms`` with a new measure: the plug-in's predicate decides which visited step divides by zero."""
    from napkon_string_matching_amd.compare import score_functions as sf
    from napkon_string_matching_amd.types.comparable_data import ComparableData, _resolve_plugin

    plugin = getattr(sf, sm.NAMES[measure])
    assert _resolve_plugin(sm.NAMES[measure]) is plugin and _resolve_plugin(plugin) is plugin
    empty_then_full, full = [[], [], ["a", "b"]], [["a"], ["a", "b"]]
    cases = {"mean": ((empty_then_full, empty_then_full),), "smaller": ((empty_then_full, full), (full, empty_then_full)),
             "left": ((empty_then_full, full),)}[measure]
    for left, right in cases:
        with pytest.raises(ZeroDivisionError):
            ComparableData.compare_terms(left, right, plugin)
        with pytest.raises(ZeroDivisionError):
            sm.levels_hits(measure, [left], [right], -1.0)  # the definition raises for the same pair


@pytest.mark.parametrize("measure", sm.MEASURES)
def test_compare_refuses_more_than_64_category_labels(measure):
    """A new measure's grid is a per-item sweep, whose category predicate runs on the device: more than 64 distinct labels
    are refused in the prelude, before any launch (Jaccard moves the predicate to the host instead)."""
    import pandas as pd

    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    columns = ["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"]
    frame = lambda tag, n: pd.DataFrame([[f"{tag}{k}", f"v{k}", "s", [f"c{k}", f"c{(k + 1) % 70}"], ["a b", "c"], ["a"], "p"]
                                         for k in range(n)], columns=columns)
    with pytest.raises(NotImplementedError) as err:
        Questionnaire(frame("l", 70)).gen_comparable(Questionnaire(frame("r", 70)), {}, {}, score_func=sm.NAMES[measure],
                                                     compare_column="Term", left_name="hap", right_name="pop",
                                                     filter_categories=True)
    assert "64" in str(err.value) and sm.NAMES[measure] in str(err.value)


# ---------------------------------------------------------------------------------------------------- input self-check
@pytest.mark.parametrize("measure", sm.MEASURES)
def test_gpu_inputs_hold_every_threshold(measure):
    """The grids of tests/test_gpu_set_measures.py hold, for every threshold t they are asked at, a pair scoring exactly t
    and a pair below it -- so t separates records and nextafter(t) drops the pair on t.  (Threshold 0 has pairs exactly
    on it and nothing below: scores are never negative.)"""
    for width in (16, 32, 64):
        left, right = sm.raw_grid(measure, width)
        assert max(len(set(r)) for r in left + right) == width
        scores = [h[0] for h in sm.raw_hits(measure, left, right, float("-inf"))]
        assert len(scores) == sum(not sm.DIVIDES_BY_ZERO[measure](len(set(a)), len(set(b))) for a in left for b in right) \
            == len(left) * len(right)  # no pair of the grid divides by zero
        for t in sm.RAW_THRESHOLDS:
            assert t in scores and min(scores) < t, (width, t)
        assert 0.0 in scores
        if width == 16:
            for side in (left, right):
                assert {len(set(r)) for r in side} >= set(range(1, 17))
            assert len(left) % 8 != 0 and sum(len(set(r)) == 4 for r in right) > 64
            assert ([] in right) == (measure != "smaller")
        else:
            assert {len(set(r)) for r in left + right} & set(range(width // 2 + 1, width + 1))
    left, right = sm.levels_grid(measure)
    assert {len(it) for it in left} == {len(it) for it in right} | {1} == {1, 2, 3, 4}
    assert all(set(a) <= set(b) for it in left + right for a, b in zip(it, it[1:]))  # suffix-nested
    cl, cr = sm.levels_categories(len(left), len(right))
    for mode in (0, 1, 2):
        keep = (lambda i, j: True) if mode == 0 else (lambda i, j: sm.category_match(int(cl[i]), int(cr[j]), mode))
        scores = [h[0] for h in sm.levels_hits(measure, left, right, float("-inf"), keep)]
        for t in sm.LEVELS_THRESHOLDS:
            assert t in scores and min(scores) < t, (mode, t)
