"""The Levenshtein score functions (levenshtein_match / levenshtein_within), as far as no device is needed: the DP and the
definitions the GPU tests are measured against, host restatements of the kernels' column update and bounds checked against
that DP, the C header and its bindings, the argument checks that end before the first HIP call, the host errors the
plug-ins raise before they ask for a device, and a self-check of the GPU tests' inputs."""
import ctypes
import math
import random
import re
from pathlib import Path

import pytest

from support import edit_distance as ed

ROOT = Path(__file__).resolve().parent.parent
BADARG = 10001


# ------------------------------------------------------------------------------------------------------- definitions
def test_definitions_by_hand():
    assert ed.distance("kitten", "sitting") == 3 and ed.levenshtein_match("kitten", "sitting") == 1 - 3 / 7
    assert ed.distance("lewenstein", "levenshtein") == 2 and ed.levenshtein_match("lewenstein", "levenshtein") == 1 - 2 / 11
    long = "gewicht des patienten bei aufnahme"
    assert ed.distance("gewicht", long) == 27 and ed.levenshtein_match("gewicht", long) == 1 - 27 / 34
    assert ed.within("gewicht", long) == 0 and ed.levenshtein_within("gewicht", long) == 1.0
    assert ed.within("gewischt", "das gewicht bei aufnahme") == 1 and ed.levenshtein_within("gewischt", "das gewicht bei aufnahme") == 0.875
    assert ed.within(long, "gewicht") == 27 and ed.levenshtein_within(long, "gewicht") == 1 - 27 / 34  # asymmetric
    assert ed.within("kitten", "sitting") == 2
    # the empty substring is an occurrence: w never exceeds la
    assert ed.within("abc", "xyz") == 3 and ed.within("abc", "") == 3 and ed.within("", "abc") == 0
    assert ed.distance("", "abc") == 3 and ed.distance("abc", "") == 3
    # 0.0 when either prepared string is empty: no ZeroDivisionError
    for f in (ed.levenshtein_match, ed.levenshtein_within):
        assert f("", "abc") == f("abc", "") == f("", "") == f("!!", "abc") == f([], ["a"]) == 0.0
    # fuzzy_match's preparation: join_sorted for lists, then default_process
    assert ed.prepared(["Bei", "aufnahme", "Gewicht"]) == "aufnahme bei gewicht" == ed.prepared("Aufnahme-bei  gewicht!".replace("  ", " "))
    assert ed.levenshtein_match(["b", "A"], "a b") == 1.0
    rng = random.Random(7)
    for _ in range(200):  # the numpy rows are the same programme
        a = "".join(rng.choice("abcd") for _ in range(rng.randint(0, 20)))
        b = "".join(rng.choice("abcd") for _ in range(rng.randint(0, 24)))
        assert ed._dp_fast(a, b, False) == ed.distance(a, b) and ed._dp_fast(a, b, True) == ed.within(a, b)
        assert 0 <= ed.within(a, b) <= min(len(a), ed.distance(a, b)) and ed.distance(a, b) == ed.distance(b, a)
        assert ed.distance(a, b) >= abs(len(a) - len(b)) and ed.within(a, b) >= max(0, len(a) - len(b))


# ------------------------------------------------------------------------------------------- the kernels' restatements
def test_column_update_word_by_word():
    """The bit-vector column update with explicit carries across 64-bit words, against the DP, in both modes, at pattern
    lengths around every word boundary, for texts shorter than, equal to and longer than the pattern."""
    rng = random.Random(11)
    for la in ed.SEAMS + (2, 5, 200):
        a = ed.text(la, 1)
        texts = [a, a[:-1], a[1:], ed.text(la, 2), a[: la // 2], ed.text(max(1, la - 3), 3), ed.text(la + 40, 4),
                 ed.text(7, 5) + a + ed.text(9, 6), a[la // 3:] + ed.text(11, 7), ""]
        mutated = list(a)
        for _ in range(max(1, la // 9)):
            mutated[rng.randrange(la)] = rng.choice(ed.ALPHABET)
        texts.append("".join(mutated))
        for b in texts:
            assert ed.column(a, b, 1) == ed._dp_fast(a, b, False), (la, len(b))
            assert ed.column(a, b, 0) == ed._dp_fast(a, b, True), (la, len(b))
    # a text symbol the pattern does not hold costs one edit: a padded column is not harmless, unlike for an LCS
    assert ed.column("abc", "abc", 1) == 0 and ed.column("abc", "abc\x00\x00", 1) == 2


def test_greatest_distance_start_is_never_below_the_answer():
    """``edit_most``: for every la, lb <= 64 and every attainable score (and its neighbours on either side) the start of
    the walk is at or above the greatest distance that reaches it, and the walk ends on it."""
    lost = 0  # pairs exactly on their threshold that a start one lower would round away
    for metric in ed.METRICS:
        for la in range(1, 65):
            for lb in range(1, 65):
                den = max(la, lb) if metric == "edit" else la
                scores = [ed.score(metric, la, lb, x) for x in range(den + 1)]
                assert all(s1 > s2 for s1, s2 in zip(scores, scores[1:]))  # strictly falling in x
                for x, s in enumerate(scores):
                    for eff, answer in ((s, x), (math.nextafter(s, 2.0), x - 1), (math.nextafter(s, -1.0), x)):
                        if eff <= 0.0:
                            answer = den
                        assert ed.most_start(metric, la, lb, eff) >= answer, (metric, la, lb, x, eff)
                        assert ed.most(metric, la, lb, eff) == answer, (metric, la, lb, x, eff)
                        lost += ed.most(metric, la, lb, eff, start_offset=-1) < answer
                assert ed.most(metric, la, lb, 1.5) == -1 and ed.most(metric, la, lb, -1.0) == den
    # the mutation DESIGN 4.17 records: one lower, and pairs exactly on their threshold are lost (floor((1 - eff) den) lands
    # on x - 1 wherever the product rounds below x)
    assert lost > 0 and ed.most("edit", 7, 6, 1 - 3 / 7) == 3


def test_histogram_bound():
    """d >= ceil(L1 / 2) for the SAD of the 32-bucket rows: with two symbols in one bucket and with a saturated bucket."""
    code_of = {ch: k for k, ch in enumerate(ed.ALPHABET)}
    assert code_of["a"] & 31 == code_of["6"] & 31 and code_of["a"] != code_of["6"]  # 'a' and '6' share bucket 0
    rng = random.Random(3)
    cases = [("aaaa", "6666"), ("a6a6", "6a6a"), ("abc", "ab6"), ("a" * 300, "a" * 280 + "b" * 20), ("a" * 300, "b" * 300),
             ("a" * 256 + "b" * 10, "a" * 400), ("a" * 10, "a" * 300)]
    for _ in range(300):
        cases.append(("".join(rng.choice("ab6789") for _ in range(rng.randint(1, 30))),
                      "".join(rng.choice("ab67cd") for _ in range(rng.randint(1, 30)))))
    tight = 0
    for a, b in cases:
        ha, hb = ed.hist32(a, code_of), ed.hist32(b, code_of)
        l1 = ed.sad(ha, hb)
        d = ed._dp_fast(a, b, False)
        assert d >= (l1 + 1) // 2, (a[:12], b[:12])
        tight += d == (l1 + 1) // 2
    assert tight >= 1  # (the bound is attained)
    assert ed.hist32("a" * 300, code_of)[0] == 255 and ed.sad(ed.hist32("a" * 300, code_of), ed.hist32("a" * 280 + "b" * 20, code_of)) == 20
    # the occurrence distance prunes on lengths alone: the bound the kernels use for it, on a row with a saturated bucket
    for a, b in (("a" * 300, "a" * 260), ("a" * 260 + "b" * 40, "a" * 300), ("a" * 10, "a" * 300)):
        assert ed._dp_fast(a, b, True) >= max(0, len(a) - len(b))


def test_class_bounds_fall_away_from_the_own_length():
    """The RAW walk's class bound -- the score at the least possible distance -- never rises away from la."""
    for metric in ed.METRICS:
        least = (lambda la, lb: abs(la - lb)) if metric == "edit" else (lambda la, lb: max(0, la - lb))
        for la in range(0, 70):
            bounds = [ed.score(metric, la, lb, least(la, lb)) for lb in range(0, 140)]
            assert all(x >= y for x, y in zip(bounds[la:], bounds[la + 1:])) and all(x <= y for x, y in zip(bounds[:la], bounds[1:la + 1]))
            if metric == "edit_within" and la:
                assert all(x == 1.0 for x in bounds[la:])  # it prunes downwards only


# ------------------------------------------------------------------------------------------------ header and bindings
INDEL_TABLES = {"raw": 2, "levels": 4}  # table arguments in front of `metric`


def test_symbol_header_and_binding():
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    assert len(_lib.EDIT_EXPORTS) == 9 and all(name.startswith("nsm_edit_") for name in _lib.EDIT_EXPORTS)
    others = (set(_lib.EXPORTS) | set(_lib.ASSIGN_EXPORTS) | set(_lib.GROUP_EXPORTS) | set(_lib.SPAN_EXPORTS)
              | set(_lib.MEASURE_EXPORTS))
    assert not set(_lib.EDIT_EXPORTS) & others
    assert (_lib.METRIC_INDEL, _lib.METRIC_EDIT, _lib.METRIC_EDIT_WITHIN) == (0, 1, 2)
    assert _lib.METRICS == {"indel": 0, "edit": 1, "edit_within": 2} == ed.CODES
    for name in _lib.EDIT_EXPORTS:
        fn, twin = _lib.entry(name), getattr(lib, name.replace("nsm_edit_", "nsm_indel_"))
        assert fn.restype is ctypes.c_int
        n = INDEL_TABLES[name.split("_")[2]]  # the Indel entry's arguments with the metric (int32) after the last table
        assert list(fn.argtypes) == list(twin.argtypes[:n]) + [ctypes.c_int32] + list(twin.argtypes[n:]), name
    assert lib.nsm_abi_version() == 5 == _lib.ABI_VERSION
    text = (ROOT / "include" / "nsm_hip_edit.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|uint64_t|const char\*)\s+(nsm_\w+)\s*\(", text, flags=re.M))
    assert declared == set(_lib.EDIT_EXPORTS)
    assert '#include "nsm_hip.h"' in text
    for name, code in (("INDEL", 0), ("EDIT", 1), ("EDIT_WITHIN", 2)):
        assert re.search(rf"#define NSM_METRIC_{name}\s+{code}\b", text)
    assert "#define NSM_ABI_VERSION 5" in (ROOT / "include" / "nsm_hip.h").read_text()
    assert "nsm_hip_edit.h" in (ROOT / "napkon-string-matching_amd" / "csrc" / "Makefile").read_text()


def _calls(metric, items, strings):
    """Every nsm_edit_* entry with non-null pointers that are never dereferenced (each case ends before the first HIP
    call).  ``items`` / ``strings``: (left, right) table arguments."""
    from napkon_string_matching_amd import _lib

    p = 0x1000
    e = _lib.entry
    (li, ri), (ls, rs) = items, strings
    return {
        "nsm_edit_raw_top_k": lambda: e("nsm_edit_raw_top_k")(ls, rs, metric, 0.5, 1, 0, p, p, None, None),
        "nsm_edit_raw_top_k_grouped": lambda: e("nsm_edit_raw_top_k_grouped")(ls, rs, metric, p, 0.5, 1, 0, p, p, None, None),
        "nsm_edit_raw_profile": lambda: e("nsm_edit_raw_profile")(ls, rs, metric, p, 1, 0, p, p, p, None, None),
        "nsm_edit_raw_floor_grid": lambda: e("nsm_edit_raw_floor_grid")(ls, rs, metric, 0.5, None, None, 0, p, 16, p, None, None),
        "nsm_edit_raw_pairs": lambda: e("nsm_edit_raw_pairs")(ls, rs, metric, p, 1, p, 1, p, 1, None),
        "nsm_edit_levels_top_k": lambda: e("nsm_edit_levels_top_k")(li, ls, ri, rs, metric, 0.5, 1, 0, 0, None, None, p, p, None, None),
        "nsm_edit_levels_profile": lambda: e("nsm_edit_levels_profile")(li, ls, ri, rs, metric, p, 1, 0, 0, None, None, p, p, p,
                                                                        None, None),
        "nsm_edit_levels_floor_grid": lambda: e("nsm_edit_levels_floor_grid")(li, ls, ri, rs, metric, 0.5, None, None, 0, 0, None,
                                                                              None, p, 16, p, None, None),
        "nsm_edit_levels_pairs": lambda: e("nsm_edit_levels_pairs")(li, ls, ri, rs, metric, p, 1, p, 1, p, 1, None),
    }


def test_argument_checks_that_need_no_device():
    from napkon_string_matching_amd import _lib

    error = lambda: _lib.load().nsm_last_error().decode()
    strings, items = _lib.NsmStrTable(), _lib.NsmLevelItems()  # (all zero: never read, the metric is checked first)
    s, i = ctypes.byref(strings), ctypes.byref(items)
    for bad in (3, -1, 99):
        calls = _calls(bad, (i, i), (s, s))
        assert set(calls) == set(_lib.EDIT_EXPORTS)
        for name, call in calls.items():
            assert call() == BADARG, name
            assert name + ":" in error() and "metric" in error() and str(bad) in error(), (name, error())
    for metric in (0, 1, 2, 7):  # a null table is reported first, whatever the metric
        for strs in ((None, s), (s, None)):
            for name, call in _calls(metric, (i, i), strs).items():
                assert call() == BADARG, name
                assert name + ":" in error() and "null" in error(), (name, error())
        for its in ((None, i), (i, None)):
            for name, call in _calls(metric, its, (s, s)).items():
                if "_levels_" in name:
                    assert call() == BADARG, name
                    assert name + ":" in error() and "null" in error(), (name, error())


# ------------------------------------------------------------------------------------- plug-ins: errors before the device
def _no_device(monkeypatch):
    """Make asking for the device an error of its own kind: a check that runs first never gets there."""
    from napkon_string_matching_amd.compare import score_functions as sf

    class Asked(Exception):
        pass

    def asked():
        raise Asked()

    monkeypatch.setattr(sf, "_device", asked)
    return Asked


@pytest.mark.parametrize("metric", ed.METRICS)
def test_plugin_resolves_and_describes_itself(metric):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare import score_functions as sf
    from napkon_string_matching_amd.types.comparable_data import _resolve_plugin

    plugin = getattr(sf, ed.NAMES[metric])
    assert plugin.kind == "strings" and plugin.metric == metric and plugin.__name__ == ed.NAMES[metric]
    assert plugin in sf.PLUGINS and sf.fuzzy_match.metric == "indel" and isinstance(plugin, type(sf.fuzzy_match))
    assert _resolve_plugin(ed.NAMES[metric]) is plugin and _resolve_plugin(plugin) is plugin
    for method in ("raw_grid", "top_k", "pairs", "profile", "best", "assign", "groups", "clusters", "forest", "cluster_tree"):
        assert callable(getattr(plugin, method))
        assert getattr(type(plugin), method) is getattr(type(sf.fuzzy_match), method)  # one copy of every method
    assert "Levenshtein" in type(plugin).__doc__
    assert [grid.check_metric(m) for m in ("indel", "edit", "edit_within")] == [0, 1, 2]
    for bad in ("levenshtein", None, 1, ["edit"]):
        with pytest.raises(ValueError):
            grid.check_metric(bad)


@pytest.mark.parametrize("metric", ed.METRICS)
def test_plugin_refuses_wide_strings_before_the_device(metric, monkeypatch):
    """Strings beyond 512 code units and a grid of more than 255 distinct code units are the general kernels', which are
    Indel-only: NotImplementedError before the device is asked for; fuzzy_match goes on to the device."""
    from napkon_string_matching_amd.compare import score_functions as sf

    asked = _no_device(monkeypatch)
    plugin = getattr(sf, ed.NAMES[metric])
    long, fits = "a" * 513, "a" * 512
    many = "".join(chr(0x4E00 + k) for k in range(300))  # 300 distinct code units
    queries = (lambda l, r: plugin.raw_grid(l, r, 0.5), lambda l, r: plugin.top_k(l, r, 1), lambda l, r: plugin.profile(l, r, [0.5]),
               lambda l, r: plugin.best(l, r), lambda l, r: plugin.assign(l, r, 0.5), lambda l, r: plugin.groups(l, r, 0.5),
               lambda l, r: plugin.forest(l, r, 0.5), lambda l, r: plugin.pairs(l, r, [(0, 0)]), lambda l, r: plugin(l[0], r[0]))
    for query in queries:
        for left, right in (([long], ["a"]), (["a"], [long]), ([many], ["a"])):
            with pytest.raises(NotImplementedError) as err:
                query(left, right)
            assert "512" in str(err.value) and metric in str(err.value) and ed.NAMES[metric] in str(err.value)
        with pytest.raises(asked):
            query([fits], ["a"])
    with pytest.raises(asked):
        sf.fuzzy_match.raw_grid([long], ["a"], 0.5)


def test_grid_wrappers_refuse_an_unknown_metric_before_the_device():
    from napkon_string_matching_amd import grid

    calls = (lambda m: grid.indel_raw_grid(None, None, 0.5, metric=m), lambda m: grid.indel_raw_top_k(None, None, 1, 0.5, metric=m),
             lambda m: grid.indel_raw_profile(None, None, [0.5], metric=m), lambda m: grid.indel_raw_floor_grid(None, None, 0.5, metric=m),
             lambda m: grid.indel_raw_pairs(None, None, [0], [0], metric=m),
             lambda m: grid.indel_levels_grid(None, None, None, None, 0.5, metric=m),
             lambda m: grid.indel_levels_top_k(None, None, None, None, 1, 0.5, metric=m),
             lambda m: grid.indel_levels_profile(None, None, None, None, [0.5], metric=m),
             lambda m: grid.indel_levels_floor_grid(None, None, None, None, 0.5, metric=m),
             lambda m: grid.indel_levels_pairs(None, None, None, None, [0], [0], metric=m))
    for call in calls:  # (the tables are never looked at)
        with pytest.raises(ValueError) as err:
            call("levenshtein")
        assert "metric" in str(err.value)
    assert grid._edit_entry("nsm_indel_raw_top_k", "indel") == ("nsm_indel_raw_top_k", ())
    assert grid._edit_entry("nsm_indel_levels_profile", "edit_within") == ("nsm_edit_levels_profile", (2,))
    with pytest.raises(NotImplementedError):
        grid._edit_entry("nsm_indel_any_grid", "edit")  # the general kernels are Indel-only


@pytest.mark.parametrize("metric", ed.METRICS)
def test_compare_refuses_more_than_64_category_labels(metric):
    """A new metric's grid is a per-item sweep, whose category predicate runs on the device: more than 64 distinct labels
    are refused in the prelude, before any launch (fuzzy_match moves the predicate to the host instead)."""
    import pandas as pd

    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    columns = ["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"]
    frame = lambda tag, n: pd.DataFrame([[f"{tag}{k}", f"v{k}", "s", [f"c{k}", f"c{(k + 1) % 70}"], ["a b", "c"], ["a"], "p"]
                                         for k in range(n)], columns=columns)
    with pytest.raises(NotImplementedError) as err:
        Questionnaire(frame("l", 70)).gen_comparable(Questionnaire(frame("r", 70)), {}, {}, score_func=ed.NAMES[metric],
                                                     compare_column="Term", left_name="hap", right_name="pop",
                                                     filter_categories=True)
    assert "64" in str(err.value) and ed.NAMES[metric] in str(err.value)


# ---------------------------------------------------------------------------------------------------- input self-check
ON_THRESHOLD = {  # pairs scoring exactly (1st threshold, 2nd threshold) in raw_corpus(stride): literal counts
    ("edit", 64): (1, 1), ("edit", 128): (1, 1), ("edit", 256): (1, 1), ("edit", 512): (1, 1),
    ("edit_within", 64): (1, 3), ("edit_within", 128): (1, 3), ("edit_within", 256): (1, 3), ("edit_within", 512): (4, 3),
}


@pytest.mark.parametrize("stride", ed.STRIDES)
@pytest.mark.parametrize("metric", ed.METRICS)
def test_gpu_raw_inputs_hold_every_threshold(metric, stride):
    """The grids of tests/test_gpu_edit_distance.py hold, for every threshold t they are asked at, a pair scoring exactly t
    and a pair below it -- so t separates records and nextafter(t) drops the pair on t."""
    from napkon_string_matching_amd import tables

    left, right = ed.raw_corpus(stride)
    assert tables.pick_stride(max(len(s) for s in left + right)) == stride
    assert all(ed.prepared(s) == s for s in left + right)  # fixed points of the preparation
    assert len(left) % 8 == 3 and "" in left and "" in right
    lengths = {len(s) for s in left}
    assert lengths >= {n for n in ed.SEAMS if stride // 2 < n <= stride} | {1, 63, 64}
    by_len = {}
    for s in right:
        by_len[len(s)] = by_len.get(len(s), 0) + 1
    assert max(by_len.values()) > 64  # a length class of more than one 64-lane batch
    scores = [h[0] for h in ed.raw_hits(metric, left, right)]
    assert len(scores) == len(left) * len(right)
    on = tuple(scores.count(t) for t in ed.RAW_THRESHOLDS[metric])
    assert on == ON_THRESHOLD[metric, stride]
    for t in ed.RAW_THRESHOLDS[metric]:
        assert min(scores) < t < max(scores)
    assert scores.count(0.0) >= len(left) + len(right) - 1  # the empty strings
    # pairs that differ only in their last / only in their first code unit, and occurrences at the start, middle and end
    for n in (k for k in ed.SEAMS if stride // 2 < k <= stride):
        base = ed.text(n, 1)
        assert base in left and base in right and base[:-1] + ed.flip(base[-1]) in right and ed.flip(base[0]) + base[1:] in right
        inside = [s for s in right if len(s) > n and base in s]
        if stride - n >= 2:
            assert any(s.startswith(base) for s in inside) and any(s.endswith(base) for s in inside)
            assert any(not s.startswith(base) and not s.endswith(base) for s in inside)
        assert any(len(s) < n and s in base for s in right)  # a right string shorter than the left


def test_gpu_saturated_inputs_saturate():
    """``saturated_corpus``: stride 512, a symbol with more than 255 copies in most rows, and the filter's bound holds on
    the saturated rows whatever codes the table assigns (here: two assignments, one with 'a' and 'k' in one bucket)."""
    from napkon_string_matching_amd import tables

    left, right = ed.saturated_corpus()
    assert tables.pick_stride(max(len(s) for s in left + right)) == 512
    assert all(ed.prepared(s) == s for s in left + right)
    assert sum(max(s.count(ch) for ch in set(s)) > 255 for s in left + right) >= 10
    symbols = sorted(set("".join(left + right)))
    for code_of in ({ch: k for k, ch in enumerate(symbols)}, {ch: (0 if ch in "ak" else k + 1) for k, ch in enumerate(symbols)}):
        saturated = attained = 0
        for a in left:
            for b in right:
                ha, hb = ed.hist32(a, code_of), ed.hist32(b, code_of)
                d = ed._dp_fast(a, b, False)
                assert d >= (ed.sad(ha, hb) + 1) // 2
                saturated += 255 in ha or 255 in hb
                attained += d == (ed.sad(ha, hb) + 1) // 2
        assert saturated >= 40 and attained >= 1
    for metric in ed.METRICS:
        scores = [h[0] for h in ed.raw_hits(metric, left, right)]
        assert len(set(scores)) >= 10 and 1.0 in scores


def test_gpu_sharp_inputs_have_no_slack():
    """The pairs of ``sharp_corpus``: the distance is x, the histogram bound is attained, and the start guess of the
    greatest distance is exactly x at the pair's own score -- one lower and the pruned sweep would drop the pair."""
    left, right = ed.sharp_corpus()
    symbols = sorted(set("".join(left + right)))
    assert len(symbols) <= 32
    code_of = {ch: k for k, ch in enumerate(symbols)}  # any assignment below 32 gives every symbol its own bucket
    for k, (n, x) in enumerate(ed.SHARP):
        a, b = left[k], right[k]
        assert len(a) == len(b) == n and ed.distance(a, b) == x == ed.within(a, b)
        assert ed.sad(ed.hist32(a, code_of), ed.hist32(b, code_of)) == 2 * x
        t = ed.score("edit", n, n, x)
        assert ed.most_start("edit", n, n, t) == x == ed.most("edit", n, n, t) and ed.most("edit", n, n, t, start_offset=-1) == x - 1


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("metric", ed.METRICS)
def test_gpu_levels_inputs_hold_every_threshold(metric, wide):
    left, right = ed.levels_corpus(wide)
    assert {len(it) for it in left} == {1, 2, 3, 4} and {len(it) for it in right} >= {1, 2, 3}
    assert max(len(s) for it in left + right for s in it) == (129 if wide else 64) and len(right) <= 64
    assert all(ed.prepared(s) == s for it in left + right for s in it)
    cl, cr = ed.levels_categories(len(left), len(right))
    full = ed.levels_hits(metric, left, right)
    for mode in (0, 1, 2):
        keep = (lambda i, j: True) if mode == 0 else (lambda i, j: ed.category_match(int(cl[i]), int(cr[j]), mode))
        kept = [h for h in full if keep(h[1], h[2])]
        scores = [h[0] for h in kept]
        for t in ed.levels_thresholds(kept):
            assert t in scores and min(scores) < t < max(scores), (mode, t)


# ------------------------------------------------------------------------------------------------------ explicit floors
def test_floor_corpus_records_are_the_definitions():
    """``floor_corpus_records`` (d and w of a pair from one stacked pass) gives the records of ``raw_hits`` / ``levels_hits``,
    the yardsticks of the GPU file."""
    for metric in ed.METRICS:
        assert ed.floor_corpus_records("raw_64", metric) == ed.raw_hits(metric, *ed.floor_corpus("raw_64"))
        assert ed.floor_corpus_records("levels", metric) == ed.levels_hits(metric, *ed.floor_corpus("levels"))
    assert ed.by_caller_id([0.5, 0.25])[[2, 5]].tolist() == [0.5, 0.25] and len(ed.by_caller_id([0.5, 0.25])) == 6


@pytest.mark.parametrize("kind", ed.FLOOR_CORPORA)
@pytest.mark.parametrize("metric", ed.METRICS)
def test_gpu_floor_inputs_sit_on_scores(metric, kind):
    """The explicit floors of tests/test_gpu_edit_distance.py: every floor of an "on" case has a pair of its item exactly
    on it, which the next double up excludes and the next double down keeps; left item ``ABOVE_ALL`` has no record in any
    case; the second-best floors differ from the best ones; the three shifts give different record lists."""
    left, right = ed.floor_corpus(kind)
    records = ed.floor_corpus_records(kind, metric)
    n, m = len(left), len(right)
    assert len(records) == n * m
    kept = {}
    for shift_name, shift in ed.FLOOR_SHIFTS.items():
        for label, lf, rf in ed.floor_cases(records, n, m, shift):
            want = kept[shift_name, label] = ed.floors_plain(records, lf, rf)
            nothing = shift > 0 and label.startswith("rank 0")  # (every floor one double above its item's best score)
            assert len(want) < len(records) and (len(want) == 0) == nothing, (shift_name, label)
            assert lf is None or not any(r[1] == ed.ABOVE_ALL for r in want)
    for label, lf, rf in ed.floor_cases(records, n, m, 0):
        for pos, floors in ((1, lf), (2, rf)):
            for item, floor in enumerate(floors or []):
                if pos == 1 and item == ed.ABOVE_ALL:
                    assert floor > max(r[0] for r in records if r[1] == item)
                    continue
                on = [r for r in records if r[pos] == item and r[0] == floor]
                assert on and all(r[0] < math.nextafter(floor, 2.0) for r in on), (label, pos, item)
        # a record on the floors of both its items is in the "on" and "below" lists and not in the "above" list
        edge = [r for r in kept["on", label] if (lf is not None and r[0] == lf[r[1]]) or (rf is not None and r[0] == rf[r[2]])]
        assert edge and set(edge) <= set(kept["below", label]) and not set(edge) & set(kept["above", label])
        assert len(kept["above", label]) < len(kept["on", label]) <= len(kept["below", label])
    best, second = ed.ranked_floors(records, n, m, 0, 0), ed.ranked_floors(records, n, m, 1, 0)
    assert sum(a > b for a, b in zip(best[0], second[0])) > n // 2 and sum(a > b for a, b in zip(best[1], second[1])) > m // 2
