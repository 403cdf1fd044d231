"""Best-match queries and floor grids: what is decided without a device.

* ``grid.best_of_hits`` / ``grid.filter_by_floors`` against the plain-Python restatement of tests/support/best_matches.py on
  the oracle's hit lists of every probe grid;
* the preconditions tests/test_gpu_best.py relies on, asserted on the oracle alone;
* argument checks that come before any device work, and the error surface of the four ``nsm_*_floor_grid`` entries: status,
  exact ``nsm_last_error()`` text, and which check speaks first.  Every case ends in host code before the entry's first HIP
  call -- read off the entries (csrc/floors_raw.hip, floors_levels.hip: null arguments, row counts, an empty side, then the
  table checks of top_k_lists.hpp; the first HIP call comes after all of them)."""
import math

import numpy as np
import pandas as pd
import pytest

from support import best_matches as bm
from support import threshold_probes as tp
from support.top_k_entry_errors import BADARG, FAKE, NULL, OK, UNSUPPORTED


def _cuts(g):
    """Thresholds the lists are cut at: 0.0 and two probes (a low and a middle one)."""
    probes = tp.probes_of(g)
    return [0.0, probes[len(probes) // 4], probes[len(probes) // 2]]


# ------------------------------------------------------------------------------------------------------ definitions
@pytest.mark.parametrize("name", tp.EVERY)
def test_best_of_hits_and_filter_by_floors_against_plain_python(name):
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    everything = tp.all_scores(g)
    gap = bm.row_gap(everything)
    assert gap > 0.0
    for thr in _cuts(g):
        records = tp.expectation(everything, thr)
        hits = bm.to_hits(records)
        for margin in (0.0, gap, 2.0):
            for mutual in (False, True):
                got = grid.best_of_hits(hits, margin, mutual, len(g.left), len(g.right))
                assert got.as_tuples() == bm.best_plain(records, margin, mutual), (name, thr, margin, mutual)
        # floors: every item's own best; the left items at a probe one ulp above it; NaN and -inf on either side
        s = records[len(records) // 2][0]
        for floor in (math.nextafter(s, 0.0), s, math.nextafter(s, 2.0)):
            left, right = bm.probe_floors(records, s, floor, len(g.left), len(g.right))
            for lf, rf in ((left, None), (None, right), (left, right), (None, None)):
                got = grid.filter_by_floors(hits, None if lf is None else np.array(lf), None if rf is None else np.array(rf))
                assert got.as_tuples() == bm.floors_plain(records, lf, rf), (name, thr, floor)


@pytest.mark.parametrize("name", tp.EVERY)
def test_properties(name):
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    for thr in _cuts(g):
        records = tp.expectation(tp.all_scores(g), thr)
        hits = bm.to_hits(records)
        assert grid.best_of_hits(hits, 2.0).as_tuples() == records                       # a margin beyond every score
        assert grid.best_of_hits(hits, 2.0, mutual=True).as_tuples() == records
        for margin in (0.0, bm.row_gap(tp.all_scores(g))):
            one, both = grid.best_of_hits(hits, margin).as_tuples(), grid.best_of_hits(hits, margin, mutual=True).as_tuples()
            assert set(both) <= set(one) <= set(records)
        lb, rb = bm.bests(records)
        exact = grid.best_of_hits(hits, 0.0).as_tuples()
        assert all(s == lb[i] for s, i, _ in exact) and {i for _, i, _ in exact} == set(lb)
        # mutual best at margin 0 does not depend on which side is called left
        swapped = bm.to_hits([(s, j, i) for s, i, j in records])
        back = grid.best_of_hits(swapped, 0.0, mutual=True)
        assert sorted((s, j, i) for s, i, j in back.as_tuples()) == sorted(grid.best_of_hits(hits, 0.0, mutual=True).as_tuples())


@pytest.mark.parametrize("name", tp.EVERY)
def test_preconditions_of_the_gpu_file(name):
    """Ties at the top are the rule on the probe grids, and mutual best is a proper, non-empty restriction."""
    records = tp.all_scores(tp.grid(name))
    lb, _ = bm.bests(records)
    at_best = {}
    for s, i, _ in records:
        if s == lb[i]:
            at_best[i] = at_best.get(i, 0) + 1
    assert sum(1 for n in at_best.values() if n >= 2) >= 5
    one, both = bm.best_plain(records, 0.0, False), bm.best_plain(records, 0.0, True)
    assert 0 < len(both) < len(one)


# ------------------------------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("margin", [-0.1, -1, math.nan, math.inf, -math.inf, "0.1", None, True, [0.1]])
def test_check_margin_refuses(margin):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    with pytest.raises(ValueError):
        grid.check_margin(margin)
    with pytest.raises(ValueError):
        grid.best_of_hits(bm.to_hits([(1.0, 0, 0)]), margin)
    for plugin in (fuzzy_match, intersection_vs_union):  # before any device work
        with pytest.raises(ValueError):
            plugin.best(["a b"], ["a c"], margin=margin)


def test_check_margin_accepts():
    from napkon_string_matching_amd import grid

    assert grid.check_margin(0) == 0.0 and grid.check_margin(0.25) == 0.25 and grid.check_margin(np.float64(2)) == 2.0


COLUMNS = ["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"]
KW = dict(score_func="fuzzy_match", compare_column="Tokens", left_name="hap", right_name="pop", score_threshold=0.2)


def _cohort(prefix, n, categories=None):
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    rows = [[f"{prefix}{k}", f"v{k}", "s", categories[k] if categories else [f"c{k % 3}"], [f"word{k % 7} w{k % 5}"],
             [f"word{k % 7}", f"w{k % 5}"], "p"] for k in range(n)]
    return Questionnaire(pd.DataFrame(rows, columns=COLUMNS))


def test_compare_refuses_bad_combinations_before_device_work():
    left, right = _cohort("a", 4), _cohort("b", 5)
    for call in (left.compare, left.gen_comparable):
        with pytest.raises(ValueError):
            call(right, None, None, best_margin=0.0, top_k=3, **KW)
        with pytest.raises(ValueError):
            call(right, None, None, mutual_best=True, **KW)
        with pytest.raises(ValueError):
            call(right, None, None, best_margin=-0.5, **KW)
        with pytest.raises(ValueError):
            call(right, None, None, best_margin=math.nan, mutual_best=True, **KW)


def test_more_than_64_category_labels_raise_before_device_work():
    labels = [[f"c{k}", f"d{k}"] for k in range(40)]
    left, right = _cohort("a", 40, labels), _cohort("b", 40, labels)
    with pytest.raises(NotImplementedError):
        left.compare(right, None, None, best_margin=0.0, filter_categories=True, **KW)


def test_cache_key_unchanged_without_best_margin_and_distinct_with_it():
    left, right = _cohort("a", 4), _cohort("b", 5)
    kwargs = {k: v for k, v in KW.items() if k not in ("compare_column", "score_threshold")}
    key = lambda *a, **kw: left._hash_compare_args(right, None, None, "Tokens", 0.2, kwargs, *a, **kw)
    plain = key()
    assert key(None, None, False) == plain and key(best_margin=None, mutual_best=False) == plain
    keys = [plain, key(3), key(best_margin=0.0), key(best_margin=0.0, mutual_best=True), key(best_margin=0.1)]
    assert len(set(keys)) == len(keys)


# -------------------------------------------------------------------------------------- the entries' error surface
def test_symbols_exported_and_declared():
    from napkon_string_matching_amd import _lib

    assert set(bm.ENTRIES) <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert lib.nsm_abi_version() == 5
    for name in bm.ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (11 if "_raw_" in name else 16 if "indel" in name else 14), name


NULL_ARG = "{who}: null argument"
ROWS = "{who}: negative row count"
EMPTY = dict(n=0)
OUT_CASES = [
    ("hit_count null", dict(hit_count=False), BADARG, NULL_ARG),
    ("hits null with capacity", dict(hits=False, capacity=1), BADARG, NULL_ARG),
    ("hits null without capacity, empty side", dict(hits=False, capacity=0, right=EMPTY), OK, None),
    ("negative n left", dict(left=dict(n=-1)), BADARG, ROWS),
    ("negative n right", dict(right=dict(n=-3)), BADARG, ROWS),
    ("negative n before empty side", dict(left=EMPTY, right=dict(n=-1)), BADARG, ROWS),
    ("null hit_count before negative n", dict(hit_count=False, left=dict(n=-1)), BADARG, NULL_ARG),
]


def _null_columns(message, left_columns, right_columns, key=("left", "right")):
    return [(f"{side} {col} null", {side_key: {col: None}}, BADARG, message)
            for side, side_key, cols in (("left", key[0], left_columns), ("right", key[1], right_columns)) for col in cols]


STRIDES_DIFFER = "{who}: strides differ (%d, %d)"
STRIDE = "{who}: stride %d unsupported (64, 128, 256 or 512 code units)"
ALPHABET = "{who}: alphabets differ or exceed 255 (%d, %d)"
RAW_STR_COLUMN = "{who}: table has a null column (the right table needs len_start)"
INDEL_RAW_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    *OUT_CASES,
    ("empty left: null columns", dict(left=dict(n=0, codes=None, len=None, orig=None)), OK, None),
    ("empty right: null columns and a stride fault", dict(right=dict(n=0, codes=None, len_start=None, stride=96)), OK, None),
    ("stride 64 vs 128", dict(right=dict(stride=128)), BADARG, STRIDES_DIFFER % (64, 128)),
    ("stride 96", dict(left=dict(stride=96), right=dict(stride=96)), UNSUPPORTED, STRIDE % 96),
    ("alphabets differ", dict(right=dict(alphabet=11)), BADARG, ALPHABET % (10, 11)),
    ("alphabet 0", dict(left=dict(alphabet=0), right=dict(alphabet=0)), BADARG, ALPHABET % (0, 0)),
    ("alphabet 256", dict(left=dict(alphabet=256), right=dict(alphabet=256)), BADARG, ALPHABET % (256, 256)),
    ("stride and alphabet: the stride speaks first", dict(left=dict(stride=96, alphabet=0), right=dict(stride=96)), UNSUPPORTED,
     STRIDE % 96),
    ("negative n before the stride", dict(left=dict(n=-1, stride=96)), BADARG, ROWS),
    ("stride before null columns", dict(left=dict(stride=128, codes=None)), BADARG, STRIDES_DIFFER % (128, 64)),
    *_null_columns(RAW_STR_COLUMN, ("codes", "len", "orig"), ("codes", "len_start", "orig")),
]

WIDTH = "{who}: width %d/%d unsupported (both sides 16, 32 or 64)"
RAW_SET_COLUMN = "{who}: table has a null column (the right table needs size_start)"
JACCARD_RAW_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    *OUT_CASES,
    ("empty left: null columns", dict(left=dict(n=0, ids=None, cnt=None, orig=None)), OK, None),
    ("empty right: null columns and a width fault", dict(right=dict(n=0, ids=None, size_start=None, width=48)), OK, None),
    ("widths differ", dict(right=dict(width=32)), BADARG, WIDTH % (16, 32)),
    ("width 48", dict(left=dict(width=48), right=dict(width=48)), BADARG, WIDTH % (48, 48)),
    ("negative n before the width", dict(left=dict(n=-1), right=dict(width=32)), BADARG, ROWS),
    ("width before null columns", dict(left=dict(ids=None), right=dict(width=32)), BADARG, WIDTH % (16, 32)),
    *_null_columns(RAW_SET_COLUMN, ("ids", "cnt", "orig"), ("ids", "size_start", "orig")),
]

PARTITION_ITEMS = "{who}: partitioned item tables are not supported (an item must be one row: encode with partition=False)"
PARTITION_SETS = "{who}: partitioned tables are not supported (an item must be one row: encode with partition=False)"
MODE = "{who}: unknown category_mode %d"
NEEDS_CAT = "{who}: a category predicate needs `cat` on both sides"
BANNED = "{who}: banned_start and banned_j go together"
LEVELS_COLUMN = "{who}: table has a null column"
INDEL_LEVELS_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    ("left_strings null", dict(left_strings=NULL), BADARG, NULL_ARG),
    ("right_strings null", dict(right_strings=NULL), BADARG, NULL_ARG),
    *OUT_CASES,
    ("empty left: null columns, half a partition", dict(left=dict(n=0, first=None, nlev=None, orig=None, seg=FAKE)), OK, None),
    ("empty right: null columns, unknown category mode", dict(right=dict(n=0, first=None), category_mode=7), OK, None),
    ("stride 64 vs 128", dict(right_strings=dict(stride=128)), BADARG, STRIDES_DIFFER % (64, 128)),
    ("stride 96", dict(left_strings=dict(stride=96), right_strings=dict(stride=96)), UNSUPPORTED, STRIDE % 96),
    ("alphabets differ", dict(right_strings=dict(alphabet=11)), BADARG, ALPHABET % (10, 11)),
    ("alphabet 256", dict(left_strings=dict(alphabet=256), right_strings=dict(alphabet=256)), BADARG, ALPHABET % (256, 256)),
    ("partitioned left", dict(left=dict(seg=FAKE, seg_start=FAKE, cat=FAKE), category_mode=1), UNSUPPORTED, PARTITION_ITEMS),
    ("seg_start on the right alone", dict(right=dict(seg_start=FAKE)), UNSUPPORTED, PARTITION_ITEMS),
    ("stride before the partition", dict(left=dict(seg=FAKE), right_strings=dict(stride=128)), BADARG, STRIDES_DIFFER % (64, 128)),
    ("partition before null columns", dict(left=dict(seg=FAKE, first=None)), UNSUPPORTED, PARTITION_ITEMS),
    *_null_columns(LEVELS_COLUMN, ("first", "nlev", "orig"), ("first", "nlev", "orig")),
    *_null_columns(LEVELS_COLUMN, ("codes", "len"), ("codes", "len"), key=("left_strings", "right_strings")),
    ("category mode 7", dict(category_mode=7), BADARG, MODE % 7),
    ("null column before category mode", dict(category_mode=7, left=dict(nlev=None)), BADARG, LEVELS_COLUMN),
    ("cat missing on the left under a category mode", dict(right=dict(cat=FAKE), category_mode=1), BADARG, NEEDS_CAT),
    ("cat missing on the right under a category mode", dict(left=dict(cat=FAKE), category_mode=2), BADARG, NEEDS_CAT),
    ("banned_start without banned_j", dict(banned=(FAKE, None)), BADARG, BANNED),
    ("banned_j without banned_start", dict(banned=(None, FAKE)), BADARG, BANNED),
    ("category mode before the blacklist", dict(category_mode=7, banned=(FAKE, None)), BADARG, MODE % 7),
]

SETS_COLUMN = "{who}: table has a null column (levels tables need nlev and plen)"
JACCARD_LEVELS_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    *OUT_CASES,
    ("empty left: null columns, half a partition", dict(left=dict(n=0, ids=None, nlev=None, seg=FAKE)), OK, None),
    ("empty right: null columns, unknown category mode", dict(right=dict(n=0, plen=None), category_mode=7), OK, None),
    ("widths differ", dict(right=dict(width=32)), BADARG, WIDTH % (16, 32)),
    ("width 48", dict(left=dict(width=48), right=dict(width=48)), BADARG, WIDTH % (48, 48)),
    ("partitioned left", dict(left=dict(seg=FAKE, seg_start=FAKE, cat=FAKE), category_mode=1), UNSUPPORTED, PARTITION_SETS),
    ("seg on the right alone", dict(right=dict(seg=FAKE)), UNSUPPORTED, PARTITION_SETS),
    ("width before the partition", dict(left=dict(seg=FAKE), right=dict(width=32)), BADARG, WIDTH % (16, 32)),
    ("partition before null columns", dict(left=dict(seg=FAKE, ids=None)), UNSUPPORTED, PARTITION_SETS),
    *_null_columns(SETS_COLUMN, ("ids", "cnt", "nlev", "plen", "orig"), ("ids", "cnt", "nlev", "plen", "orig")),
    ("max_levels 0", dict(left=dict(max_levels=0)), BADARG, SETS_COLUMN),
    ("category mode 7", dict(category_mode=7), BADARG, MODE % 7),
    ("cat missing on the left under a category mode", dict(right=dict(cat=FAKE), category_mode=1), BADARG, NEEDS_CAT),
    ("banned_start without banned_j", dict(banned=(FAKE, None)), BADARG, BANNED),
]

CASES = dict(zip(bm.ENTRIES, (INDEL_RAW_CASES, JACCARD_RAW_CASES, INDEL_LEVELS_CASES, JACCARD_LEVELS_CASES)))


@pytest.mark.parametrize("entry", bm.ENTRIES)
def test_floor_grid_entries_answer_malformed_calls(entry):
    bm.check_table(entry, CASES[entry])


def test_every_case_is_an_error_or_an_empty_side():
    """A table entry that expects success must have an empty side: any other successful call would have launched."""
    for cases in CASES.values():
        for label, kw, status, message in cases:
            if status == OK:
                assert message is None and any((kw.get(side) or {}).get("n") == 0 for side in ("left", "right")), label
            else:
                assert status in (BADARG, UNSUPPORTED) and message, label
