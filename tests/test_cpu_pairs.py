"""Listed pairs without a GPU: the four ``nsm_*_pairs`` entries' exports and argument checks, ``grid.lookup_pairs`` (the
definition of a pairs query) against a plain-Python recomputation, the seam grids of tests/support/pairs_cases.py through
the oracle alone, and the host faces' device-free checks.

Entry errors: every case ends in host code before the entry's first HIP call -- read off csrc/pairs.hip, not found by
running: ``check_pair_args``, the table checks and the ``n_pairs == 0`` return all precede ``launch_pairs``, the only place
that touches HIP.  A case that expects success therefore has ``n_pairs == 0``; any other successful call would launch.

Host checks: ``plugin.pairs`` validates ``pairs`` and raises the per-pair ``ZeroDivisionError`` before it asks for a device
(compare/score_functions.py); ``ComparableData.score_pairs`` validates its arguments and raises the first listed pair's
``IndexError`` / ``ZeroDivisionError`` before ``_levels_pairs`` (types/comparable_data.py)."""
import random

import numpy as np
import pytest

from support import pairs_cases as pc
from support import threshold_probes as tp
from support.pairs_entry_errors import ENTRIES, call, check_table
from support.top_k_entry_errors import BADARG, FAKE, NULL, OK, UNSUPPORTED

PLAIN = tp.RAW_INDEL + tp.RAW_JACCARD + ["levels_indel_one_word"] + [f"levels_indel_multi_word_{s}" for s in (128, 256, 512)] + \
    ["levels_jaccard"]


# ---------------------------------------------------------------------------------------------------------------- exports
def test_library_exports_the_pairs_entries():
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert lib.nsm_abi_version() == 5 == _lib.ABI_VERSION


# ----------------------------------------------------------------------------------------------------------- entry errors
NULL_ARG = "{who}: null argument"
STRIDE = "{who}: stride %d/%d unsupported (both sides 64, 128, 256 or 512 code units)"
ALPHABET = "{who}: alphabets differ or exceed 255 (%d, %d)"
WIDTH = "{who}: width %d/%d unsupported (both sides 16, 32 or 64)"
PARTITION = "{who}: partitioned tables are not supported (an item must be one row: encode with partition=False)"
ROWS = "{who}: negative row count"
IDS = "{who}: negative id count (%d, %d)"
COLUMN = "{who}: table has a null column"
NONE = dict(n_pairs=0)

COMMON_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    ("pairs null with n_pairs", dict(pairs=False), BADARG, NULL_ARG),
    ("left_row null with left_ids", dict(left_row=None), BADARG, NULL_ARG),
    ("right_row null with right_ids", dict(right_row=None), BADARG, NULL_ARG),
    ("a null table speaks before negative ids", dict(left=NULL, left_ids=-1), BADARG, NULL_ARG),
    ("negative left_ids", dict(left_ids=-1), BADARG, IDS % (-1, 5000)),
    ("negative right_ids", dict(right_ids=-7, right_row=None), BADARG, IDS % (5000, -7)),
    ("negative ids speak before an empty list", dict(left_ids=-1, **NONE), BADARG, IDS % (-1, 5000)),
    ("negative n left", dict(left=dict(n=-1)), BADARG, ROWS),
    ("negative n right", dict(right=dict(n=-3), **NONE), BADARG, ROWS),
    ("negative ids speak before a negative n", dict(left=dict(n=-1), right_ids=-1), BADARG, IDS % (5000, -1)),
    # n_pairs == 0: no launch, whatever the list pointer; row maps may be null when no id is mapped
    ("empty list", NONE, OK, None),
    ("empty list, null pairs", dict(pairs=False, **NONE), OK, None),
    ("empty list, null row maps without ids", dict(left_row=None, left_ids=0, right_row=None, right_ids=0, **NONE), OK, None),
    ("empty list, empty tables", dict(left=dict(n=0), right=dict(n=0), **NONE), OK, None),
]

STRING_CASES = lambda key: [
    ("stride 64 vs 128", {key[1]: dict(stride=128)}, UNSUPPORTED, STRIDE % (64, 128)),
    ("stride 96", {key[0]: dict(stride=96), key[1]: dict(stride=96)}, UNSUPPORTED, STRIDE % (96, 96)),
    ("stride 96 on an empty list", {key[0]: dict(stride=96), key[1]: dict(stride=96), **NONE}, UNSUPPORTED, STRIDE % (96, 96)),
    ("alphabets differ", {key[1]: dict(alphabet=11)}, BADARG, ALPHABET % (10, 11)),
    ("alphabet 0", {key[0]: dict(alphabet=0), key[1]: dict(alphabet=0)}, BADARG, ALPHABET % (0, 0)),
    ("alphabet 256", {key[0]: dict(alphabet=256), key[1]: dict(alphabet=256)}, BADARG, ALPHABET % (256, 256)),
    ("stride and alphabet: the stride speaks first", {key[0]: dict(stride=96, alphabet=0)}, UNSUPPORTED, STRIDE % (96, 64)),
    ("negative ids speak before the stride", {key[0]: dict(stride=96), "left_ids": -1}, BADARG, IDS % (-1, 5000)),
    ("alphabet before negative n", {key[0]: dict(alphabet=0, n=-1)}, BADARG, ALPHABET % (0, 10)),
    ("codes null", {key[0]: dict(codes=None)}, BADARG, COLUMN),
    ("len null on the right", {key[1]: dict(len=None)}, BADARG, COLUMN),
    ("columns the entry does not read may be null", {key[0]: dict(orig=None, len_start=None), key[1]: dict(orig=None, len_start=None),
                                                      **NONE}, OK, None),
]

INDEL_RAW_CASES = COMMON_CASES + STRING_CASES(("left", "right")) + [
    ("a table without rows may lack its columns", dict(left=dict(n=0, codes=None, len=None), **NONE), OK, None),
]

SEG = dict(seg=FAKE, seg_start=FAKE)
INDEL_LEVELS_CASES = COMMON_CASES + STRING_CASES(("left_strings", "right_strings")) + [
    ("left_strings null", dict(left_strings=NULL), BADARG, NULL_ARG),
    ("right_strings null", dict(right_strings=NULL), BADARG, NULL_ARG),
    ("partitioned left", dict(left=SEG), UNSUPPORTED, PARTITION),
    ("seg_start alone on the right", dict(right=dict(seg_start=FAKE)), UNSUPPORTED, PARTITION),
    ("alphabet before the partition", dict(left=SEG, right_strings=dict(alphabet=11)), BADARG, ALPHABET % (10, 11)),
    ("partition before negative n", dict(left=dict(n=-1, **SEG)), UNSUPPORTED, PARTITION),
    ("negative string rows", dict(left_strings=dict(n=-1)), BADARG, ROWS),
    ("first null", dict(left=dict(first=None)), BADARG, COLUMN),
    ("nlev null on the right", dict(right=dict(nlev=None)), BADARG, COLUMN),
    ("items without rows may lack their columns", dict(left=dict(n=0, first=None, nlev=None, orig=None),
                                                        left_strings=dict(codes=None, len=None), **NONE), OK, None),
]

SET_CASES = [
    ("widths differ", dict(right=dict(width=32)), BADARG, WIDTH % (16, 32)),
    ("width 48", dict(left=dict(width=48), right=dict(width=48)), BADARG, WIDTH % (48, 48)),
    ("width 48 on an empty list", dict(left=dict(width=48), right=dict(width=48), **NONE), BADARG, WIDTH % (48, 48)),
    ("negative ids speak before the width", dict(right=dict(width=32), right_ids=-1), BADARG, IDS % (5000, -1)),
    ("partitioned left", dict(left=SEG), UNSUPPORTED, PARTITION),
    ("seg alone on the right", dict(right=dict(seg=FAKE)), UNSUPPORTED, PARTITION),
    ("width before the partition", dict(left=dict(width=48, **SEG)), BADARG, WIDTH % (48, 16)),
    ("partition before negative n", dict(right=dict(n=-1, **SEG)), UNSUPPORTED, PARTITION),
    ("ids null", dict(left=dict(ids=None)), BADARG, COLUMN),
    ("cnt null on the right", dict(right=dict(cnt=None)), BADARG, COLUMN),
    ("a table without rows may lack its columns", dict(right=dict(n=0, ids=None, cnt=None, orig=None, size_start=None), **NONE),
     OK, None),
]

JACCARD_RAW_CASES = COMMON_CASES + SET_CASES + [
    ("a RAW table carries no levels", dict(left=dict(nlev=None, plen=None, max_levels=0),
                                           right=dict(nlev=None, plen=None, max_levels=0), **NONE), OK, None),
]

LEVELS = "{who}: levels tables need nlev and plen"
JACCARD_LEVELS_CASES = COMMON_CASES + SET_CASES + [
    ("nlev null", dict(left=dict(nlev=None)), BADARG, LEVELS),
    ("plen null on the right", dict(right=dict(plen=None)), BADARG, LEVELS),
    ("max_levels 0", dict(right=dict(max_levels=0)), BADARG, LEVELS),
    ("levels columns are asked for even on an empty table and list", dict(left=dict(n=0, nlev=None), **NONE), BADARG, LEVELS),
    ("partition before the levels columns", dict(left=dict(nlev=None, **SEG)), UNSUPPORTED, PARTITION),
    ("levels columns before negative n", dict(left=dict(n=-1, plen=None)), BADARG, LEVELS),
]

CASES = {"nsm_indel_raw_pairs": INDEL_RAW_CASES, "nsm_jaccard_raw_pairs": JACCARD_RAW_CASES,
         "nsm_indel_levels_pairs": INDEL_LEVELS_CASES, "nsm_jaccard_levels_pairs": JACCARD_LEVELS_CASES}


@pytest.mark.parametrize("entry", ENTRIES)
def test_pairs_entry_answers(entry):
    check_table(entry, CASES[entry])


def test_every_case_is_an_error_or_an_empty_list():
    """A table entry that expects success must have ``n_pairs == 0``: any other successful call would have launched."""
    for cases in CASES.values():
        for label, kw, status, message in cases:
            if status == OK:
                assert message is None and kw.get("n_pairs") == 0, label
            else:
                assert status in (BADARG, UNSUPPORTED) and message, label


def test_an_error_leaves_the_message_of_its_own_entry():
    assert call("nsm_jaccard_raw_pairs", left=NULL) == (BADARG, "nsm_jaccard_raw_pairs: null argument")
    assert call("nsm_indel_levels_pairs", pairs=False) == (BADARG, "nsm_indel_levels_pairs: null argument")


# ----------------------------------------------------------------------------------------------------------- lookup_pairs
def _sample(g, n, seed):
    rng = random.Random(seed)
    return [(rng.randrange(len(g.left)), rng.randrange(len(g.right))) for _ in range(n)]


@pytest.mark.parametrize("name", PLAIN)
def test_lookup_pairs_equals_a_plain_python_recomputation(name):
    """500 seeded pairs of every plain probe grid: the oracle's score picked by ``lookup_pairs`` is the score recomputed
    with an O(nm) LCS table, Python sets and the levels sum.  (RAW Jaccard: the grids hold no empty set on the left.)"""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    pairs = _sample(g, 500, 4100 + len(name))
    i, j = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    got = grid.lookup_pairs(tp.all_scores(g), i, j)
    want = np.array([pc.pair_score(g, a, b) for a, b in pairs])
    assert got.dtype == np.float64 and np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5])


def test_lookup_pairs_absent_duplicates_and_order():
    from napkon_string_matching_amd import grid

    hits = grid.Hits(np.array([0.9, 0.5, 0.25]), np.array([2, 0, 7], dtype=np.int32), np.array([1, 3, 7], dtype=np.int32))
    i, j = [7, 0, 2, 0, 5, 2, -1, 1 << 40, 0], [7, 3, 1, 3, 5, 2, 3, 3, -2]
    want = [0.25, 0.5, 0.9, 0.5, -1.0, -1.0, -1.0, -1.0, -1.0]
    assert grid.lookup_pairs(hits, i, j).tolist() == want
    # the same from records in any order, and from nothing
    assert grid.lookup_pairs([(0.5, 0, 3), (0.25, 7, 7), (0.9, 2, 1)], i, j).tolist() == want
    assert grid.lookup_pairs([], i, j).tolist() == [-1.0] * len(i)
    assert grid.lookup_pairs(hits, [], []).shape == (0,)
    with pytest.raises(ValueError):
        grid.lookup_pairs(hits, [1, 2], [1])
    with pytest.raises(ValueError):
        grid.lookup_pairs(hits, [1.5], [1])
    with pytest.raises(ValueError):
        grid.lookup_pairs(hits, [[1]], [[1]])


def test_pairs_wrappers_refuse_bad_id_columns_before_any_device_work():
    """``check_pair_ids`` is the first statement of every wrapper: the tables are not touched."""
    from napkon_string_matching_amd import grid

    for fn, tabs in ((grid.indel_raw_pairs, (None, None)), (grid.jaccard_raw_pairs, (None, None)),
                     (grid.indel_levels_pairs, (None, None, None, None)), (grid.jaccard_levels_pairs, (None, None))):
        with pytest.raises(ValueError, match="2 left ids for 1 right ids"):
            fn(*tabs, [1, 2], [1])
        with pytest.raises(ValueError, match="integer"):
            fn(*tabs, [0.5], [1])


# ------------------------------------------------------------------------------------------------------------- seam grids
@pytest.mark.parametrize("name", pc.EVERY)
def test_seam_grids_through_the_oracle(name):
    """Every pair of every seam grid: the oracle agrees with the plain-Python recomputation, and no pair is missing (the
    grids hold no pair the oracle would raise for)."""
    from napkon_string_matching_amd import grid

    g = pc.grid(name)
    pairs = [(i, j) for i in range(len(g.left)) for j in range(len(g.right))]
    if len(pairs) > 600:  # (the O(nm) tables of 512-unit strings are slow in Python: a seeded sample, the planted pairs kept)
        pairs = random.Random(5).sample(pairs, 600)
    i, j = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    got = grid.lookup_pairs(tp.all_scores(g), i, j)
    short = [k for k, (a, b) in enumerate(pairs) if g.raw is False or len(g.left[a]) * len(g.right[b]) <= 20000]
    assert (got >= 0.0).all(), name
    assert [got[k] for k in short] == [pc.pair_score(g, *pairs[k]) for k in short], name


@pytest.mark.parametrize("stride", pc.STRIDES)
def test_indel_seam_grids_hold_what_they_claim(stride):
    from napkon_string_matching_amd import tables

    g = pc.indel_seams(stride)
    assert tables.pick_stride(max(len(s) for s in g.left + g.right)) == stride
    assert {len(s) for s in g.left} >= {n for n in pc.LENGTHS if n <= stride} <= {len(s) for s in g.right}
    for i, j in g.self_pairs:
        assert g.left[i] == g.right[j]
    i, j, lcs = g.straddle
    assert pc.lcs(g.left[i], g.right[j]) == lcs == len(pc.straddle_positions(stride)) == 2 * (stride // 64) - 1
    assert all(p % 64 in (63, 0) for p in pc.straddle_positions(stride))
    for i, j, lcs in g.runs:
        assert len(set(g.left[i]) | set(g.right[j])) == 1 and abs(len(g.left[i]) - len(g.right[j])) == 1
        assert min(len(g.left[i]), len(g.right[j])) == lcs == stride - 1


def test_set_and_levels_seam_grids_hold_what_they_claim():
    for w in (16, 32, 64):
        g = pc.jaccard_seams(w)
        assert {len(r) for r in g.right} >= {0, 1, w} and {len(r) for r in g.left} >= {1, w} and all(g.left)
        scores = {pc.jaccard(a, b) for a in g.left for b in g.right}
        assert {0.0, 1.0, 0.5} <= scores  # disjoint, equal, nested (half of the other)
    for kind in ("indel", "jaccard"):
        g = pc.levels_seams(kind)
        depths = lambda side: {len(it) for it in side}
        assert depths(g.left) == depths(g.right) == set(pc.DEPTHS)
    for w in (32, 64):
        g = pc.levels_jaccard_wide(w)
        assert (len(g.left[0]), len(g.right[0]), len(g.left[1]), len(g.right[1])) == (64, 1, 1, 64)
        assert max(len(it[-1]) for it in g.left + g.right) == w and all(lv for it in g.left + g.right for lv in it)


# -------------------------------------------------------------------------------------------------------------- host faces
def test_plugin_pairs_argument_errors_need_no_device():
    from napkon_string_matching_amd.compare import score_functions as sf

    for plugin in (sf.fuzzy_match, sf.intersection_vs_union):
        with pytest.raises(ValueError):
            plugin.pairs(["a b"], ["a"], [(0, 0, 0)])       # not (i, j)
        with pytest.raises(ValueError):
            plugin.pairs(["a b"], ["a"], [(0.0, 0.0)])      # not integers
        with pytest.raises(ValueError):
            plugin.pairs(["a b"], ["a"], [0, 0])            # one-dimensional
        with pytest.raises(IndexError):
            plugin.pairs(["a b"], ["a"], [(0, 1)])          # no such right item
        with pytest.raises(IndexError):
            plugin.pairs(["a b"], ["a"], np.array([[-1, 0]]))
        assert plugin.pairs(["a b"], ["a"], []).shape == (0,)
    # a listed pair of two empty sets: the plugin's ZeroDivisionError, whatever else the lists hold; unlisted pairs do not count
    with pytest.raises(ZeroDivisionError, match="division by zero"):
        sf.intersection_vs_union.pairs(["a", ""], ["b", []], [(0, 0), (1, 1)])
    assert sf.intersection_vs_union.pairs(["a", ""], ["b", []], np.zeros((0, 2), dtype=np.int64)).shape == (0,)


def _frames():
    import pandas as pd

    from napkon_string_matching_amd.types.comparable_data import ComparableData

    left = ComparableData(pd.DataFrame({"Identifier": ["l0", "l1", "l2"], "Term": [["fever"], ["none"], ["blank"]],
                                        "Tokens": [["fever high"], [], [""]]}))
    right = ComparableData(pd.DataFrame({"Identifier": ["r0", "r1", "r2"], "Term": [["fever"], ["none"], ["blank"]],
                                         "Tokens": [["high fever"], [], [""]]}))
    return left, right


def test_score_pairs_argument_errors_need_no_device():
    from napkon_string_matching_amd.types.mapping import Mapping

    left, right = _frames()
    kw = dict(compare_column="Tokens", score_func="intersection_vs_union", left_name="hap", right_name="pop")
    with pytest.raises(ValueError):
        left.score_pairs(right, [("l0",)], **kw)                       # not a pair
    with pytest.raises(ValueError):
        left.score_pairs(right, "l0", **kw)                            # not a list of pairs
    with pytest.raises(ValueError, match="left_name and right_name"):
        left.score_pairs(right, Mapping({"u": {"hap": ["l0"], "pop": ["r0"]}}), compare_column="Tokens",
                         score_func="intersection_vs_union")
    with pytest.raises(AttributeError):
        left.score_pairs(right, [("l0", "r0")], **dict(kw, score_func="no_such_function"))


def test_score_pairs_raises_for_the_first_listed_pair_that_compare_terms_would_raise_for():
    left, right = _frames()
    kw = dict(compare_column="Tokens", left_name="hap", right_name="pop")
    # (l1 and r1 have no levels; the only level of l2 and of r2 is an empty set)
    with pytest.raises(IndexError, match="list index out of range"):
        left.score_pairs(right, [("l1", "r0")], score_func="intersection_vs_union", **kw)
    with pytest.raises(IndexError, match="list index out of range"):
        left.score_pairs(right, [("l0", "r1")], score_func="fuzzy_match", **kw)
    with pytest.raises(ZeroDivisionError, match="division by zero"):
        left.score_pairs(right, [("l2", "r2")], score_func="intersection_vs_union", **kw)
    # the FIRST listed raising pair decides, unknown identifiers and level-less pairs before it do not
    with pytest.raises(ZeroDivisionError):
        left.score_pairs(right, [("nobody", "r0"), ("l1", "r1"), ("l2", "r2"), ("l1", "r0")], score_func="intersection_vs_union", **kw)
    with pytest.raises(IndexError):
        left.score_pairs(right, [("l1", "r1"), ("l1", "r0"), ("l2", "r2")], score_func="intersection_vs_union", **kw)


def test_score_pairs_without_a_scorable_pair_needs_no_device():
    """Two level-less items score 0, an unknown identifier gives NaN; neither reaches the device."""
    left, right = _frames()
    out = left.score_pairs(right, [("l1", "r1"), ("nobody", "r0"), ("l0", "nobody")], compare_column="Tokens",
                           score_func="fuzzy_match", left_name="hap", right_name="pop")
    score = out.dataframe()["MatchScore"].to_numpy()
    assert len(out) == 3 and score[0] == 0.0 and np.isnan(score[1]) and np.isnan(score[2])
    assert out.dataframe()["HapIdentifier"].tolist() == ["l1", "nobody", "l0"]
    assert out.dataframe()["PopIdentifier"].tolist() == ["r1", "r0", "nobody"]
