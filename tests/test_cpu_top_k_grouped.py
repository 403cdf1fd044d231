"""Grouped top-k of the RAW grids (one record per group of right rows): what is decided before any device work."""
import ctypes

import numpy as np
import pytest

from support.grouped import group_cut
from support.top_k_entry_errors import NULL, check_table

BADARG = 10001


def test_c_entries_reject_bad_arguments_without_touching_the_device():
    from napkon_string_matching_amd import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("libnsm_hip.so not built")
    lib = _lib.load()
    cnt = ctypes.c_ulonglong(0)
    hit = _lib.NsmHit()
    grp = (ctypes.c_int32 * 3)(0, 1, 2)
    out, pc, pg = ctypes.addressof(hit), ctypes.addressof(cnt), ctypes.addressof(grp)
    s = _lib.NsmStrTable(None, None, None, None, None, 3, 64, 10)
    a = _lib.NsmSetTable(None, None, None, None, None, None, None, None, None, None, None, None, 3, 16, 0)
    for k in (0, -1):
        rc = lib.nsm_indel_raw_top_k_grouped(s, s, pg, 0.5, k, _lib.FLAG_PRUNE, out, pc, None, None)
        assert rc == BADARG and b"k" in lib.nsm_last_error()
        rc = lib.nsm_jaccard_raw_top_k_grouped(a, a, pg, 0.5, k, _lib.FLAG_PRUNE, out, pc, None, None)
        assert rc == BADARG and b"k" in lib.nsm_last_error()
    # no group column
    rc = lib.nsm_indel_raw_top_k_grouped(s, s, None, 0.5, 1, 0, out, pc, None, None)
    assert rc == BADARG and b"right_group" in lib.nsm_last_error()
    rc = lib.nsm_jaccard_raw_top_k_grouped(a, a, None, 0.5, 1, 0, out, pc, None, None)
    assert rc == BADARG and b"right_group" in lib.nsm_last_error()
    # width / stride mismatch and a right table without its class starts, as for the ungrouped entries
    b = _lib.NsmSetTable(None, None, None, None, None, None, None, None, None, None, None, None, 3, 32, 0)
    rc = lib.nsm_jaccard_raw_top_k_grouped(a, b, pg, 0.5, 1, 0, out, pc, None, None)
    assert rc == BADARG and b"width" in lib.nsm_last_error()
    s2 = _lib.NsmStrTable(None, None, None, None, None, 3, 128, 10)
    rc = lib.nsm_indel_raw_top_k_grouped(s, s2, pg, 0.5, 1, 0, out, pc, None, None)
    assert rc == BADARG and b"stride" in lib.nsm_last_error()
    rc = lib.nsm_indel_raw_top_k_grouped(s, s, pg, 0.5, 1, 0, out, pc, None, None)
    assert rc == BADARG and b"len_start" in lib.nsm_last_error()
    rc = lib.nsm_jaccard_raw_top_k_grouped(a, a, pg, 0.5, 1, 0, out, pc, None, None)
    assert rc == BADARG and b"size_start" in lib.nsm_last_error()
    assert b"_grouped" in lib.nsm_last_error()
    assert cnt.value == 0


def _hits_with_ties():
    from napkon_string_matching_amd import grid

    # (score, i, j); groups below put equal scores inside one group (j 1, 3) and across groups (j 3, 4 / j 0, 6)
    recs = [(0.9, 0, 4), (0.9, 0, 3), (0.9, 0, 1), (0.5, 0, 0), (0.5, 0, 6), (0.7, 0, 2), (0.2, 0, 5),
            (0.9, 1, 2), (0.7, 1, 5), (0.5, 1, 0), (0.5, 1, 3), (0.5, 1, 1), (0.1, 1, 9),
            (0.3, 3, 7), (0.3, 3, 8)]
    score = np.array([r[0] for r in recs])
    i = np.array([r[1] for r in recs], dtype=np.int32)
    j = np.array([r[2] for r in recs], dtype=np.int32)
    order = np.lexsort((j, i, -score))
    return grid.Hits(score[order], i[order], j[order])


def test_select_top_k_with_groups_is_the_group_cut():
    from napkon_string_matching_amd import grid

    hits = _hits_with_ties()
    groups = np.array([7, 3, 3, 3, -2, 7, 11, 5, 5, 3], dtype=np.int32)
    assert group_cut([(0.9, 0, 4), (0.9, 0, 3), (0.9, 0, 1), (0.5, 0, 0)], groups, 2) == [(0.9, 0, 1), (0.9, 0, 4)]
    for k in (1, 2, 3, 10):
        got = grid.select_top_k(hits, k, groups).as_tuples()
        assert got == group_cut(hits.as_tuples(), groups, k), k
    # every right row a group of its own: the ungrouped cut; one group: one record per left item
    for k in (1, 2, 10):
        assert grid.select_top_k(hits, k, np.arange(10)).as_tuples() == grid.select_top_k(hits, k).as_tuples()
    assert grid.select_top_k(hits, 5, np.zeros(10, dtype=np.int64)).as_tuples() == [(0.9, 0, 1), (0.9, 1, 2), (0.3, 3, 7)]
    empty = grid.Hits(np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert len(grid.select_top_k(empty, 3, groups)) == 0


def test_select_top_k_without_groups_is_unchanged():
    from napkon_string_matching_amd import grid

    hits = _hits_with_ties()
    want = {1: [(0.9, 0, 1), (0.9, 1, 2), (0.3, 3, 7)],
            2: [(0.9, 0, 1), (0.9, 0, 3), (0.9, 1, 2), (0.7, 1, 5), (0.3, 3, 7), (0.3, 3, 8)]}
    for k, rows in want.items():
        assert grid.select_top_k(hits, k).as_tuples() == rows
        assert grid.select_top_k(hits, k, None).as_tuples() == rows
    assert grid.select_top_k(hits, 10).as_tuples() == hits.as_tuples()


def test_wrong_number_of_groups_raises_value_error_before_device_work():
    from napkon_string_matching_amd import grid, tables
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    for groups in (["x"], ["x", "y", "z"], []):
        with pytest.raises(ValueError):
            fuzzy_match.top_k(["abc"], ["abd", "x"], 1, groups=groups)
        with pytest.raises(ValueError):
            intersection_vs_union.top_k(["a b"], ["a", "b c"], 2, 0.5, groups=groups)
    codes = np.zeros((3, 64), dtype=np.uint8)
    lens = np.array([3, 2, 1], dtype=np.int32)
    lt = tables.StrTable.from_codes(codes[:2], lens[:2], 4, "cpu")
    rt = tables.StrTable.from_codes(codes, lens, 4, "cpu")
    ids = np.array([[0, 1, -1, -1], [2, -1, -1, -1], [1, 2, 3, -1]], dtype=np.int32)
    ls = tables.SetTable.from_padded(ids[:2], "left", "cpu")
    rs = tables.SetTable.from_padded(ids, "right", "cpu")
    for groups in (np.zeros(2, dtype=np.int32), np.zeros(4, dtype=np.int32), [0, 1]):
        with pytest.raises(ValueError):
            grid.indel_raw_top_k(lt, rt, 2, 0.0, groups=groups)
        with pytest.raises(ValueError):
            grid.jaccard_raw_top_k(ls, rs, 2, 0.0, groups=groups)


def test_grouped_top_k_without_gpu_raises_library_error():
    import torch

    from napkon_string_matching_amd import _lib
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.NsmLibraryError):
        fuzzy_match.top_k(["abc"], ["abd", "x"], 1, groups=["g", "g"])
    with pytest.raises(_lib.NsmLibraryError):
        intersection_vs_union.top_k(["a b"], ["a", "b c"], 2, 0.5, groups=[1, 2])


# ---------------------------------------------------------------------------------------------- the entries' error surface
# (label, arguments of support.top_k_entry_errors.call, status, nsm_last_error()): recorded from the library before the
# entries' host code was unified; a case with two faults pins which check speaks first
S = dict
INDEL_GROUP_CASES = [
    ('null right_group', S(group=NULL),
     BADARG, '{who}: right_group is null'),
    ('null right_group + null out', S(group=NULL, out=False),
     BADARG, '{who}: null argument'),
    ('null right_group + k = 0', S(group=NULL, k=0),
     BADARG, '{who}: k = 0 (must be >= 1)'),
    ('null right_group + strides differ', S(group=NULL, right=S(stride=128)),
     BADARG, '{who}: right_group is null'),
    ('null right_group + k beyond 4096', S(group=NULL, k=4097),
     BADARG, '{who}: right_group is null'),
    ('null right_group + empty left side', S(group=NULL, left=S(n=0)),
     BADARG, '{who}: right_group is null'),
]
JACCARD_GROUP_CASES = [
    ('null right_group', S(group=NULL),
     BADARG, '{who}: right_group is null'),
    ('null right_group + null out_count', S(group=NULL, out_count=False),
     BADARG, '{who}: null argument'),
    ('null right_group + k = -1', S(group=NULL, k=-1),
     BADARG, '{who}: k = -1 (must be >= 1)'),
    ('null right_group + widths differ', S(group=NULL, right=S(width=32)),
     BADARG, '{who}: right_group is null'),
    ('null right_group + k beyond 4096', S(group=NULL, k=4097),
     BADARG, '{who}: right_group is null'),
]


def test_grouped_entries_answer_a_null_group_column_exactly_as_recorded():
    from napkon_string_matching_amd import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("libnsm_hip.so not built")
    check_table(["nsm_indel_raw_top_k_grouped"], INDEL_GROUP_CASES)
    check_table(["nsm_jaccard_raw_top_k_grouped"], JACCARD_GROUP_CASES)
