"""Per-item top-k of the RAW grids: what is decided before any device work (no GPU needed)."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from support.top_k_entry_errors import BADARG, NULL, OK, UNSUPPORTED, check_table

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("k", [0, -1, 2.5, True, "3", None])
def test_bad_k_raises_value_error_before_device_work(k):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    with pytest.raises(ValueError):
        fuzzy_match.top_k(["a"], ["a"], k)
    with pytest.raises(ValueError):
        intersection_vs_union.top_k(["a"], ["a"], k)
    with pytest.raises(ValueError):
        grid.check_k(k)


def test_bad_limit_raises_value_error():
    import pandas as pd

    from napkon_string_matching_amd.terminology.mesh import MeshProvider

    provider = MeshProvider(None, synonyms=pd.DataFrame({"Id": ["D1"], "Term": ["Dialyse"]}))
    with pytest.raises(ValueError):
        provider.get_matches_batch([["dialyse"]], 0.1, limit=0)


def test_top_k_without_gpu_raises_library_error():
    import torch

    from napkon_string_matching_amd import _lib
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.NsmLibraryError):
        fuzzy_match.top_k(["abc"], ["abd", "x"], 1)
    with pytest.raises(_lib.NsmLibraryError):
        intersection_vs_union.top_k(["a b"], ["a", "b c"], 2, 0.5)


def test_c_entries_reject_bad_k_without_touching_the_device():
    from napkon_string_matching_amd import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("libnsm_hip.so not built")
    lib = _lib.load()
    cnt = ctypes.c_ulonglong(0)
    hit = _lib.NsmHit()
    s = _lib.NsmStrTable(None, None, None, None, None, 3, 64, 10)
    a = _lib.NsmSetTable(None, None, None, None, None, None, None, None, None, None, None, None, 3, 16, 0)
    for k in (0, -1):
        rc = lib.nsm_indel_raw_top_k(s, s, 0.5, k, _lib.FLAG_PRUNE, ctypes.addressof(hit), ctypes.addressof(cnt), None, None)
        assert rc == 10001 and b"k" in lib.nsm_last_error()
        rc = lib.nsm_jaccard_raw_top_k(a, a, 0.5, k, _lib.FLAG_PRUNE, ctypes.addressof(hit), ctypes.addressof(cnt), None, None)
        assert rc == 10001 and b"k" in lib.nsm_last_error()
    # width / stride mismatch and a right table without its class starts: NSM_E_BADARG, before any launch
    b = _lib.NsmSetTable(None, None, None, None, None, None, None, None, None, None, None, None, 3, 32, 0)
    rc = lib.nsm_jaccard_raw_top_k(a, b, 0.5, 1, 0, ctypes.addressof(hit), ctypes.addressof(cnt), None, None)
    assert rc == 10001 and b"width" in lib.nsm_last_error()
    s2 = _lib.NsmStrTable(None, None, None, None, None, 3, 128, 10)
    rc = lib.nsm_indel_raw_top_k(s, s2, 0.5, 1, 0, ctypes.addressof(hit), ctypes.addressof(cnt), None, None)
    assert rc == 10001 and b"stride" in lib.nsm_last_error()
    rc = lib.nsm_indel_raw_top_k(s, s, 0.5, 1, 0, ctypes.addressof(hit), ctypes.addressof(cnt), None, None)
    assert rc == 10001 and b"len_start" in lib.nsm_last_error()
    rc = lib.nsm_jaccard_raw_top_k(a, a, 0.5, 1, 0, ctypes.addressof(hit), ctypes.addressof(cnt), None, None)
    assert rc == 10001 and b"size_start" in lib.nsm_last_error()
    assert cnt.value == 0


def test_select_top_k_is_the_rank_cut():
    from napkon_string_matching_amd import grid

    score = np.array([0.9, 0.9, 0.5, 0.5, 0.5, 0.7, 0.1])
    i = np.array([0, 1, 0, 0, 1, 1, 1], dtype=np.int32)
    j = np.array([4, 2, 3, 1, 0, 5, 9], dtype=np.int32)
    order = np.lexsort((j, i, -score))
    hits = grid.Hits(score[order], i[order], j[order])
    got = grid.select_top_k(hits, 2).as_tuples()
    assert got == [(0.9, 0, 4), (0.9, 1, 2), (0.7, 1, 5), (0.5, 0, 1)]
    assert grid.select_top_k(hits, 10).as_tuples() == hits.as_tuples()


# ---------------------------------------------------------------------------------------------- the entries' error surface
# (label, arguments of support.top_k_entry_errors.call, status, nsm_last_error()): recorded from the library before the
# entries' host code was unified; a case with two faults pins which check speaks first
S = dict
INDEL_RAW_CASES = [
    ('null left', S(left=NULL),
     BADARG, '{who}: null argument'),
    ('null right', S(right=NULL),
     BADARG, '{who}: null argument'),
    ('null out', S(out=False),
     BADARG, '{who}: null argument'),
    ('null out_count', S(out_count=False),
     BADARG, '{who}: null argument'),
    ('k = 0', S(k=0),
     BADARG, '{who}: k = 0 (must be >= 1)'),
    ('k = -1', S(k=-1),
     BADARG, '{who}: k = -1 (must be >= 1)'),
    ('k beyond 4096 after clamping', S(k=4097),
     UNSUPPORTED, '{who}: k = 4097 exceeds the supported 4096'),
    ('k clamped to the right rows, empty left side', S(k=4097, left=S(n=0), right=S(n=30)),
     OK, None),
    ('k beyond 4096, empty left side', S(k=4097, left=S(n=0)),
     UNSUPPORTED, '{who}: k = 4097 exceeds the supported 4096'),
    ('strides differ', S(right=S(stride=128)),
     BADARG, '{who}: strides differ (64, 128)'),
    ('stride 32', S(left=S(stride=32), right=S(stride=32)),
     UNSUPPORTED, '{who}: stride 32 unsupported (64, 128, 256 or 512 code units)'),
    ('stride 1024', S(left=S(stride=1024), right=S(stride=1024)),
     UNSUPPORTED, '{who}: stride 1024 unsupported (64, 128, 256 or 512 code units)'),
    ('alphabets differ', S(right=S(alphabet=11)),
     BADARG, '{who}: alphabets differ or exceed 255 (10, 11)'),
    ('alphabet 0', S(left=S(alphabet=0), right=S(alphabet=0)),
     BADARG, '{who}: alphabets differ or exceed 255 (0, 0)'),
    ('alphabet 256', S(left=S(alphabet=256), right=S(alphabet=256)),
     BADARG, '{who}: alphabets differ or exceed 255 (256, 256)'),
    ('negative left n', S(left=S(n=-1)),
     BADARG, '{who}: negative row count'),
    ('negative right n', S(right=S(n=-2)),
     BADARG, '{who}: negative row count'),
    ('no len_start', S(right=S(len_start=NULL)),
     BADARG, '{who}: table has a null column (the right table needs len_start)'),
    ('no left codes', S(left=S(codes=NULL)),
     BADARG, '{who}: table has a null column (the right table needs len_start)'),
    ('no left len_start (not needed), empty right side', S(left=S(len_start=NULL), right=S(n=0)),
     OK, None),
    ('null left + k = 0', S(left=NULL, k=0),
     BADARG, '{who}: null argument'),
    ('k = 0 + strides differ', S(k=0, right=S(stride=128)),
     BADARG, '{who}: k = 0 (must be >= 1)'),
    ('k = -1 + no len_start', S(k=-1, right=S(len_start=NULL)),
     BADARG, '{who}: k = -1 (must be >= 1)'),
    ('strides differ + alphabets differ', S(right=S(stride=128, alphabet=11)),
     BADARG, '{who}: strides differ (64, 128)'),
    ('stride 32 + alphabets differ', S(left=S(stride=32), right=S(stride=32, alphabet=11)),
     UNSUPPORTED, '{who}: stride 32 unsupported (64, 128, 256 or 512 code units)'),
    ('alphabets differ + negative n', S(left=S(n=-1), right=S(alphabet=11)),
     BADARG, '{who}: alphabets differ or exceed 255 (10, 11)'),
    ('negative n + no len_start', S(left=S(n=-1), right=S(len_start=NULL)),
     BADARG, '{who}: negative row count'),
    ('no len_start + k beyond 4096', S(k=4097, right=S(len_start=NULL)),
     BADARG, '{who}: table has a null column (the right table needs len_start)'),
    ('negative right n + k = 5', S(k=5, right=S(n=-2)),
     BADARG, '{who}: negative row count'),
]
JACCARD_RAW_CASES = [
    ('null left', S(left=NULL),
     BADARG, '{who}: null argument'),
    ('null right', S(right=NULL),
     BADARG, '{who}: null argument'),
    ('null out', S(out=False),
     BADARG, '{who}: null argument'),
    ('null out_count', S(out_count=False),
     BADARG, '{who}: null argument'),
    ('k = 0', S(k=0),
     BADARG, '{who}: k = 0 (must be >= 1)'),
    ('k = -1', S(k=-1),
     BADARG, '{who}: k = -1 (must be >= 1)'),
    ('k beyond 4096 after clamping', S(k=4097),
     UNSUPPORTED, '{who}: k = 4097 exceeds the supported 4096'),
    ('k clamped to the right rows, empty left side', S(k=4097, left=S(n=0), right=S(n=30)),
     OK, None),
    ('widths differ', S(right=S(width=32)),
     BADARG, '{who}: width 16/32 unsupported (both sides 16, 32 or 64)'),
    ('width 8', S(left=S(width=8), right=S(width=8)),
     BADARG, '{who}: width 8/8 unsupported (both sides 16, 32 or 64)'),
    ('width 128', S(left=S(width=128), right=S(width=128)),
     BADARG, '{who}: width 128/128 unsupported (both sides 16, 32 or 64)'),
    ('negative left n', S(left=S(n=-1)),
     BADARG, '{who}: negative row count'),
    ('negative right n', S(right=S(n=-2)),
     BADARG, '{who}: negative row count'),
    ('no size_start', S(right=S(size_start=NULL)),
     BADARG, '{who}: table has a null column (the right table needs size_start)'),
    ('no left cnt', S(left=S(cnt=NULL)),
     BADARG, '{who}: table has a null column (the right table needs size_start)'),
    ('no left size_start (not needed), empty right side', S(left=S(size_start=NULL), right=S(n=0)),
     OK, None),
    ('null right + k = -1', S(right=NULL, k=-1),
     BADARG, '{who}: null argument'),
    ('k = 0 + widths differ', S(k=0, right=S(width=32)),
     BADARG, '{who}: k = 0 (must be >= 1)'),
    ('widths differ + negative n', S(left=S(n=-1), right=S(width=32)),
     BADARG, '{who}: width 16/32 unsupported (both sides 16, 32 or 64)'),
    ('negative n + no size_start', S(left=S(n=-1), right=S(size_start=NULL)),
     BADARG, '{who}: negative row count'),
    ('no size_start + k beyond 4096', S(k=4097, right=S(size_start=NULL)),
     BADARG, '{who}: table has a null column (the right table needs size_start)'),
]


def test_raw_entries_answer_malformed_calls_exactly_as_recorded():
    from napkon_string_matching_amd import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("libnsm_hip.so not built")
    check_table(["nsm_indel_raw_top_k", "nsm_indel_raw_top_k_grouped"], INDEL_RAW_CASES)
    check_table(["nsm_jaccard_raw_top_k", "nsm_jaccard_raw_top_k_grouped"], JACCARD_RAW_CASES)
