"""Per-item top-k of the RAW grids: what is decided before any device work (no GPU needed)."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

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
