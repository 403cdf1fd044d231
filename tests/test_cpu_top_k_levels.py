"""Per-item top-k of the LEVELS grids and compare(top_k=): what is decided before any device work (no GPU needed)."""
import ctypes
import json
from hashlib import md5

import pandas as pd
import pytest

COLUMNS = ["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"]


def _cohort(prefix, n, categories=None):
    rows = [[f"{prefix}{k}", f"v{k}", "s", categories[k] if categories else [f"c{k % 3}"], [f"word{k % 7} w{k % 5}"],
             [f"word{k % 7}", f"w{k % 5}"], "p"] for k in range(n)]
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    return Questionnaire(pd.DataFrame(rows, columns=COLUMNS))


KW = dict(score_func="fuzzy_match", compare_column="Tokens", left_name="hap", right_name="pop", score_threshold=0.2)


@pytest.mark.parametrize("k", [0, -1, 2.5, True, "3"])
def test_bad_k_raises_value_error_before_device_work(k):
    left, right = _cohort("a", 4), _cohort("b", 5)
    with pytest.raises(ValueError):
        left.compare(right, None, None, top_k=k, **KW)
    with pytest.raises(ValueError):
        left.gen_comparable(right, None, None, top_k=k, **KW)


def test_k_beyond_4096_raises_before_device_work():
    left, right = _cohort("a", 2), _cohort("b", 4100)
    with pytest.raises(NotImplementedError):
        left.compare(right, None, None, top_k=4097, **KW)
    # clamped to the right side's items first: 4097 on 4100 items is too many, on 30 it is 30
    small = _cohort("c", 30)
    from napkon_string_matching_amd import _lib

    import torch

    if not torch.cuda.is_available():
        with pytest.raises(_lib.NsmLibraryError):  # (past the argument checks: the device is missing)
            left.compare(small, None, None, top_k=4097, **KW)


def test_more_than_64_category_labels_raise_before_device_work():
    labels = [[f"c{k}", f"d{k}"] for k in range(40)]
    left, right = _cohort("a", 40, labels), _cohort("b", 40, labels)
    with pytest.raises(NotImplementedError):
        left.compare(right, None, None, top_k=3, filter_categories=True, **KW)


def _old_key(data, other, wl, bl, column, thr, kwargs):
    """The compare cache key as it was before top_k existed."""
    parts = [data.to_csv(), other.to_csv(), json.dumps({}, sort_keys=True), json.dumps({}, sort_keys=True), str(column),
             repr(thr), json.dumps({k: kwargs.get(k) for k in ("score_func", "filter_categories", "category_column",
                                                               "left_name", "right_name")}, sort_keys=True, default=str)]
    return md5("\x1f".join(parts).encode("utf-8"), usedforsecurity=False).hexdigest()


def test_cache_key_unchanged_without_top_k_and_distinct_with_it():
    left, right = _cohort("a", 4), _cohort("b", 5)
    kwargs = {k: v for k, v in KW.items() if k not in ("compare_column", "score_threshold")}
    plain = left._hash_compare_args(right, None, None, "Tokens", 0.2, kwargs)
    assert plain == _old_key(left, right, None, None, "Tokens", 0.2, kwargs)
    assert left._hash_compare_args(right, None, None, "Tokens", 0.2, kwargs, None) == plain
    with_k = left._hash_compare_args(right, None, None, "Tokens", 0.2, kwargs, 3)
    assert with_k != plain and with_k != left._hash_compare_args(right, None, None, "Tokens", 0.2, kwargs, 4)


def test_symbols_exported_and_entries_check_arguments_without_the_device():
    from napkon_string_matching_amd import _lib

    assert {"nsm_indel_levels_top_k", "nsm_jaccard_levels_top_k"} <= set(_lib.EXPORTS)
    if not _lib.LIB_PATH.exists():
        pytest.skip("libnsm_hip.so not built")
    lib = _lib.load()
    assert lib.nsm_abi_version() == 5
    cnt = ctypes.c_ulonglong(0)
    hit = _lib.NsmHit()
    fake = 16  # column pointers are never dereferenced on the host; the calls below end before any launch
    items = _lib.NsmLevelItems(fake, fake, fake, None, None, None, 5000)
    s64 = _lib.NsmStrTable(fake, fake, fake, None, None, 0, 64, 10)
    s128 = _lib.NsmStrTable(fake, fake, fake, None, None, 0, 128, 10)
    sets = _lib.NsmSetTable(fake, fake, None, None, fake, None, fake, fake, None, None, None, None, 5000, 16, 4)
    sets32 = _lib.NsmSetTable(fake, fake, None, None, fake, None, fake, fake, None, None, None, None, 5000, 32, 4)
    out = (ctypes.addressof(hit), ctypes.addressof(cnt), None, None)
    for k in (0, -1):
        assert lib.nsm_indel_levels_top_k(items, s64, items, s64, 0.5, k, 0, 1, None, None, *out) == 10001
        assert lib.nsm_jaccard_levels_top_k(sets, sets, 0.5, k, 0, 1, None, None, *out) == 10001
    assert lib.nsm_indel_levels_top_k(items, s64, items, s64, 0.5, 4097, 0, 1, None, None, *out) == 10002
    assert lib.nsm_jaccard_levels_top_k(sets, sets, 0.5, 4097, 0, 1, None, None, *out) == 10002
    assert lib.nsm_indel_levels_top_k(items, s64, items, s128, 0.5, 3, 0, 1, None, None, *out) == 10001
    assert b"stride" in lib.nsm_last_error()
    assert lib.nsm_jaccard_levels_top_k(sets, sets32, 0.5, 3, 0, 1, None, None, *out) == 10001
    assert b"width" in lib.nsm_last_error()
    part = _lib.NsmLevelItems(fake, fake, fake, fake, fake, fake, 5000)
    assert lib.nsm_indel_levels_top_k(part, s64, part, s64, 0.5, 3, 1, 1, None, None, *out) == 10002
    # a category predicate without masks, half a blacklist: NSM_E_BADARG
    assert lib.nsm_indel_levels_top_k(items, s64, items, s64, 0.5, 3, 1, 1, None, None, *out) == 10001
    assert lib.nsm_jaccard_levels_top_k(sets, sets, 0.5, 3, 0, 1, fake, None, *out) == 10001
    assert cnt.value == 0
