"""Per-item top-k of the LEVELS grids and compare(top_k=): what is decided before any device work (no GPU needed)."""
import ctypes
import json
from hashlib import md5

import pandas as pd
import pytest

from support.top_k_entry_errors import BADARG, FAKE, NULL, OK, UNSUPPORTED, check_table

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


# ---------------------------------------------------------------------------------------------- the entries' error surface
# (label, arguments of support.top_k_entry_errors.call, status, nsm_last_error()): recorded from the library before the
# entries' host code was unified; a case with two faults pins which check speaks first
S = dict
INDEL_LEVELS_CASES = [
    ('null left', S(left=NULL),
     BADARG, '{who}: null argument'),
    ('null right', S(right=NULL),
     BADARG, '{who}: null argument'),
    ('null left_strings', S(left_strings=NULL),
     BADARG, '{who}: null argument'),
    ('null right_strings', S(right_strings=NULL),
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
    ('k clamped to the right items, empty left side', S(k=4097, left=S(n=0), right=S(n=30)),
     OK, None),
    ('strides differ', S(right_strings=S(stride=128)),
     BADARG, '{who}: strides differ (64, 128)'),
    ('stride 32', S(left_strings=S(stride=32), right_strings=S(stride=32)),
     UNSUPPORTED, '{who}: stride 32 unsupported (64, 128, 256 or 512 code units)'),
    ('stride 1024', S(left_strings=S(stride=1024), right_strings=S(stride=1024)),
     UNSUPPORTED, '{who}: stride 1024 unsupported (64, 128, 256 or 512 code units)'),
    ('alphabets differ', S(right_strings=S(alphabet=11)),
     BADARG, '{who}: alphabets differ or exceed 255 (10, 11)'),
    ('alphabet 0', S(left_strings=S(alphabet=0), right_strings=S(alphabet=0)),
     BADARG, '{who}: alphabets differ or exceed 255 (0, 0)'),
    ('alphabet 256', S(left_strings=S(alphabet=256), right_strings=S(alphabet=256)),
     BADARG, '{who}: alphabets differ or exceed 255 (256, 256)'),
    ('partitioned left (seg)', S(left=S(seg=FAKE)),
     UNSUPPORTED, '{who}: partitioned item tables are not supported (an item must be one row: encode with partition=False)'),
    ('partitioned right (seg_start)', S(right=S(seg_start=FAKE)),
     UNSUPPORTED, '{who}: partitioned item tables are not supported (an item must be one row: encode with partition=False)'),
    ('negative left n', S(left=S(n=-1)),
     BADARG, '{who}: negative item count'),
    ('negative right n', S(right=S(n=-2)),
     BADARG, '{who}: negative item count'),
    ('no left first', S(left=S(first=NULL)),
     BADARG, '{who}: table has a null column'),
    ('no right strings len', S(right_strings=S(len=NULL)),
     BADARG, '{who}: table has a null column'),
    ('len_start is not needed, empty right side', S(right_strings=S(len_start=NULL), right=S(n=0)),
     OK, None),
    ('unknown category_mode', S(category_mode=7),
     BADARG, '{who}: unknown category_mode 7'),
    ('category_mode without cat', S(category_mode=1),
     BADARG, '{who}: a category predicate needs `cat` on both sides'),
    ('category_mode with cat on one side', S(category_mode=2, left=S(cat=FAKE)),
     BADARG, '{who}: a category predicate needs `cat` on both sides'),
    ('banned_start alone', S(banned=(FAKE, NULL)),
     BADARG, '{who}: banned_start and banned_j go together'),
    ('banned_j alone', S(banned=(NULL, FAKE)),
     BADARG, '{who}: banned_start and banned_j go together'),
    ('null right + k = 0', S(right=NULL, k=0),
     BADARG, '{who}: null argument'),
    ('k = 0 + strides differ', S(k=0, right_strings=S(stride=128)),
     BADARG, '{who}: k = 0 (must be >= 1)'),
    ('strides differ + alphabets differ', S(right_strings=S(stride=128, alphabet=11)),
     BADARG, '{who}: strides differ (64, 128)'),
    ('stride 32 + partitioned', S(left_strings=S(stride=32), right_strings=S(stride=32), left=S(seg=FAKE)),
     UNSUPPORTED, '{who}: stride 32 unsupported (64, 128, 256 or 512 code units)'),
    ('alphabets differ + partitioned', S(right_strings=S(alphabet=11), left=S(seg=FAKE)),
     BADARG, '{who}: alphabets differ or exceed 255 (10, 11)'),
    ('partitioned + negative n', S(left=S(seg=FAKE, n=-1)),
     UNSUPPORTED, '{who}: partitioned item tables are not supported (an item must be one row: encode with partition=False)'),
    ('negative n + null column', S(left=S(n=-1, first=NULL)),
     BADARG, '{who}: negative item count'),
    ('null column + unknown category_mode', S(left=S(first=NULL), category_mode=7),
     BADARG, '{who}: table has a null column'),
    ('unknown category_mode + banned_start alone', S(category_mode=7, banned=(FAKE, NULL)),
     BADARG, '{who}: unknown category_mode 7'),
    ('category_mode without cat + banned_j alone', S(category_mode=1, banned=(NULL, FAKE)),
     BADARG, '{who}: a category predicate needs `cat` on both sides'),
    ('banned_start alone + k beyond 4096', S(banned=(FAKE, NULL), k=4097),
     BADARG, '{who}: banned_start and banned_j go together'),
    ('category_mode without cat + k beyond 4096', S(category_mode=1, k=4097),
     BADARG, '{who}: a category predicate needs `cat` on both sides'),
    ('k beyond 4096 + empty left side', S(k=4097, left=S(n=0)),
     UNSUPPORTED, '{who}: k = 4097 exceeds the supported 4096'),
]
JACCARD_LEVELS_CASES = [
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
    ('k clamped to the right items, empty left side', S(k=4097, left=S(n=0), right=S(n=30)),
     OK, None),
    ('widths differ', S(right=S(width=32)),
     BADARG, '{who}: width 16/32 unsupported (both sides 16, 32 or 64)'),
    ('width 8', S(left=S(width=8), right=S(width=8)),
     BADARG, '{who}: width 8/8 unsupported (both sides 16, 32 or 64)'),
    ('width 128', S(left=S(width=128), right=S(width=128)),
     BADARG, '{who}: width 128/128 unsupported (both sides 16, 32 or 64)'),
    ('partitioned left (seg_start)', S(left=S(seg_start=FAKE)),
     UNSUPPORTED, '{who}: partitioned tables are not supported (an item must be one row: encode with partition=False)'),
    ('partitioned right (seg)', S(right=S(seg=FAKE)),
     UNSUPPORTED, '{who}: partitioned tables are not supported (an item must be one row: encode with partition=False)'),
    ('negative left n', S(left=S(n=-1)),
     BADARG, '{who}: negative row count'),
    ('negative right n', S(right=S(n=-2)),
     BADARG, '{who}: negative row count'),
    ('no plen', S(right=S(plen=NULL)),
     BADARG, '{who}: table has a null column (levels tables need nlev and plen)'),
    ('no left nlev', S(left=S(nlev=NULL)),
     BADARG, '{who}: table has a null column (levels tables need nlev and plen)'),
    ('max_levels 0', S(left=S(max_levels=0)),
     BADARG, '{who}: table has a null column (levels tables need nlev and plen)'),
    ('size_start is not needed, empty right side', S(right=S(size_start=NULL, n=0)),
     OK, None),
    ('unknown category_mode', S(category_mode=-1),
     BADARG, '{who}: unknown category_mode -1'),
    ('category_mode without cat', S(category_mode=2),
     BADARG, '{who}: a category predicate needs `cat` on both sides'),
    ('banned_start alone', S(banned=(FAKE, NULL)),
     BADARG, '{who}: banned_start and banned_j go together'),
    ('banned_j alone', S(banned=(NULL, FAKE)),
     BADARG, '{who}: banned_start and banned_j go together'),
    ('null left + k = -1', S(left=NULL, k=-1),
     BADARG, '{who}: null argument'),
    ('k = 0 + widths differ', S(k=0, right=S(width=32)),
     BADARG, '{who}: k = 0 (must be >= 1)'),
    ('widths differ + partitioned', S(right=S(width=32, seg=FAKE)),
     BADARG, '{who}: width 16/32 unsupported (both sides 16, 32 or 64)'),
    ('partitioned + negative n', S(right=S(seg=FAKE, n=-2)),
     UNSUPPORTED, '{who}: partitioned tables are not supported (an item must be one row: encode with partition=False)'),
    ('negative n + no plen', S(left=S(n=-1), right=S(plen=NULL)),
     BADARG, '{who}: negative row count'),
    ('no plen + unknown category_mode', S(right=S(plen=NULL), category_mode=9),
     BADARG, '{who}: table has a null column (levels tables need nlev and plen)'),
    ('unknown category_mode + banned_j alone', S(category_mode=9, banned=(NULL, FAKE)),
     BADARG, '{who}: unknown category_mode 9'),
    ('category_mode without cat + banned_start alone', S(category_mode=1, banned=(FAKE, NULL)),
     BADARG, '{who}: a category predicate needs `cat` on both sides'),
    ('banned_j alone + k beyond 4096', S(banned=(NULL, FAKE), k=4097),
     BADARG, '{who}: banned_start and banned_j go together'),
]


def test_levels_entries_answer_malformed_calls_exactly_as_recorded():
    from napkon_string_matching_amd import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("libnsm_hip.so not built")
    check_table(["nsm_indel_levels_top_k"], INDEL_LEVELS_CASES)
    check_table(["nsm_jaccard_levels_top_k"], JACCARD_LEVELS_CASES)
