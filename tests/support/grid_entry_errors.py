"""Malformed calls to the four ``nsm_*_grid`` entries and to ``nsm_indel_levels_workspace_bytes``, made without a device:
every call here ends in the entry's host code -- an argument check, an empty side, or a geometry that does not fit --
before any HIP call.  The struct builders are those of ``top_k_entry_errors``; the tables of cases with the exact
(status, ``nsm_last_error()``) live in ``test_cpu_grid_entry_errors.py``."""
import ctypes
from types import MappingProxyType

from support.top_k_entry_errors import FAKE, level_items, set_table, str_table

VALID = MappingProxyType({})  # no override: the table as the builder makes it (read-only; None is NULL, a null table pointer)
LEVEL_SETS = dict(sig=FAKE, filt=FAKE)  # what a levels-mode set table carries beyond the builder's columns


def call(entry, left=VALID, right=VALID, left_strings=VALID, right_strings=VALID, threshold=0.5, category_mode=0, flags=0, hits=True,
         capacity=1, hit_count=True, workspace=None, workspace_bytes=0, expected_survivors=0.0):
    """(status, message) of the grid ``entry`` on tables that are valid but for the given overrides (a dict of struct
    fields, or NULL for a null table pointer).  The message of a call that succeeds is None.  No call may count a hit."""
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    hit, cnt = _lib.NsmHit(), ctypes.c_ulonglong(0)
    out = (ctypes.addressof(hit) if hits else None, capacity, ctypes.addressof(cnt) if hit_count else None)
    if entry == "nsm_indel_levels_grid":
        args = (level_items(left), str_table(left_strings), level_items(right), str_table(right_strings), threshold,
                category_mode, flags) + out + (workspace, workspace_bytes, expected_survivors, None)
    elif entry == "nsm_indel_raw_grid":
        args = (str_table(left), str_table(right), threshold, flags) + out + (None,)
    elif entry == "nsm_jaccard_raw_grid":
        args = (set_table(left), set_table(right), threshold, flags) + out + (None,)
    else:
        both = [None if t is None else {**LEVEL_SETS, **t} for t in (left, right)]
        args = (set_table(both[0]), set_table(both[1]), threshold, category_mode, flags) + out + (None,)
    rc = getattr(lib, entry)(*args)
    assert cnt.value == 0
    return rc, (lib.nsm_last_error().decode() if rc else None)


def workspace_bytes(left=VALID, right=VALID, left_strings=VALID, right_strings=VALID, threshold=0.8, flags=1, expected_survivors=0.0):
    """``nsm_indel_levels_workspace_bytes`` on a grid the split path takes (5000 x 5000 one-word strings with histograms,
    NSM_FLAG_PRUNE, threshold 0.8) but for the given overrides."""
    from napkon_string_matching_amd import _lib

    hist = dict(hist=FAKE)
    strings = [None if t is None else {**hist, **t} for t in (left_strings, right_strings)]
    return _lib.load().nsm_indel_levels_workspace_bytes(level_items(left), str_table(strings[0]), level_items(right),
                                                       str_table(strings[1]), threshold, flags, expected_survivors)


def check_table(entry, cases):
    """``cases``: (label, keyword arguments of ``call``, status, message with ``{who}`` for the entry's name)."""
    for label, kw, status, message in cases:
        want = (status, None if message is None else message.format(who=entry))
        assert call(entry, **kw) == want, (entry, label)
