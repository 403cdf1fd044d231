"""Malformed calls to the four ``nsm_*_pairs`` entries, made without a device: every call here ends in the entry's host
code -- an argument check, or the ``n_pairs == 0`` return -- before any HIP call.  The struct builders are those of
``top_k_entry_errors``; the tables of cases with the exact (status, ``nsm_last_error()``) live in ``test_cpu_pairs.py``."""
import ctypes

from support.grid_entry_errors import VALID
from support.top_k_entry_errors import FAKE, level_items, set_table, str_table

ENTRIES = ("nsm_indel_raw_pairs", "nsm_jaccard_raw_pairs", "nsm_indel_levels_pairs", "nsm_jaccard_levels_pairs")


def call(entry, left=VALID, right=VALID, left_strings=VALID, right_strings=VALID, left_row=FAKE, left_ids=5000, right_row=FAKE,
         right_ids=5000, pairs=True, n_pairs=1):
    """(status, message) of the pairs ``entry`` on tables that are valid but for the given overrides (a dict of struct
    fields, or None for a null table pointer).  The message of a call that succeeds is None.  No call may write a score."""
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    hit = _lib.NsmHit(score=7.0, i=1, j=2)
    tail = (left_row, left_ids, right_row, right_ids, ctypes.addressof(hit) if pairs else None, n_pairs, None)
    if entry == "nsm_indel_raw_pairs":
        args = (str_table(left), str_table(right))
    elif entry == "nsm_indel_levels_pairs":
        args = (level_items(left), str_table(left_strings), level_items(right), str_table(right_strings))
    else:
        args = (set_table(left), set_table(right))
    rc = getattr(lib, entry)(*args, *tail)
    assert (hit.score, hit.i, hit.j) == (7.0, 1, 2)
    return rc, (lib.nsm_last_error().decode() if rc else None)


def check_table(entry, cases):
    """``cases``: (label, keyword arguments of ``call``, status, message with ``{who}`` for the entry's name)."""
    for label, kw, status, message in cases:
        want = (status, None if message is None else message.format(who=entry))
        assert call(entry, **kw) == want, (entry, label)
