"""Floor grids and best matches: the definitions in plain Python on (score, i, j) records, shared by
tests/test_cpu_best.py (``grid.best_of_hits`` / ``grid.filter_by_floors`` against them on the oracle's lists) and
tests/test_gpu_best.py (the device paths against them), and malformed calls to the four ``nsm_*_floor_grid`` entries made
without a device (struct builders of ``top_k_entry_errors``)."""
import ctypes
import math
from types import MappingProxyType

import numpy as np

from support.top_k_entry_errors import FAKE, level_items, set_table, str_table

canonical = lambda records: sorted(records, key=lambda r: (-r[0], r[1], r[2]))


def bests(records):
    """({left item: its largest score}, {right item: its largest score}) of a record list."""
    lb, rb = {}, {}
    for s, i, j in records:
        lb[i] = max(lb.get(i, s), s)
        rb[j] = max(rb.get(j, s), s)
    return lb, rb


def best_plain(records, margin, mutual):
    """The records within ``margin`` of their left item's best score, with ``mutual`` also of their right item's: one
    double subtraction, exact comparisons.  Canonical order."""
    lb, rb = bests(records)
    return canonical([r for r in records if r[0] >= lb[r[1]] - margin and (not mutual or r[0] >= rb[r[2]] - margin)])


def floors_plain(records, left_floor, right_floor):
    """The records that reach their items' floors (sequences by item, or None); a NaN floor admits nothing."""
    return canonical([r for r in records if (left_floor is None or r[0] >= left_floor[r[1]])
                      and (right_floor is None or r[0] >= right_floor[r[2]])])


def to_hits(records):
    from napkon_string_matching_amd import grid

    return grid.Hits(np.array([r[0] for r in records], dtype=np.float64), np.array([r[1] for r in records], dtype=np.int32),
                     np.array([r[2] for r in records], dtype=np.int32))


def row_gap(records):
    """A positive difference of two scores of one left row (the first row that has two distinct positive scores): a margin
    that keeps some of a row's runners-up and not others."""
    rows = {}
    for s, i, _ in records:
        rows.setdefault(i, set()).add(s)
    for i in sorted(rows):
        distinct = sorted(rows[i], reverse=True)
        if len(distinct) >= 3 and distinct[1] > 0.0:
            return distinct[0] - distinct[1]
    raise AssertionError("no row with three distinct scores")


def probe_floors(records, s, floor, n_left, n_right):
    """The floors of one probe case: ``floor`` for the left items whose best score is ``s``, every other item its own
    best (an item without a record: 0.0); on either side one NaN and one -inf floor, put on items that have records (on the
    left side: that are not at the probe, if there are any)."""
    lb, rb = bests(records)
    left = [floor if lb.get(i) == s else lb.get(i, 0.0) for i in range(n_left)]
    right = [rb.get(j, 0.0) for j in range(n_right)]
    li, rj = [i for i in sorted(lb) if lb[i] != s], sorted(rb)  # (the items at the probe keep their floor)
    if li:  # (under the overlap measure every left item of a RAW probe grid has the best score 1.0)
        left[li[len(li) // 3]], left[li[2 * len(li) // 3]] = math.nan, -math.inf
    right[rj[len(rj) // 3]], right[rj[2 * len(rj) // 3]] = math.nan, -math.inf
    return left, right


# ------------------------------------------------------------------------------------------------ malformed calls
VALID = MappingProxyType({})
LEVEL_SETS = dict(filt=FAKE)
ENTRIES = ("nsm_indel_raw_floor_grid", "nsm_jaccard_raw_floor_grid", "nsm_indel_levels_floor_grid",
           "nsm_jaccard_levels_floor_grid")


def call(entry, left=VALID, right=VALID, left_strings=VALID, right_strings=VALID, threshold=0.5, left_floor=None,
         right_floor=None, category_mode=0, flags=1, banned=(None, None), hits=True, capacity=1, hit_count=True):
    """(status, message) of the floor grid ``entry`` on tables that are valid but for the given overrides (a dict of struct
    fields, or None for a null table pointer).  The message of a call that succeeds is None.  No call may count a hit:
    every call made here ends in the entry's host code, before any HIP call."""
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    hit, cnt = _lib.NsmHit(), ctypes.c_ulonglong(0)
    out = (ctypes.addressof(hit) if hits else None, capacity, ctypes.addressof(cnt) if hit_count else None, None, None)
    floors = (threshold, left_floor, right_floor)
    if entry == "nsm_indel_raw_floor_grid":
        args = (str_table(left), str_table(right)) + floors + (flags,)
    elif entry == "nsm_jaccard_raw_floor_grid":
        args = (set_table(left), set_table(right)) + floors + (flags,)
    elif entry == "nsm_indel_levels_floor_grid":
        args = (level_items(left), str_table(left_strings), level_items(right), str_table(right_strings)) + floors + \
            (category_mode, flags) + tuple(banned)
    else:
        both = [None if t is None else {**LEVEL_SETS, **t} for t in (left, right)]
        args = (set_table(both[0]), set_table(both[1])) + floors + (category_mode, flags) + tuple(banned)
    rc = getattr(lib, entry)(*args, *out)
    assert cnt.value == 0
    return rc, (lib.nsm_last_error().decode() if rc else None)


def check_table(entry, cases):
    """``cases``: (label, keyword arguments of ``call``, status, message with ``{who}`` for the entry's name)."""
    for label, kw, status, message in cases:
        want = (status, None if message is None else message.format(who=entry))
        assert call(entry, **kw) == want, (entry, label)
