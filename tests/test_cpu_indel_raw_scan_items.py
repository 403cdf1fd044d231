"""The work items of the persistent packed scan (tests/support/scan_items.py restates csrc/indel_raw_coarse.hpp:
c3p_prepass_kernel's interval, hull, window and item rules, and the scan's guided pull) against a brute-force "which
(tile, row) can fit" on small tables.

The scan keeps its own test per class and lane, so the list only has to be a SUPERSET: every row that fits some string
of a tile must lie in exactly one item of that tile, no item may cross a window of 2^15 rows or exceed ``item_rows``, and
an empty interval gives no item.
"""
import random

import pytest

from tests.support import scan_items as si


def _tables(left_lengths, right_lengths):
    """Sorted (descending) length columns and the left len_start (66 entries)."""
    llen = sorted(left_lengths, reverse=True)
    rlen = sorted(right_lengths, reverse=True)
    lstart = [sum(1 for x in llen if x > 64 - c) for c in range(66)]
    assert lstart[0] == 0 and lstart[65] == len(llen)
    return llen, rlen, lstart


def _fitting_rows(t, llen, rlen, lcsmin, zero_need):
    lbs = set(rlen[t * si.TILE:(t + 1) * si.TILE])
    return {i for i, la in enumerate(llen) if any(si.fits(la, lb, lcsmin, zero_need) for lb in lbs)}


def _check(llen, rlen, lstart, threshold, item_rows):
    lcsmin, zero_need = si.lcsmin_of(threshold)
    items = si.item_list(rlen, lstart, len(llen), lcsmin, zero_need, item_rows)
    assert items == sorted(items, key=lambda it: (it[0], it[1])), "tile-major, rows ascending"
    n_tiles = -(-len(rlen) // si.TILE)
    for t in range(n_tiles):
        mine = [it for it in items if it[0] == t]
        covered = []
        for _, first, end, base in mine:
            assert 0 <= base <= first < end <= len(llen)
            assert end - first <= item_rows
            assert end - base <= si.WINDOW, "an item must not cross its window"
            assert (first - base) % item_rows == 0
            covered += range(first, end)
        assert len(covered) == len(set(covered)), "a row in two items"
        want = _fitting_rows(t, llen, rlen, lcsmin, zero_need)
        assert want <= set(covered), f"tile {t}: rows that fit are in no item"
        if not want and zero_need != 0:
            # (a hull over one or two lengths that fit nothing is empty; a wider tile may cover rows that fit nothing)
            r0, rows = si.tile_interval(t, rlen, lstart, len(llen), lcsmin, zero_need)
            assert (rows == 0) == (not mine)
        bases = sorted({it[3] for it in mine})
        assert all(b - bases[0] in range(0, 1 << 31, si.WINDOW) for b in bases)
    assert len(items) <= n_tiles * si.items_of(len(llen), item_rows), "the host's bound on the list"
    return items


@pytest.mark.parametrize("threshold", [0.0, 0.8, 1.0])
@pytest.mark.parametrize("item_rows", [32, 64, 96])
def test_every_fitting_row_is_in_exactly_one_item(threshold, item_rows):
    rng = random.Random(int(threshold * 10) * 100 + item_rows)
    left = [rng.choice([0, 1, 2, 7, 8, 9, 10, 31, 32, 33, 40, 41, 50, 63, 64]) for _ in range(700)]
    right = [rng.randint(0, 64) for _ in range(3 * si.TILE + 17)]
    llen, rlen, lstart = _tables(left, right)
    items = _check(llen, rlen, lstart, threshold, item_rows)
    if threshold == 0.0:
        assert len(items) == 4 * si.items_of(700, item_rows)  # every row, every tile
    if threshold == 1.0:  # only equal lengths fit: the hull of a tile's lengths, no more
        for t, first, end, _ in items:
            lbs = rlen[t * si.TILE:(t + 1) * si.TILE]
            assert all(min(lbs) <= llen[i] <= max(lbs) for i in range(first, end))


def test_a_tile_with_two_far_apart_lengths():
    """Right lengths 64 and 16 in one tile at 0.8: the hull covers every left length from what fits 16 to what fits 64, the
    lengths between them included, which fit neither -- a superset, never less."""
    llen, rlen, lstart = _tables([64] * 40 + [40] * 70 + [16] * 40 + [5] * 30, [64] * 64 + [16] * 64)
    items = _check(llen, rlen, lstart, 0.8, 64)
    rows = {i for _, first, end, _ in items for i in range(first, end)}
    assert rows == set(range(0, 150)), "the rows of length 5 fit nothing and are left out; those of length 40 ride along"


def test_empty_intervals_give_no_item():
    """Left rows of 60 .. 64 units against right strings of 8 units at 0.8, and empty right strings where they do not score."""
    llen, rlen, lstart = _tables([60, 61, 62, 63, 64] * 20, [8] * 130 + [0] * 130)
    assert _check(llen, rlen, lstart, 0.8, 32) == []
    assert len(_check(llen, rlen, lstart, 0.0, 32)) == 3 * si.items_of(100, 32)


def test_windows():
    """2^15 + 200 rows of one length: the second window starts a new base, and the first window's last item is cut at it."""
    n = si.WINDOW + 200
    llen, rlen, lstart = _tables([30] * n, [30] * 129)
    items = _check(llen, rlen, lstart, 0.8, 2400)
    tile0 = [it for it in items if it[0] == 0]
    assert {it[3] for it in tile0} == {0, si.WINDOW}
    assert (0, 13 * 2400, si.WINDOW, 0) in tile0 and (0, si.WINDOW, n, si.WINDOW) in tile0
    assert len(items) == 2 * (14 + 1)


@pytest.mark.parametrize("n_waves", [1, 4, 4096])
@pytest.mark.parametrize("n_items", [0, 1, 5, 1000, 71000])
def test_guided_pull_covers_every_item_once(n_waves, n_items):
    rng = random.Random(n_waves + n_items)

    def order():
        while True:
            yield rng.randrange(n_waves)

    for stale in (0, 3 * n_waves):
        taken = si.guided_pulls(n_items, n_waves, order(), stale=stale)
        ranges = sorted(r for rs in taken.values() for r in rs)
        assert all(a < b <= n_items for a, b in ranges)
        assert [a for a, _ in ranges] == [0] * (n_items > 0) + [b for _, b in ranges[:-1]], "ranges must tile [0, n)"
        assert (ranges[-1][1] if ranges else 0) == n_items
