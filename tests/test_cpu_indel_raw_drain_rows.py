"""The stack entry and the drain's row enumeration of the two-stage RAW fuzzy kernel (csrc/indel_raw_coarse.hpp), restated
in Python (tests/support/drain_rows.py) and checked against plain loops: no GPU.

An entry stands for one lane of the scan: 16 rows of a block of 32, rows (k & 3) + 8 (k >> 2) + 4 (lane >> 5).  Its low
word is the number of rows of the block that exist, and the drain keeps the verdict of exactly those of the lane's rows
that are below it.  A pass of the drain gives an entry four lanes, a row per lane and run, and the LCS walk finds entry and
row again from a lane and a bit of its mask.  The inputs are those of tests/test_gpu_indel_raw_drain_rows.py, where the same sets are compared with what the kernel
reports."""
import itertools

import pytest

from tests.support import drain_rows as dr


def test_entry_layout():
    """Every field survives a round trip at its extremes, and the high word is what the kernel's shifts give."""
    for row_rel, la, tile, lane, n_rows in itertools.product((0, 32, (1 << 15) - 32), (0, 1, 63, 64), range(4), (0, 31, 32, 63),
                                                             (1, 31, 32)):
        hi, lo = dr.pack_entry(row_rel, la, tile, lane, n_rows)
        assert hi < (1 << 32) and lo == n_rows
        assert hi == row_rel * 32768 + la * 256 + tile * 64 + lane
        assert dr.unpack_entry(hi, lo) == (row_rel, la, tile, lane, n_rows)


@pytest.mark.parametrize("n_rows", range(1, 33))
def test_rows_visited(n_rows):
    """Over both lane halves, the rows the drain visits are exactly the rows of the block that exist, each once."""
    seen = []
    for lane in (7, 39):  # one lane of either half
        rows = dr.drain_rows(lane, n_rows)
        plain = [r for r in range(32) if r < n_rows and ((r >> 2) & 1) == (lane >> 5)]
        assert sorted(rows) == plain and len(set(rows)) == len(rows)
        seen += rows
    assert sorted(seen) == list(range(n_rows))


def test_rows_of_a_lane():
    """The 64 lanes of a full block cover its 32 rows x 32 columns once: 16 rows a lane, two lanes a column, and the drain's
    rows of an entry are the rows of its scan lane."""
    cells = [(r, lane & 31) for lane in range(64) for r in dr.drain_rows(lane, 32)]
    assert len(cells) == 1024 and set(cells) == set(itertools.product(range(32), range(32)))
    assert [dr.lane_row(0, k) for k in range(16)] == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27]
    assert [dr.lane_row(32, k) for k in range(16)] == [4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]
    for lane in range(64):
        assert sorted(dr.drain_rows(lane, 32)) == [dr.lane_row(lane, k) for k in range(16)]


def test_places_of_a_pass():
    """The 64 entries x 16 rows of a pass take the 64 x 16 (drain lane, bit) places once, the four lanes of an entry are
    neighbours with consecutive rows (one run of 128 bytes per load), and the LCS walk finds entry and row again."""
    places = {}
    for e, g, m in itertools.product(range(64), range(4), range(4)):
        lane, bit = dr.place(e, g, m)
        assert 0 <= lane < 64 and 0 <= bit < 16 and (lane, bit) not in places
        places[lane, bit] = (e, g, m)
        assert lane >> 2 == e & 15 and lane & 3 == m
        for scan_lane in (5, 37):
            assert dr.walk_decode(lane, bit, scan_lane) == (e, 8 * g + 4 * (scan_lane >> 5) + m)
    assert len(places) == 1024


def _plain_lcs_pairs(m):
    """The pairs that pass the exact 32-bucket test within the lanes the fold passes, by a loop over rows."""
    out = set()
    for first, end, half, j in m.fold_lanes:
        for row in range(first, end):
            if ((row - first) >> 2) & 1 == half and m.exact(row, j):
                out.add((row, j))
    return out


def _cases():
    left, right, want = dr.case_row_positions()
    yield "row_positions", left, right, 0.8, want
    left, right, want = dr.case_many_rows()
    yield "many_rows", left, right, 0.8, want
    left, right, want = dr.case_short_blocks()
    yield "short_blocks", left, right, 0.8, want
    left, right, want = dr.case_chunk_ends()
    yield "chunk_ends", left, right, 0.8, want
    for n in (1, 33, 129):
        left, right = dr.case_ragged(n)
        yield f"ragged_{n}", left, right, 0.8, None
    left, right = dr.case_zero_and_one()
    yield "zero", left, right, 0.0, set(itertools.product(range(40), range(40)))
    yield "one", left, right, 1.0, {(i, j) for i, x in enumerate(left) for j, y in enumerate(right) if x == y and x}
    left, right = dr.case_four_letters()
    yield "four_letters", left, right, 0.5, None
    for which in ("long", "short"):
        left, right = dr.case_edge_lengths(which)
        yield f"edge_{which}", left, right, 0.8, None


CASES = {name: rest for name, *rest in _cases()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pairs_that_reach_the_lcs(name):
    """The drain's enumeration, entry by entry, reaches the LCS with the pairs that pass the exact test within the lanes the
    fold passes, each once, and the hits among them are the pairs the case was built for (or, where it names none, the
    pairs whose sum of bucket minima reaches need)."""
    left, right, thr, want = CASES[name]
    m = dr.Model(left, right, thr)
    assert len(m.lcs_pairs) == len(set(m.lcs_pairs))
    assert set(m.lcs_pairs) == _plain_lcs_pairs(m)
    hits = m.hits()
    assert len(hits) == len(set(hits))
    if want is None:
        want = set()
        for (i, x), (j, y) in itertools.product(enumerate(left), enumerate(right)):
            nd = dr.need_of(thr, len(x), len(y))
            if min(len(x), len(y)) >= nd and sum(map(min, dr.counts(x), dr.counts(y))) >= nd:
                want.add((i, j))
    assert set(hits) == want and len(want) > 0


def test_what_the_cases_are_about():
    """The row-position case has its 15 neighbours at need - 1, the many-rows case lanes of 2, 5 and 16 pairs, the chunk case
    chunks of 64 rows, and the four-letter case more than 128 entries waiting at a check."""
    left, right, want = dr.case_row_positions()
    lh, rh = list(map(dr.counts, left)), list(map(dr.counts, right))
    assert dr.need(0.8, 80) == 32 and {len(x) for x in left + right} == {40}
    for r_hit, j in want:
        for r in range(32):
            lcs = sum(map(min, lh[r], rh[j]))
            same_lane = ((r >> 2) & 1) == ((r_hit >> 2) & 1)
            assert lcs == (32 if r == r_hit else 31 if same_lane else 30 if (r & 3, r >> 3) != (r_hit & 3, r_hit >> 3) else 31)
    assert {r for r, _ in want} == set(range(32)) and all({r for r, j in want if j // 32 == t} == set(range(32)) for t in range(4))

    left, right, want = dr.case_many_rows()
    m = dr.Model(left, right, 0.8)
    per_entry = sorted(sum(1 for row, j in m.lcs_pairs if j == jj and ((row >> 2) & 1) == h) for jj in (0, 5, 17, 35) for h in (0, 1))
    assert per_entry == [0, 0, 0, 2, 3, 3, 5, 16]

    left, right, _ = dr.case_chunk_ends()
    assert dr.rows_per_chunk(len(left), len(right)) == 64
    m = dr.Model(left, right, 0.8)
    assert {chunk for _, chunk, _, _ in m.entries} == {0, 1, 2, 3}
    assert {dr.unpack_entry(hi, lo)[4] for _, chunk, hi, lo in m.entries if chunk == 3} == {8}  # 200 - 192 rows exist

    left, right, _ = dr.case_short_blocks()
    m = dr.Model(left, right, 0.8)
    assert {dr.unpack_entry(hi, lo)[4] for _, _, hi, lo in m.entries} == {1, 31, 32}  # last blocks of 65, 33, 32, 31, 1 rows

    left, right = dr.case_four_letters()
    m = dr.Model(left, right, 0.5)
    assert max(m.waiting) > dr.DRAIN_AT and len(m.entries) > 4 * 64 * 3
