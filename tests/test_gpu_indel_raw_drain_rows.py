"""The drain of the two-stage RAW fuzzy kernel (csrc/indel_raw_coarse.hpp) when the scan pushes LANES and not rows.

A stack entry stands for one lane of the scan whose folded result passed: 16 left rows of a block against one right
string, and the number of rows of the block that exist.  The drain runs the exact 32-bucket test on those rows and scores
every pair that passes.  What can go wrong is the mapping from a bit of the drain's mask to a row of the block, the walk of
the LCS loop over lanes that hold several pairs, the rows past the end of a short block (they repeat its last row: a pair
must not show twice), blocks cut by the end of a chunk, right tables that leave tiles ragged, and the drain running
between the blocks of a class.

The inputs (tests/support/drain_rows.py, shared with tests/test_cpu_indel_raw_drain_rows.py, which checks the host-side
model of the same kernel) are sorted runs, LCS = sum of the bucket minima, so pairs sit exactly at need or at need - 1.
Every case compares the two-stage kernel with the exhaustive kernel (prune off) and with the oracle: records equal in
canonical order, counts equal."""
import itertools

import pytest

from tests.support import drain_rows as dr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _oracle(left, right, thr):
    from oracle import native

    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    return native.indel_raw(cp(left), cp(right), thr, cap=1 << 20)


def _check(dev, left, right, thresholds):
    """Two-stage, one-stage and exhaustive kernel against the oracle at every threshold; returns the oracle's hits at the
    lowest one and the left table."""
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd import tables as tb

    lt, rt = tb.encode_strings(left, right, dev)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None and lt.alphabet <= 32
    base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in ({}, {"prune": False}, {"two_stage": False}):
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return base, lt


def _pairs(base):
    pairs = [(i, j) for _, i, j in base]
    assert len(pairs) == len(set(pairs))
    return set(pairs)


def test_every_row_position(dev):
    """One hit in each of the 32 row positions of a block (both lane halves) in each of the four tiles; the other 15 rows of
    the hit's lane are at need - 1 with the same right string."""
    left, right, want = dr.case_row_positions()
    base, lt = _check(dev, left, right, (0.8,))
    assert lt.orig.cpu().tolist() == list(range(32))
    assert _pairs(base) == want and len(want) == 128


def test_lanes_with_many_pairs(dev):
    """Lanes with 2, 5 and all 16 of their rows at need with one right string, and a right string with three rows in either
    lane half: every pair once."""
    left, right, want = dr.case_many_rows()
    base, _ = _check(dev, left, right, (0.8,))
    assert _pairs(base) == want and len(want) == 2 + 5 + 16 + 6


def test_short_blocks(dev):
    """Length classes of 32, 31, 1, 65 and 33 rows whose last row hits every right string and whose second to last row hits
    none: last blocks of 32, 31 and 1 rows, each pair exactly once."""
    left, right, want = dr.case_short_blocks()
    base, lt = _check(dev, left, right, (0.8,))
    assert lt.orig.cpu().tolist() == list(range(len(left)))  # (built in table order: longest class first)
    assert _pairs(base) == want and len(want) == 5 * 33


def test_chunk_ends(dev):
    """One class of 200 rows in chunks of 64: hits in the last row before each chunk end and in the first row after it."""
    left, right, want = dr.case_chunk_ends()
    assert dr.rows_per_chunk(len(left), len(right)) == 64
    base, lt = _check(dev, left, right, (0.8,))
    assert lt.orig.cpu().tolist() == list(range(200))
    assert _pairs(base) == want and len(want) == 6 * 33


@pytest.mark.parametrize("n_right", [1, 33, 129])
def test_ragged_right_tables(dev, n_right):
    """Right tables of 1, 33 and 129 rows: tiles with columns that do not exist, and a second wave with one string."""
    left, right = dr.case_ragged(n_right)
    base, _ = _check(dev, left, right, (0.8,))
    assert 0 < len(base) < len(left) * n_right


@pytest.mark.parametrize("which", ["long", "short"])
def test_waves_that_fit_one_class_or_none(dev, which):
    """A wave whose right strings fit no length class of the chunk returns before it scans; one whose right strings fit only
    the chunk's longest (or shortest) class must not.  Threshold 0.0 on the same tables: empty-string scoring is on, nobody
    returns early and every pair is a hit."""
    left, right = dr.case_edge_lengths(which)
    base, _ = _check(dev, left, right, (0.0, 0.8))
    assert len(base) == len(left) * len(right)
    hits = [(len(left[i]), len(right[j])) for s, i, j in base if s >= 0.8]
    assert len(hits) > 200 and set(hits) == {(34, 51) if which == "long" else (40, 27)}


def test_threshold_zero_and_one(dev):
    """Threshold 0 with empty strings on both sides (every pair is a hit, the empty ones through zero_need) and threshold
    1.0 (equal strings alone)."""
    left, right = dr.case_zero_and_one()
    base, _ = _check(dev, left, right, (0.0, 1.0))
    assert _pairs(base) == set(itertools.product(range(40), range(40)))
    assert {(i, j) for s, i, j in base if s >= 1.0} == {(i, j) for i, x in enumerate(left) for j, y in enumerate(right) if x == y and x}


def test_drain_between_the_blocks(dev):
    """Four letters, 96 x 161 at threshold 0.5: nearly every lane pushes on every tile.  That more than 128 entries wait at a
    drain check is asserted from the host-side model of the stack, not inferred from the device."""
    left, right = dr.case_four_letters()
    m = dr.Model(left, right, 0.5)
    assert max(m.waiting) > dr.DRAIN_AT
    base, _ = _check(dev, left, right, (0.5, 0.8))
    assert _pairs(base) == set(m.hits()) and len(base) > len(left) * len(right) // 3
