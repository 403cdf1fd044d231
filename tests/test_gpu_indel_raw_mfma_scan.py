"""The matrix-pipe scan of the two-stage RAW fuzzy grid (csrc/indel_raw_coarse.hpp) at the edges of its filter.

The scan decides 32 left rows x 32 right strings per tile with CAP chained i8 MFMAs over thermometer codes of the
32-bucket histograms: D = sum over buckets of min(a, r) where r < CAP and of a where r >= CAP, and a pair goes on when
D >= need.  The strings here are SORTED RUNS, c0^a0 c1^a1 ... with ascending symbols: their LCS is exactly
sum_c min(a_c, r_c), so with at most 32 distinct symbols the filter is tight wherever r_c < CAP or a_c <= r_c, and a
right row whose length grows one unit at a time (a filler symbol of its own, which adds to lb and nothing to the LCS)
walks a pair across the threshold.  Where a > r >= CAP the bound is loose (the bucket gives a), so rows that lack a
symbol altogether are mixed in: the test computes D and need itself and asserts where D == need and D == need - 1 sit.
Every case is compared with the oracle, the one-stage kernel and the exhaustive kernel, hits bit for bit.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

# 40 symbols in ascending order; the first 8 are the "core" of the run strings, "y" and "z" are fillers
SYMS = "".join(sorted("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMN"))
CORE = "abcdefgh"


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _runs(counts, syms=CORE, tail=""):
    """c0^a0 c1^a1 ... (symbols ascending), then ``tail`` (symbols above every one of ``syms``)."""
    return "".join(s * a for s, a in zip(syms, counts)) + tail


def _oracle(left, right, thr):
    from oracle import native

    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    return native.indel_raw(cp(left), cp(right), thr, cap=1 << 20)


def _check(dev, left, right, thresholds, base=None, tables=False):
    """The three kernels against the oracle at every threshold; returns the oracle's hits at the lowest one."""
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd import tables as tb

    lt, rt = tb.encode_strings(left, right, dev)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None
    if base is None:
        base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in ({}, {"two_stage": False}, {"prune": False}):
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return ((base, lt), rt) if tables else (base, lt)


def _left_rows(c, n, seed):
    """n rows of ONE length 8 c: every core symbol c times, but one symbol c + 1 and another c - 1."""
    rng = random.Random(seed)
    rows = []
    for _ in range(n):
        counts = [c] * 8
        up, down = rng.sample(range(8), 2)
        counts[up] += 1
        counts[down] -= 1
        rows.append(_runs(counts))
    return rows


def _right_rows(c, n, seed):
    """Right rows with core counts c - 1, c, c + 1 (up to two symbols off c) and a filler run of 0..24 units (fewer where
    the row would pass 64 units): every 32 consecutive rows (one tile) hold every filler length, so against every left
    row the tile's pairs step across the threshold one unit of lb at a time."""
    rng = random.Random(seed)
    rows = []
    for j in range(n):
        counts = [c] * 8
        for s in rng.sample(range(8), j % 3):
            counts[s] += rng.choice((-1, 1))
        rows.append(_runs(counts, tail="z" * min((j * 7) % 32 % 25, 64 - sum(counts))))
    return rows


def _need(thr, s):
    """The smallest LCS with which strings of la + lb = s reach ``thr`` (csrc/indel_score.hpp, the same doubles), or None."""
    for lcs in range(s // 2 + 1):
        if (1.0 - float(s - 2 * lcs) / float(s)) * 100.0 / 100.0 >= thr:
            return lcs
    return None


def _dot(x, y, cap):
    """The scan's D of a pair (at most 32 distinct symbols: one bucket each)."""
    return sum(min(x.count(ch), y.count(ch)) if y.count(ch) < cap else x.count(ch) for ch in set(x))


def _boundary_cover(left, right, l_order, r_order, thresholds=(0.5, 0.8)):
    """Where the pairs with D == need and with D == need - 1 sit (among those the length filter lets through), per CAP:
    {(cap, kind)} -> (set of left block positions, set of tiles of a wave).  ``l_order`` / ``r_order``: the tables' rows as
    indices into ``left`` / ``right`` (one left length class from row 0 of one chunk: block position = row & 31)."""
    cover = {(cap, k): (set(), set()) for cap in (3, 4) for k in (0, 1)}
    for pi, i in enumerate(l_order):
        for pj, j in enumerate(r_order):
            x, y = left[i], right[j]
            for thr in thresholds:
                need = _need(thr, len(x) + len(y))
                if need is None or min(len(x), len(y)) < need:
                    continue
                for cap in (3, 4):
                    k = need - _dot(x, y, cap)
                    if k in (0, 1):
                        cover[cap, k][0].add(pi & 31)
                        cover[cap, k][1].add((pj >> 5) & 3)
    return cover


def _right_rows_thin(c, n, seed):
    """Like ``_right_rows``, but one or two core symbols are missing (r = 0 < CAP: the bucket gives min(a, 0) = 0, so D
    falls below la and can sit one short of need even where every other count is >= CAP), and the filler run is as long
    as puts need = ceil(0.4 (la + lb)) at the D of a left row with every count at c, or one above it, give or take a
    unit: against the left rows (whose D differs by the one unit they are off c) these rows sit on both sides of the
    boundary at threshold 0.8 whatever their place in the table."""
    rng = random.Random(seed)
    rows = []
    for j in range(n):
        counts = [c] * 8
        for s in rng.sample(range(8), j % 3):
            counts[s] += rng.choice((-1, 1))
        missing = rng.sample(range(8), 1 + j % 2)
        for s in missing:
            counts[s] = 0
        d = 8 * c - c * len(missing)
        lb = int((d + (j // 2) % 2) / 0.4) - 8 * c + (j // 4) % 3 - 1
        rows.append(_runs(counts, tail="z" * max(0, min(lb, 64) - sum(counts))))
    return rows


def _position_case(c):
    left = _left_rows(c, 65, c)
    right = _right_rows(c, 65, 100 + c) + _right_rows_thin(c, 192, 300 + c)
    random.Random(c).shuffle(right)
    return left, right


@pytest.mark.parametrize("c", [2, 3, 4, 5])
def test_every_block_position(dev, c):
    """65 left rows of one length (two full blocks and a block of one row) against 257 right rows (two waves and a third
    with one string), per-symbol counts at c - 1, c and c + 1 on both sides (c = 2..5: CAP - 1, CAP and CAP + 1 for CAP 3
    and 4).  D and need are computed here for every pair, in the tables' own row order: for both caps, pairs with
    D == need and pairs with D == need - 1 sit in every one of the 32 row positions of a block (both lane halves) and in
    every tile of a wave."""
    left, right = _position_case(c)
    (base, lt), rt = _check(dev, left, right, (0.5, 0.8), tables=True)
    assert len(set(map(len, left))) == 1
    cover = _boundary_cover(left, right, lt.orig.cpu().tolist(), rt.orig.cpu().tolist())
    for (cap, k), (positions, tiles) in cover.items():
        assert positions == set(range(32)), f"cap {cap}, D == need - {k}: left positions {sorted(positions)}"
        assert tiles == set(range(4)), f"cap {cap}, D == need - {k}: tiles {sorted(tiles)}"


# left length classes of 65, 33, 32, 31 and 1 rows (lengths 40, 32, 24, 16 and 17), an empty string at the end
_CLASSES = ((5, 65, 0), (4, 33, 0), (3, 32, 0), (2, 31, 0), (2, 1, 1))


@pytest.fixture(scope="module")
def sizes_case():
    left = []
    for c, size, extra in _CLASSES:
        left += [row + "y" * extra for row in _left_rows(c, size, 10 * c + size)]
    left.append("")
    right = []
    for c in (2, 3, 4, 5):
        right += _right_rows(c, 64, 200 + c)
    random.Random(5).shuffle(right)
    right = right[:30] + [""] + right[30:]  # (an empty string inside the one-tile tables too)
    assert len(right) == 257
    return left, right, _oracle(left, right, 0.0)


@pytest.mark.parametrize("n_right", [1, 31, 32, 33, 127, 128, 129, 257])
def test_sizes(dev, sizes_case, n_right):
    """Length classes of 1, 31, 32, 33 and 65 left rows (a last block of 1, 31, 32 rows; one and two blocks before it)
    against right tables that end a tile early, fill tiles and waves exactly or start the next one, at every threshold;
    an empty string on each side (zero_need at threshold 0.0, where every pair is a hit)."""
    left, right, base = sizes_case
    # (a right table of the first n_right rows keeps their indices: the oracle's hits are filtered, not recomputed)
    _check(dev, left, right[:n_right], (0.0, 0.5, 0.8, 1.0), base=[h for h in base if h[2] < n_right])
    assert sum(1 for h in base if h[2] < n_right) == len(left) * n_right


def test_more_than_32_symbols(dev):
    """Run strings over 37 symbols: codes 32..36 share the buckets of codes 0..4, so D over-counts there and the exact
    32-bucket test and the LCS have to drop what the scan lets through."""
    rng = random.Random(37)
    syms = SYMS[:37]

    def row():
        counts = [0] * 37
        for s in rng.sample(range(37), rng.randint(4, 14)):
            counts[s] = rng.randint(1, 5)
        return _runs(counts, syms)

    left = [row() for _ in range(100)]
    right = []
    for k in range(150):  # a left row with some runs changed
        counts = [left[k % 100].count(s) for s in syms]
        for s in rng.sample(range(37), k % 7):
            counts[s] = max(0, counts[s] + rng.choice((-2, -1, 1, 2)))
        if sum(counts) <= 64:
            right.append(_runs(counts, syms))
    base, lt = _check(dev, left, right, (0.5, 0.8, 1.0))
    assert lt.alphabet > 32
    assert 0 < sum(1 for h in base if h[0] >= 0.8) < len(base) < len(left) * len(right)


def test_stack_pressure(dev):
    """A 4-letter alphabet at threshold 0.5: most pairs pass the scan and the exact test, entries carry many bits and go
    back on the stack up to 16 times, and the drain runs between the blocks."""
    rng = random.Random(31)
    rand = lambda n: ["".join(rng.choice("abcd") for _ in range(rng.randint(0, 64))) for _ in range(n)]
    left, right = rand(600), rand(300)
    base, _ = _check(dev, left, right, (0.5,))
    assert len(base) > len(left) * len(right) // 3
