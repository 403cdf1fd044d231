"""The scan of the two-stage RAW fuzzy grid (csrc/indel_raw_coarse.hpp) at the edges of its verdict word.

The scan tests 16 left rows x 2 right tiles per push: one accumulator register per left row carries both tiles in its
16-bit halves, the verdict is the carry into bit 8 + r of the half (r = the row's position in its group of 8), and two
groups share one 32-bit mask.  The strings here make the histogram bound TIGHT, so pairs sit exactly at L1 == limit and
L1 == limit + 1: for x = a^p b^(n-p) and y = a^q b^(m-q), LCS = min(p, q) + min(n - p, m - q) and the L1 distance of the
histograms is |p - q| + |(n - p) - (m - q)| = n + m - 2 LCS.  Every case is compared with the oracle, the one-stage
kernel and the exhaustive kernel, hits bit for bit.
"""
import random

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _ab(n, p):
    return "a" * p + "b" * (n - p)


def _oracle(left, right, thr):
    from oracle import native

    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    return native.indel_raw(cp(left), cp(right), thr, cap=1 << 20)


def _check(dev, left, right, thresholds, base=None):
    """The three kernels against the oracle at every threshold; returns the oracle's hits at the lowest one."""
    from napkon_string_matching_amd import grid, tables

    lt, rt = tables.encode_strings(left, right, dev)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None
    if base is None:
        base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in ({}, {"two_stage": False}, {"prune": False}):
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return base


def _sweep(lengths):
    """Every a^q b^(m-q) of the given lengths."""
    return [_ab(m, q) for m in lengths for q in range(m + 1)]


@pytest.mark.parametrize("n", [16, 40, 64])
def test_every_mask_position(dev, n):
    """37 left rows of ONE length (two full pushes and a tail of 5: every one of the 16 row slots, twice) against right
    rows that sweep q over lengths n - 4 .. n + 4 (more than 128 of them: both tiles of a wave): every left row has
    pairs on both sides of the boundary in both tiles."""
    left = [_ab(n, (7 * k) % (n + 1)) for k in range(37)]
    right = _sweep(range(n - 4, min(64, n + 4) + 1))
    random.Random(n).shuffle(right)
    assert len(right) > 128
    base = _check(dev, left, right, (0.5, 0.8))
    for thr in (0.5, 0.8):
        per_row = [0] * len(left)
        for s, i, _ in base:
            per_row[i] += s >= thr
        assert all(0 < c < len(right) for c in per_row)  # every row slot holds hits and misses


# length classes of 33, 17, 9, 1 (+ 4: the first 64-row chunk ends with a class) and 16, 15, 8, 7 rows: partial first
# group, partial second group, an exactly full push, pushes plus a tail
_TAIL_CLASSES = ((40, 33), (39, 17), (38, 9), (37, 1), (36, 4), (35, 16), (34, 15), (33, 8), (32, 7))


@pytest.fixture(scope="module")
def tail_case():
    left = [_ab(n, (5 * k + n) % (n + 1)) for n, size in _TAIL_CLASSES for k in range(size)]
    right = _sweep(range(30, 43))
    random.Random(77).shuffle(right)
    right = right[:200]
    return left, right, _oracle(left, right, 0.5)


@pytest.mark.parametrize("n_right", [1, 64, 65, 128, 129, 200])
def test_tails(dev, tail_case, n_right):
    """Length classes of 1, 7, 8, 9, 15, 16, 17 and 33 left rows; right rows that end a tile early, fill one or two
    tiles exactly, or start a second wave (invalid lanes, a missing second tile)."""
    left, right, base = tail_case
    # (a right table of the first n_right rows keeps their indices: the oracle's hits are filtered, not recomputed)
    _check(dev, left, right[:n_right], (0.5, 0.8), base=[h for h in base if h[2] < n_right])


def test_bias_range(dev):
    """The seeds at both ends of their range.  Threshold 0: limit = la + lb (128 for two 64-unit strings: the smallest
    seed), every pair a hit, empty strings on both sides; threshold 1: limit = 0."""
    left = [_ab(64, (9 * k) % 65) for k in range(20)] + ["", _ab(3, 1), ""]
    right = [_ab(64, q) for q in range(65)] + ["", "", _ab(3, 1), _ab(5, 5)]
    base = _check(dev, left, right, (0.0, 1.0))
    assert len(base) == len(left) * len(right)


def test_cannot_fit_beside_a_hit(dev):
    """limit = -1 (min(la, lb) < need: the largest seed, the verdict bit set before any SAD) in one half of a register
    whose other half holds a hit -- in the low half (a carry out of it would flip tile 1's verdict) and in the high
    half.  Right rows are sorted by length: tile 0 = 64 rows of 64 units, tile 1 = 32 rows of 40 and 32 rows of 8, so
    a left row of 64 units hits in tile 0 only, one of 40 or 8 units in tile 1 only."""
    left = [_ab(64, (9 * k) % 65) for k in range(16)] + [_ab(40, (3 * k) % 41) for k in range(16)] + [_ab(8, k % 9) for k in range(16)]
    right = [_ab(64, q) for q in range(64)] + [_ab(40, q) for q in range(32)] + [_ab(8, q % 9) for q in range(32)]
    base = _check(dev, left, right, (0.8,))
    lens = {len(left[i]) for _, i, _ in base}
    assert lens == {64, 40, 8} and all(len(left[i]) == len(right[j]) for _, i, j in base)


def test_stack_pressure(dev):
    """A 2-letter alphabet at threshold 0.3: most bits of most entries are set, so entries go back on the stack up to 32
    times and the drain runs between pushes."""
    rng = random.Random(31)
    rand = lambda n: ["".join(rng.choice("ab") for _ in range(rng.randint(0, 64))) for _ in range(n)]
    left, right = rand(600), rand(300)
    base = _check(dev, left, right, (0.3,))
    assert len(base) > len(left) * len(right) // 2
