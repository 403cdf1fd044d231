"""The value-table codes of the packed FP4 scan of the two-stage RAW kernel (csrc/indel_raw_coarse.hpp, NSM_C3C_CODES2): slots
3 and 4 of a bucket are FP4 value tables on both sides, the bound D is a multiple of 1/4, and the OR fold keeps 4 D in 11-bit
fields.

What can go wrong: a table entry that is too small (the code is no upper bound), the two slots in each other's nibble on one
side, a left count above 15 that does not saturate, a scaled right string's table index or its scale byte, a field or a flag
bit in the wrong place.  The scan is a filter, so a fault shows as a LOST hit, and only where nothing else in the lane passes:
the cases keep the rows and the columns that hit sparse.

The strings are sorted runs over at most 32 symbols (one bucket each: LCS = sum of min).  The packed call, the unpacked call,
the library's own choice, the one-stage kernel and the oracle are compared bit for bit.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

SYMS = "".join(sorted("abcdefghijklmnopqrstuvwxyzABCDEF"))  # 32 symbols, ascending: bucket = position
VARIANTS = ({"pack": True}, {"pack": False}, {}, {"two_stage": False})


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _runs(counts):
    assert len(counts) == 32
    return "".join(s * a for s, a in zip(SYMS, counts))


def _oracle(left, right, thr):
    from oracle import native

    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    return native.indel_raw(cp(left), cp(right), thr, cap=1 << 22)


def _check(dev, left, right, thresholds, in_order=False):
    """Every variant against the oracle at every threshold; returns the oracle's hits at the lowest one."""
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd import tables as tb

    lt, rt = tb.encode_strings(left, right, dev)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None and lt.alphabet <= 32
    if in_order:  # (built in table order: longest first, equal lengths as given)
        assert lt.orig.cpu().tolist() == list(range(len(left))) and rt.orig.cpu().tolist() == list(range(len(right)))
    base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in VARIANTS:
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return base


def _d(a, r):
    """The packed scan's bound of a pair of histograms (tests/support/scan_codes2.py)."""
    from tests.support import scan_codes2 as c2

    return c2.bound(a, r)


def _need(thr, la, lb):
    from tests.support import drain_rows as dr

    return dr.need_of(thr, la, lb)


def _with_count(bucket, count, length=64):
    """`count` units in `bucket` and the rest of `length` spread over the other buckets, two each from the bucket after it."""
    counts = [0] * 32
    counts[bucket] = count
    todo, b = length - count, bucket
    while todo > 0:
        b = (b + 1) % 32
        assert b != bucket
        counts[b] = min(2, todo)
        todo -= counts[b]
    return counts


# --- 1. table sizes and class sizes -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_right", [1, 33, 129])
def test_table_and_class_sizes(dev, n_right):
    """Right tables of 1, 33 and 129 rows against left length classes of 65, 33, 32, 31 and 1 rows, packed by force among
    the variants.  Every string has eight buckets of 4 to 7 units, so every pair meets the value tables.  Left row i is near
    right string i mod n_right.  At threshold 0 every pair that exists is a hit and no pair with a column that does not
    exist is."""
    rng = random.Random(1500 + n_right)
    rights = []
    for _ in range(n_right):
        counts = [0] * 32
        for s in rng.sample(range(32), 8):
            counts[s] = 5
        rights.append(counts)
    left, mates = [], []
    for length, n_rows in ((44, 65), (43, 33), (42, 32), (41, 31), (39, 1)):
        for _ in range(n_rows):
            j = len(left) % n_right
            counts = list(rights[j])
            used = [s for s in range(32) if counts[s]]
            for u in range(abs(length - 40)):
                counts[used[(u * 3) % 8]] += 1 if length > 40 else -1
            left.append(_runs(counts))
            mates.append(j)
            assert len(left[-1]) == length
    base = _check(dev, left, list(map(_runs, rights)), (0.0, 0.8, 1.0), in_order=True)
    assert len(base) == 162 * n_right
    assert {(i, j) for s, i, j in base if s >= 0.8} >= set(enumerate(mates))


# --- 2. real hits on large counts ------------------------------------------------------------------------------------------------

_COUNTS = (3, 4, 5, 6, 8, 13, 16, 17, 39, 40, 64)
_BUCKETS = (0, 15, 16, 31)  # the first and the last byte of both lane halves
_ROWS = (0, 3, 4, 31)


def test_hits_on_large_counts(dev):
    """Case n = (count, bucket): a 64-unit string with `count` units in `bucket` and at most two in every other, as row
    _ROWS[n % 4] of left block n and as column n // 4 of right tile n % 4; every other row and column is far from all of them.
    At threshold 1.0 the pair needs D = 64 and every other bucket gives its minimum exactly, so a bucket bound below the count
    loses the hit.  Counts above 15 carry a scale on the right and saturate on the left."""
    from tests.support import scan_fp4 as fp4

    far_l = _runs([32 if b in (7, 23) else 0 for b in range(32)])
    far_r = _runs([13 if b in (8, 9, 10, 11) else 12 if b == 12 else 0 for b in range(32)])
    cases = [(c, b) for c in _COUNTS for b in _BUCKETS]
    left, right, want = [], [far_r] * 128, []
    for n, (c, b) in enumerate(cases):
        counts = _with_count(b, c)
        assert sum(counts) == 64 and fp4.scale_of(counts) == (0 if c <= 15 else 1 if c <= 27 else 2 if c <= 51 else 3)
        assert _d(counts, counts) >= 64
        block = [far_l] * 32
        block[_ROWS[n % 4]] = _runs(counts)
        col = 32 * (n % 4) + n // 4
        right[col] = _runs(counts)
        want.append((len(left) + _ROWS[n % 4], col))
        left += block
    assert {n % 4 for n in range(len(cases))} == {0, 1, 2, 3} and {_ROWS[n % 4] for n in range(len(cases))} == set(_ROWS)
    base = _check(dev, left, right, (0.8, 1.0), in_order=True)
    assert {(i, j) for s, i, j in base if s >= 1.0} == set(want)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_hits_on_large_counts_in_every_tile(dev, shift):
    """The same cases with tile and row position turned by `shift`: with the test above every case meets every tile and every
    row position."""
    far_l = _runs([32 if b in (7, 23) else 0 for b in range(32)])
    far_r = _runs([13 if b in (8, 9, 10, 11) else 12 if b == 12 else 0 for b in range(32)])
    cases = [(c, b) for c in _COUNTS for b in _BUCKETS]
    left, right, want = [], [far_r] * 128, []
    for n, (c, b) in enumerate(cases):
        counts = _with_count(b, c)
        block = [far_l] * 32
        row, tile = _ROWS[(n + shift) % 4], (n + shift) % 4
        block[row] = _runs(counts)
        col = 32 * tile + n // 4
        right[col] = _runs(counts)
        want.append((len(left) + row, col))
        left += block
    base = _check(dev, left, right, (1.0,), in_order=True)
    assert {(i, j) for _, i, j in base} == set(want)


# --- 3. on the need, one below it, and a bound on the need above an LCS below it ---------------------------------------------


def _move(counts, down, up):
    out = list(counts)
    out[down] -= 1
    out[up] += 1
    return out


def test_on_need_one_below_and_bound_on_need(dev):
    """60-unit strings at threshold 0.8: need 48.  Left row A = twelve buckets of 5.  Columns, in lanes of their own in
    every tile: a right string with sum of min = 48 (a hit), one with 47 (no hit), and one whose sum of min is below 48 while
    the scan's bound is exactly 48: it passes the scan, and the drain's exact test has to drop it."""
    thr = 0.8
    assert _need(thr, 60, 60) == 48
    a = [5] * 12 + [0] * 20
    on = [4] * 12 + [0] * 8 + [1] * 12                    # sum of min 48
    below = _move(on, 0, 20)                              # 47
    assert sum(map(min, a, on)) == 48 and sum(map(min, a, below)) == 47 and sum(on) == sum(below) == 60
    # bound on the need, LCS below: buckets of 6 against 5 give 5 + 1/2 . 2 ... searched, not guessed
    rng = random.Random(77)
    tight = None
    for _ in range(20000):
        r = [rng.choice((0, 3, 4, 6, 7, 8)) for _ in range(12)] + [0] * 20
        rest = 60 - sum(r)
        if not 0 <= rest <= 40:
            continue
        for b in range(12, 32):
            r[b] = min(2, rest)
            rest -= r[b]
        if rest == 0 and _d(a, r) == 48 and sum(map(min, a, r)) < 48:
            tight = r
            break
    assert tight is not None
    far_l = _runs([30 if b in (30, 31) else 0 for b in range(32)])
    far_r = _runs([15 if b in (26, 27, 28, 29) else 0 for b in range(32)])
    left = [far_l] * 64
    left[3], left[32 + 31] = _runs(a), _runs(a)
    right, want = [far_r] * 128, []
    for t in range(4):
        right[32 * t + 2 + t], right[32 * t + 9 + t], right[32 * t + 20 + t] = _runs(on), _runs(below), _runs(tight)
        want += [(3, 32 * t + 2 + t), (63, 32 * t + 2 + t)]
    base = _check(dev, left, right, (thr,), in_order=True)
    assert sorted((i, j) for _, i, j in base) == sorted(want)


# --- 4. block scales --------------------------------------------------------------------------------------------------------


def test_scaled_right_strings(dev):
    """Right strings with k = 1, 2 and 3 among ordinary ones in tiles 0 and 1, tile 2 of nothing but scaled strings, tile 3
    ordinary; every string 64 units, each scaled string against its own copy on the left."""
    from tests.support import scan_fp4 as fp4

    shapes = ((16, 16, 16, 16), (28, 28, 8), (52, 12), (27, 20, 17), (51, 7, 6), (64,))
    far_l = _runs([32 if b in (30, 31) else 0 for b in range(32)])
    far_r = _runs([13] * 4 + [12] + [0] * 27)
    left, right, want = [far_l] * 64, [far_r] * 128, []

    def plant(col, shape, at, row):
        counts = [0] * 32
        for n, c in enumerate(shape):
            counts[(at + 5 * n) % 30] = c  # (buckets 30 and 31 are the far rows')
        assert sum(counts) == 64 and fp4.scale_of(counts) >= 1
        right[col] = _runs(counts)
        if row is not None:
            left[row] = _runs(counts)
            want.append((row, col))

    for tile in (0, 1):
        for n, shape in enumerate(shapes):
            plant(32 * tile + 1 + 2 * n, shape, 3 * n + tile, 32 * tile + 5 * n + tile)
    for c in range(32):  # a tile of only scaled strings; six of them have their copy on the left
        shape = shapes[c % 6]
        plant(64 + c, shape, c, 26 + c if c < 6 else None)
    base = _check(dev, left, right, (0.8, 1.0), in_order=True)
    exact = {(i, j) for s, i, j in base if s >= 1.0}
    assert exact >= set(want)


# --- 5. a stack that fills, and a captured call -------------------------------------------------------------------------------


def test_four_letters(dev):
    """A 4-letter alphabet (counts around 10 in four buckets), 96 left rows of one length x 161 right rows at threshold 0:
    every lane of every tile pair pushes both its entries; 0.8 and 1.0 ride along."""
    rng = random.Random(1962)
    word = lambda n: "".join(rng.choice("abcd") for _ in range(n))
    left = [word(40) for _ in range(96)]
    right = [word(rng.randint(24, 64)) for _ in range(150)] + left[:11]
    base = _check(dev, left, right, (0.0, 0.8, 1.0))
    assert len(base) == 96 * 161 and sum(s >= 1.0 for s, _, _ in base) >= 11


def test_captured_call(dev):
    """The scan on a stream that is being captured (it never packs): the graph replays to the eager call's hits."""
    import torch

    from napkon_string_matching_amd import _lib, grid
    from napkon_string_matching_amd import tables as tb

    rng = random.Random(16)

    def word():  # counts of 4 to 6 among small ones: the value tables' entries
        while True:
            w = _runs([rng.choice((0, 0, 0, 0, 1, 2, 4, 5, 6)) for _ in range(32)])
            if 0 < len(w) <= 64:
                return w

    left = [word() for _ in range(70)]
    right = left[:20] + [word() for _ in range(109)]
    lt, rt = tb.encode_strings(left, right, dev)
    lib = _lib.load()
    want = grid.indel_raw_grid(lt, rt, 0.8, pack=True).as_tuples()
    assert want == _oracle(left, right, 0.8) and len(want) >= 20

    def launch(buf, stream):
        buf.count.zero_()
        _lib.check(lib.nsm_indel_raw_grid(lt.struct(), rt.struct(), 0.8, _lib.FLAG_PRUNE, buf.records.data_ptr(), buf.capacity,
                                          buf.count.data_ptr(), stream.cuda_stream), "nsm_indel_raw_grid")

    def hits_of(buf):
        return grid.sort_hits_device(buf, int(buf.count.item())).as_tuples()

    stream = torch.cuda.Stream(dev)
    buf = grid.HitBuffer(1 << 12, dev)
    buf.reset()
    with torch.cuda.stream(stream):
        launch(buf, stream)
        stream.synchronize()
        assert hits_of(buf) == want
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            launch(buf, stream)
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize(dev)
            assert hits_of(buf) == want
