"""The OR fold of the FP4 scan of the two-stage RAW kernel (csrc/indel_raw_coarse.hpp, NSM_C3C_ORFOLD): tiles 2 p and 2 p + 1
of a wave share one accumulator as two 9-bit fields on a bias that holds the lane's needs, the fold is an OR on the fields'
flag bits, and the push decodes the two flags into entries for the two tiles.

What can go wrong: the B scale of the even tile (a field in the wrong place), the two flags' tiles in each other's place,
a lane's need taken from the wrong tile or parity (one bias serves the lane's four columns: it has to be the SMALLEST need
of a parity), a carry between the fields, a column that does not exist taken for an empty string, the stack with 128 pushes
a tile pair.  The scan is a filter, so a fault shows as a LOST hit, and only where nothing else in the lane passes: the
cases keep the rows and the columns that hit sparse.

The strings are sorted runs over at most 32 symbols (one bucket each: LCS = sum of min).  The packed call, the unpacked
call, the library's own choice, the one-stage kernel and the oracle are compared bit for bit.
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
    """The scan's bound of a pair of histograms (tests/support/scan_fp4.py)."""
    from tests.support import scan_fp4 as fp4

    k = fp4.scale_of(r)
    return sum(fp4.bucket(x, y, k) for x, y in zip(a, r))


def _need(thr, la, lb):
    from tests.support import drain_rows as dr

    return dr.need_of(thr, la, lb)


def _moved(counts, rng):
    """One unit in another bucket that the string already uses (its set of symbols stays)."""
    out = list(counts)
    used = [s for s in range(32) if out[s] > 0]
    down = rng.choice(used)
    up = rng.choice([s for s in used if s != down])
    out[down] -= 1
    out[up] += 1
    return out


# --- 1. table sizes and class sizes -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_right", [1, 33, 65, 129])
def test_table_and_class_sizes(dev, n_right):
    """Right tables of 1, 33, 65 and 129 rows: no odd tile, a short odd tile, a short third tile whose partner does not
    exist, and two waves.  Left length classes of 65, 33, 32, 31 and 1 rows, 162 rows in chunks of 64: the class of 65 ends
    on the first row of the second chunk.  Left row i is near right string i mod n_right and far from every other.  At
    threshold 0 every pair that exists is a hit and no pair with a column that does not exist is."""
    rng = random.Random(700 + n_right)
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
                counts[used[u % 8]] += 1 if length > 40 else -1
            left.append(_runs(_moved(counts, rng)))
            mates.append(j)
            assert len(left[-1]) == length
    base = _check(dev, left, list(map(_runs, rights)), (0.0, 0.8, 1.0), in_order=True)
    assert len(base) == 162 * n_right
    assert {(i, j) for s, i, j in base if s >= 0.8} >= set(enumerate(mates))


# --- 2. a pair on its need and the pair one below it, by tile and by row of the block -------------------------------------------

_ROWS = (0, 3, 4, 31)
_WHERE = ("even", "odd", "both")


def _two_each(n):
    """63 units, no count above 3 (the bound is exact): 2 in every bucket but bucket n, 1 there."""
    counts = [2] * 32
    counts[n] = 1
    return counts


def test_on_need_and_one_below_by_tile_and_row(dev):
    """One left length class of 63 units in blocks of 32 rows, 31 of them far from everything, and 128 right strings of 63
    units, which keep their order: lane c of the wave has columns c, 32 + c, 64 + c and 96 + c.  Case n (a row position of
    0, 3, 4 or 31 x the copy in an even tile only, in an odd tile only, or in both) has its row in block n and its copies in
    lane n, the copies with one unit elsewhere (one below the need at threshold 1.0) in lane n + 16.  Nothing else of the
    lane passes, so a flag that is lost, read for the wrong tile or pushed for the wrong tile loses the hit."""
    far = _runs([31 if b == 8 else 32 if b == 24 else 0 for b in range(32)])
    filler = _runs([12 if b in (1, 5, 11, 17, 29) else 3 if b == 30 else 0 for b in range(32)])
    left, right, on_need = [], [filler] * 128, []
    cases = [(r, w) for w in _WHERE for r in _ROWS]
    for n, (r, where) in enumerate(cases):
        counts = _two_each(n)
        below = list(counts)
        below[(n + 1) % 32] -= 1
        below[(n + 2) % 32] += 1
        assert _d(counts, counts) == 63 == _need(1.0, 63, 63) and _d(counts, below) == 62
        block = [far] * 32
        block[r] = _runs(counts)
        tiles = {"even": (2 * (n & 1),), "odd": (1 + 2 * (n & 1),), "both": (2 * (n & 1), 3 - 2 * (n & 1))}[where]
        for t in tiles:
            right[32 * t + n] = _runs(counts)
            right[32 * t + n + 16] = _runs(below)
            on_need.append((len(left) + r, 32 * t + n))
        left += block
    assert all(len(x) == 63 for x in left + right)
    base = _check(dev, left, right, (0.95, 1.0), in_order=True)
    exact = {(i, j) for s, i, j in base if s >= 1.0}
    assert exact == set(on_need) and len(on_need) == 16
    # (at 0.95 the copies with a unit elsewhere, and the cases' rows among each other, are hits too: one below the need at 1.0)
    assert all((i, j + 16) in {(a, b) for _, a, b in base} for i, j in on_need)


# --- 3. the carry guard -----------------------------------------------------------------------------------------------------

_BIG = [52 if b == 0 else 4 if b in (1, 2, 3) else 0 for b in range(32)]  # 64 units, against itself D = 128
_IN = {0: 15, 1: 4, 2: 4, 3: 4}                                          # 27 units inside _BIG: D = LCS = 27
_ON = [_IN.get(b, {10: 15, 11: 15, 12: 7}.get(b, 0)) for b in range(32)]  # ... in a string of 64
_BELOW = [3 if b == 1 else {10: 15, 11: 15, 12: 8}.get(b, _IN.get(b, 0)) for b in range(32)]  # 26 inside (an excess of 11 would round up)
_THR = 0.42  # two strings of 64 units: need 27


@pytest.mark.parametrize("big_tile", [0, 1])
def test_carry_guard(dev, big_tile):
    """Two identical 64-unit strings with the largest bound there is, D = 128, in one tile of a pair (lanes 5 and 6), and in
    the lane's other tile the same row exactly on its need (lane 5) and one below it (lane 6): the largest field beside a
    flag that one unit decides, in the even tile beside the odd one and the other way round.  Every string has 64 units, so
    the right table keeps its order."""
    assert sum(_BIG) == sum(_ON) == sum(_BELOW) == 64
    assert _d(_BIG, _BIG) == 128
    assert _d(_BIG, _ON) == 27 == _need(_THR, 64, 64) and _d(_BIG, _BELOW) == 26
    left = [_runs([32 if b in (20, 21) else 0 for b in range(32)])] * 32
    left[9] = _runs(_BIG)
    far = _runs([32 if b in (26, 27) else 0 for b in range(32)])
    big, small = [far] * 32, [far] * 32
    big[5] = big[6] = _runs(_BIG)
    small[5], small[6] = _runs(_ON), _runs(_BELOW)
    right = big + small if big_tile == 0 else small + big
    base = _check(dev, left, right, (_THR, 0.8), in_order=True)
    on = 32 * (1 - big_tile) + 5
    assert {(i, j) for _, i, j in base} == {(9, 32 * big_tile + 5), (9, 32 * big_tile + 6), (9, on)}


# --- 4. one bias for four columns ---------------------------------------------------------------------------------------------


def _partner(a, lb, common):
    """A right histogram of lb units that shares exactly `common` units with `a` (sum of min): buckets 0 and 1 take a's
    counts and all the units beyond the common ones, the other common units come from bucket 2 on."""
    r, todo = [0] * 32, common
    for b in range(32):
        r[b] = min(a[b], todo)
        todo -= r[b]
    assert todo == 0 and r[0] == a[0] and r[1] == a[1]
    extra = lb - common
    r[0] += extra // 2
    r[1] += extra - extra // 2
    assert sum(r) == lb and max(r) <= 15 and sum(map(min, a, r)) == common
    return r


def test_four_lengths_in_a_wave(dev):
    """A wave whose tiles hold right strings of 60, 50, 40 and 12 units, and left classes of 56 and 44 units.  The last
    tile fits neither class (kNever beside a column that fits), and the need of the class of 56 is 47, 43 and 39 in the
    others: the bias of a lane holds 39 for its even tiles, looser than the 47 of tile 0, and 43 for its odd ones.  Pairs
    exactly on their own need in tile 0 (lane 3), tile 1 (lane 4) and tile 2 (lanes 5 and 7, lane 7 with a pair one below
    its need in tile 0); a need taken as the LARGEST of the parity, or the odd tiles' for both fields, loses those of tile 2."""
    thr = 0.8
    a56 = [2] * 24 + [1] * 8
    a44 = [2] * 12 + [1] * 20
    lengths = (60, 50, 40, 12)
    need56 = [_need(thr, 56, lb) for lb in lengths[:3]]
    assert need56 == [47, 43, 39] and _need(thr, 56, 12) > 12 and _need(thr, 44, 12) > 12
    fillers = [[15] * (lb // 15) + [lb % 15] + [0] * 32 for lb in lengths]
    right = [[_runs([0] * 12 + f[:20]) for _ in range(32)] for f in fillers]  # buckets 12 ..: away from 0, 1, 8 and 24
    want = []

    def plant(tile, lane, a, row, common, hit):
        right[tile][lane] = _runs(_partner(a, lengths[tile], common))
        if hit:
            want.append((row, 32 * tile + lane))

    plant(0, 3, a56, 2, need56[0], True)
    plant(1, 4, a56, 2, need56[1], True)
    plant(2, 5, a56, 2, need56[2], True)
    plant(2, 7, a56, 2, need56[2], True)
    plant(0, 7, a56, 2, need56[0] - 1, False)
    plant(1, 9, a44, 32 + 30, _need(thr, 44, 50), True)
    plant(2, 9, a44, 32 + 30, _need(thr, 44, 40) - 1, False)
    far56 = _runs([28 if b in (8, 24) else 0 for b in range(32)])
    far44 = _runs([22 if b in (8, 24) else 0 for b in range(32)])
    left = [far56] * 32 + [far44] * 32
    left[2], left[32 + 30] = _runs(a56), _runs(a44)
    base = _check(dev, left, [x for tile in right for x in tile], (thr,), in_order=True)
    assert sorted((i, j) for _, i, j in base) == sorted(want)


# --- 5. block scales on either tile -------------------------------------------------------------------------------------------


def test_scaled_right_strings_in_both_tiles(dev):
    """Right strings with k = 1, 2 and 3 in an even tile (lanes 1, 2, 3) and in an odd one (lanes 4, 5, 6), every string 64
    units, each against its own copy on the left: the scale byte of the even tile carries 2^9 AND 2^k."""
    from tests.support import scan_fp4 as fp4

    shapes = ((16, 16, 16, 16), (28, 28, 8), (52, 12))
    far_l = _runs([32 if b in (30, 31) else 0 for b in range(32)])
    far_r = _runs([13] * 4 + [12] + [0] * 27)
    left, right, want = [far_l] * 32, [far_r] * 64, []
    for tile in (0, 1):
        for k, shape in enumerate(shapes, start=1):
            counts = [0] * 32
            for n, c in enumerate(shape):
                counts[5 + 8 * tile + 4 * (k - 1) // 2 + n + 4 * (k - 1)] = c
            assert sum(counts) == 64 and fp4.scale_of(counts) == k
            lane = 3 * tile + k
            right[32 * tile + lane] = _runs(counts)
            left[4 * lane] = _runs(counts)
            want.append((4 * lane, 32 * tile + lane))
    base = _check(dev, left, right, (0.8, 1.0), in_order=True)
    assert {(i, j) for s, i, j in base if s >= 1.0} == set(want)


# --- 6. a stack that fills, and a captured call -------------------------------------------------------------------------------


def test_four_letters(dev):
    """A 4-letter alphabet, 96 left rows of one length x 161 right rows at threshold 0: every lane of every tile pair
    pushes both its entries, 128 a pair, and the stack fills in the middle of the class; 0.8 and 1.0 ride along."""
    rng = random.Random(962)
    word = lambda n: "".join(rng.choice("abcd") for _ in range(n))
    left = [word(40) for _ in range(96)]
    right = [word(rng.randint(24, 64)) for _ in range(150)] + left[:11]
    base = _check(dev, left, right, (0.0, 0.8, 1.0))
    assert len(base) == 96 * 161 and sum(s >= 1.0 for s, _, _ in base) >= 11


def test_captured_call(dev):
    """The scan on a stream that is being captured: the graph replays to the eager call's hits."""
    import torch

    from napkon_string_matching_amd import _lib, grid
    from napkon_string_matching_amd import tables as tb

    rng = random.Random(6)
    word = lambda: _runs([rng.randint(0, 2) for _ in range(32)])
    left = [word() for _ in range(70)]
    right = left[:20] + [word() for _ in range(109)]
    lt, rt = tb.encode_strings(left, right, dev)
    lib = _lib.load()
    want = grid.indel_raw_grid(lt, rt, 0.8).as_tuples()
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
