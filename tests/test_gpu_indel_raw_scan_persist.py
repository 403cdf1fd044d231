"""The persistent launch of the packed two-stage RAW scan (csrc/indel_raw_coarse.hpp: c3p_prepass_kernel lists work items,
(right tile, run of left rows, base row), and indel_raw_coarse_kernel<.., true, true> is a fixed number of waves that pull
them; NSM_FLAG_ONE_GROUP launches ONE workgroup, whose four waves then each take many items of several tiles and bases).

What can go wrong: an interval that ends a length class short, an item cut in the wrong place (a class that straddles two
items, a window of 2^15 rows), a stack entry whose row is counted from the item's first row instead of its base, a stack
or a right set-up that outlives a change of tile, a head that is not zeroed or a list that is not rebuilt between calls, a
pulled range that runs past the list.  The scan is a filter, so most of these show as LOST hits; the packed call with
and without ``one_group``, the unpacked call, the one-stage kernel and the oracle are compared bit for bit.

The strings are sorted runs over at most 32 symbols (one bucket each: LCS = sum of min), so a pair's score follows from
its count vectors and mates can be planted exactly on a threshold.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

SYMS = "".join(sorted("abcdefghijklmnopqrstuvwxyzABCDEF"))  # 32 symbols, ascending: bucket = position
VARIANTS = ({"pack": True}, {"pack": True, "one_group": True}, {"pack": False}, {"two_stage": False})


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


def _encode(dev, left, right):
    from napkon_string_matching_amd import tables as tb

    lt, rt = tb.encode_strings(left, right, dev)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None
    return lt, rt


def _check(dev, left, right, thresholds):
    """Every variant against the oracle at every threshold; returns the oracle's hits at the lowest one."""
    from napkon_string_matching_amd import grid

    lt, rt = _encode(dev, left, right)
    base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in VARIANTS:
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return base


def _right_counts(rng, n, units=5, runs=8):
    out = []
    for _ in range(n):
        counts = [0] * 32
        for s in rng.sample(range(32), runs):
            counts[s] = units
        out.append(counts)
    return out


def _resized(counts, length):
    """The same symbols, `length` units: units added to or taken from the used buckets in turn."""
    out = list(counts)
    used = [s for s in range(32) if out[s]]
    assert length >= len(used)
    have, u = sum(out), 0
    while have != length:
        step = 1 if length > have else -1
        if out[used[u % len(used)]] + step >= 1:
            out[used[u % len(used)]] += step
            have += step
        u += 1
    return out


# --- 1. class sizes against table sizes: items that end inside a class, more tiles than a workgroup has waves --------------


@pytest.mark.parametrize("n_right", [1, 33, 129, 641])
def test_class_and_table_sizes(dev, n_right):
    """Left length classes of 65, 33, 32, 31 and 1 rows and one of 200 rows, 362 rows in items of 64: every class but the
    first starts inside an item, and the class of 200 runs across three item ends.  641 right strings are six tiles, more
    than the one workgroup has waves.  Left row i is near right string i mod n_right and far from every other."""
    rng = random.Random(700 + n_right)
    rights = _right_counts(rng, n_right)
    left, mates = [], []
    for length, n_rows in ((44, 65), (43, 33), (42, 32), (41, 31), (40, 200), (39, 1)):
        for _ in range(n_rows):
            j = len(left) % n_right
            left.append(_runs(_resized(rights[j], length)))
            mates.append(j)
    assert len(left) == 362
    base = _check(dev, left, list(map(_runs, rights)), (0.8, 1.0))
    pairs = {(i, j) for _, i, j in base}
    assert len(pairs) == len(base) and pairs >= set(enumerate(mates))


# --- 2. tiles that fit nothing ----------------------------------------------------------------------------------------------


def test_a_tile_that_fits_nothing_between_two_that_do(dev):
    """Right tiles of 60, of 30 and of 10 units against left rows of 60 and of 10 units at 0.8: the middle tile's interval is
    empty, it gets no item and the tiles beside it keep theirs."""
    rng = random.Random(11)
    rights = ([_resized(c, 60) for c in _right_counts(rng, 128)] + [_resized(c, 30) for c in _right_counts(rng, 128)]
              + [_resized(c, 10) for c in _right_counts(rng, 128, units=1)])
    left = [_runs(rights[k]) for k in range(100)] + [_runs(rights[256 + k]) for k in range(100)]
    base = _check(dev, left, list(map(_runs, rights)), (0.8,))
    hit = {(i, j) for _, i, j in base}
    assert {(k, k) for k in range(100)} | {(100 + k, 256 + k) for k in range(100)} <= hit
    assert not any(128 <= j < 256 for _, j in hit)


def test_no_tile_fits_anything(dev):
    """Left rows of 64 units, right strings of 8: no item, no hit -- and the call after it on the same stream finds its own."""
    rng = random.Random(12)
    rights = [_resized(c, 8) for c in _right_counts(rng, 200, units=1)]
    left = [_runs(_resized(c, 64)) for c in _right_counts(rng, 70)]
    assert _check(dev, left, list(map(_runs, rights)), (0.8,)) == []
    assert len(_check(dev, left[:40], left[:10], (0.8,))) >= 10


# --- 3. the ends of an interval ---------------------------------------------------------------------------------------------


def test_strings_that_fit_only_the_ends_of_their_interval(dev):
    """A right string of 40 units at 0.8 fits left lengths 27 .. 60 and no other: 2 x 40 / 100 and 2 x 27 / 67 reach 0.8,
    2 x 40 / 101 and 2 x 26 / 66 do not.  Left rows of 61, 60, 27 and 26 units that hold, or are held by, their right string:
    the hits are all in the longest and in the shortest class of the interval, which an interval one class short loses."""
    rng = random.Random(13)
    rights = _right_counts(rng, 129)
    left = []
    for length in (61, 60, 27, 26):
        for j in range(129):
            left.append(_runs(_resized(rights[j], length)))
    base = _check(dev, left, list(map(_runs, rights)), (0.8,))
    hit = {(i, j) for _, i, j in base}
    for j in range(129):
        assert (129 + j, j) in hit and (2 * 129 + j, j) in hit
        assert (j, j) not in hit and (3 * 129 + j, j) not in hit


# --- 4. thresholds 0 and 1 ---------------------------------------------------------------------------------------------------


def test_thresholds_zero_and_one(dev):
    """Threshold 0: every pair is a hit, empty rows included, and every tile's interval is every row.  1.0: equal strings."""
    rng = random.Random(14)

    def word(n):
        counts = [0] * 32
        for _ in range(n):
            counts[rng.randrange(32)] += 1
        return _runs(counts)

    left = [word(rng.choice((0, 1, 9, 40, 64))) for _ in range(90)]
    right = left[:30] + [word(rng.choice((0, 2, 40, 63))) for _ in range(110)]
    base = _check(dev, left, right, (0.0, 1.0))
    assert len(base) == 90 * 140


# --- 5. a stack that is full at a tile change ---------------------------------------------------------------------------------


def test_four_letters(dev):
    """A 4-letter alphabet, 96 left rows of one length x 161 right rows (two tiles) at threshold 0: every pair passes, the stack
    drains in the middle of an item and is full where the wave goes on to the other tile; 0.8 and 1.0 ride along."""
    rng = random.Random(961)
    word = lambda n: "".join(rng.choice("abcd") for _ in range(n))
    left = [word(40) for _ in range(96)]
    right = [word(rng.randint(24, 64)) for _ in range(150)] + left[:11]
    base = _check(dev, left, right, (0.0, 0.8, 1.0))
    assert len(base) == 96 * 161 and sum(s >= 1.0 for s, _, _ in base) >= 11


# --- 6. a window boundary ---------------------------------------------------------------------------------------------------


def test_window_boundary(dev):
    """2^15 + 200 left rows of one length against 129 right strings: a tile's rows are two windows, and the entries of the
    second count their rows from ITS first row.  Mates in rows 32 766 .. 32 770 and in the last row.  The whole grid against
    the one-stage kernel, rows 32 700 .. 32 840 against the oracle."""
    from napkon_string_matching_amd import grid

    rng = random.Random(15)
    rights = _right_counts(rng, 129)
    n = (1 << 15) + 200
    far = SYMS[8] * 20 + SYMS[24] * 20
    left = [far] * n
    planted = list(range(32766, 32771)) + [n - 1]
    for k, i in enumerate(planted):
        left[i] = _runs(rights[20 * k + 3])
    right = list(map(_runs, rights))
    lt, rt = _encode(dev, left, right)
    want = grid.indel_raw_grid(lt, rt, 0.8, two_stage=False).as_tuples()
    assert {(i, 20 * k + 3) for k, i in enumerate(planted)} <= {(i, j) for _, i, j in want}
    for kw in VARIANTS[:3]:
        assert grid.indel_raw_grid(lt, rt, 0.8, **kw).as_tuples() == want, kw
    lo, hi = 32700, 32840
    sub = _oracle(left[lo:hi], right, 0.8)
    assert [(s, i - lo, j) for s, i, j in want if lo <= i < hi] == sub and len(sub) >= 5


# --- 7. the list and the head are made again by every call ---------------------------------------------------------------------


def _tables_for_calls(dev):
    rng = random.Random(16)
    out = []
    for n_left, n_right in ((150, 300), (40, 10), (333, 129), (70, 641)):
        rights = _right_counts(rng, n_right)
        left = [_runs(_resized(rights[i % n_right], rng.choice((38, 40, 43)))) for i in range(n_left)]
        out.append(_encode(dev, left, list(map(_runs, rights))))
    return out


def _launch(lib, lt, rt, buf, stream, one_group):
    from napkon_string_matching_amd import _lib

    flags = _lib.FLAG_PRUNE | _lib.FLAG_PACK | (_lib.FLAG_ONE_GROUP if one_group else 0)
    _lib.check(lib.nsm_indel_raw_grid(lt.struct(), rt.struct(), 0.8, flags, buf.records.data_ptr(), buf.capacity,
                                      buf.count.data_ptr(), stream.cuda_stream), "nsm_indel_raw_grid")


@pytest.mark.parametrize("one_group", [False, True])
def test_calls_back_to_back_and_on_two_streams(dev, one_group):
    """Four calls with different tables back to back on one stream, then two calls on two streams with no synchronisation
    between them: every call lists its own items and pulls from a head of its own."""
    import torch

    from napkon_string_matching_amd import _lib, grid

    lib = _lib.load()
    tables = _tables_for_calls(dev)
    want = [grid.indel_raw_grid(lt, rt, 0.8, pack=False).as_tuples() for lt, rt in tables]
    assert all(len(w) >= 40 for w in want)
    hits_of = lambda buf: grid.sort_hits_device(buf, int(buf.count.item())).as_tuples()
    bufs = [grid.HitBuffer(1 << 16, dev) for _ in tables]
    for b in bufs:
        b.reset()
    torch.cuda.synchronize(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for (lt, rt), b in zip(tables, bufs):
        _launch(lib, lt, rt, b, s1, one_group)
    s1.synchronize()
    assert [hits_of(b) for b in bufs] == want
    for b in bufs:
        b.reset()
    torch.cuda.synchronize(dev)
    _launch(lib, *tables[0], bufs[0], s1, one_group)
    _launch(lib, *tables[2], bufs[2], s2, one_group)
    _launch(lib, *tables[3], bufs[3], s1, one_group)
    _launch(lib, *tables[1], bufs[1], s2, one_group)
    s1.synchronize()
    s2.synchronize()
    assert [hits_of(b) for b in bufs] == want
