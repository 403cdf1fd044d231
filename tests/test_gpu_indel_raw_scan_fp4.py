"""The FP4 scan of the two-stage RAW kernel (csrc/indel_raw_coarse.hpp, NSM_C3C_FP4): four code slots per bucket in two
v_mfma_f32_32x32x64_f8f6f4, the second with the right string's block scale.

Per bucket D_b = [a>=1][r>=1] + [a>=2][r>=2] + 2^k [a>=3][r>=3] + 2^k [a>=4] E(r), E the excess r - 3 rounded up to the
grid {0, 1, 2, 3, 4, 6, 8, 12} 2^k (tests/support/scan_fp4.py restates the codes; the tests compute D with it).  What can go
wrong: a slot's nibble on one side not facing its partner on the other, the rounding of E, the [a >= 4] switch, the scale
byte of another tile, a lane half with the other half's buckets, and everything around the scan that the operands' new
shapes touch (the B fragments made again behind a drain, the fold on f32 bits, threshold 0).

The strings are SORTED RUNS over at most 32 symbols (one bucket each), so LCS = sum of min and a pair whose D sits on its
need is a true hit exactly where sum of min does too.  The two-stage kernel, the one-stage kernel (NSM_FLAG_ONE_STAGE) and
the exhaustive kernel are compared with the oracle, bit for bit.
"""
import itertools
import random

import pytest

from tests.support import scan_fp4 as fp4

pytestmark = pytest.mark.gpu

SYMS = "".join(sorted("abcdefghijklmnopqrstuvwxyzABCDEF"))  # 32 symbols, ascending: bucket = position


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
    """The three kernels against the oracle at every threshold; returns the oracle's hits at the lowest one."""
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd import tables as tb

    lt, rt = tb.encode_strings(left, right, dev)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None and lt.alphabet <= 32
    if in_order:  # (built in table order: longest first, equal lengths as given)
        assert lt.orig.cpu().tolist() == list(range(len(left))) and rt.orig.cpu().tolist() == list(range(len(right)))
    base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in ({}, {"two_stage": False}, {"prune": False}):
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return base


def _need(thr, s):
    """The smallest LCS with which strings of la + lb = s reach ``thr`` (csrc/indel_score.hpp, the same doubles), or None."""
    for lcs in range(s // 2 + 1):
        if (1.0 - float(s - 2 * lcs) / float(s)) * 100.0 / 100.0 >= thr:
            return lcs
    return None


def _d(a, r):
    """The scan's D of two count vectors."""
    k = fp4.scale_of(r)
    return sum(fp4.bucket(x, y, k) for x, y in zip(a, r))


def _sum_min(a, r):
    return sum(map(min, a, r))


# --- 1. every slot, every excess value, every bucket, row position and tile ---------------------------------------------------

# kind -> (count of the special bucket, number of buckets with one unit behind it)
_KINDS = {"slot1": (1, 19), "slot2": (2, 18), "slot3": (3, 17)}
_KINDS.update({f"excess{e}": (3 + e, 10) for e in (1, 2, 3, 4, 5, 6, 7, 12, 13)})
_KINDS["excess61"] = (64, 0)
_ROUNDED = ("excess5", "excess7", "excess13", "excess61")  # E of the row itself is above its excess
_LESS_ROUNDED = ("excess6", "excess12", "excess61")  # ... and E of the row with one unit less


def _kind_counts(kind, b):
    if kind == "all":  # counts of 1, 2, 3, 5, 9 and 15 side by side: every slot gives to D
        counts = [0] * 32
        for u, c in enumerate((1, 2, 3, 5, 9, 15)):
            counts[(b + u) % 32] = c
        return counts
    special, ones = _KINDS[kind]
    counts = [0] * 32
    counts[b] = special
    for u in range(1, ones + 1):
        counts[(b + u) % 32] = 1
    return counts


def _one_less(counts, b):
    """One unit of bucket b in the bucket before it, which the row does not use."""
    out = list(counts)
    assert out[(b + 31) % 32] == 0 and out[b] >= 1
    out[b] -= 1
    out[(b + 31) % 32] = 1
    return out


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_slots_at_the_bound(dev, shift):
    """For every kind of row (D's last unit from slot 1, 2, 3, from an excess of 1 .. 7, 12, 13 = scale 2, 61 = scale 8, and
    all slots together) and every bucket b: a left row, its copy on the right (sum of min = need at threshold 1.0) and the copy
    with one unit of bucket b elsewhere (sum of min = need - 1; D = need - 1 where E is exact, D >= need where E rounds up:
    the bound lets a pair through that the drain has to drop).  A kind's 32 left rows are one block, row position = bucket;
    ``shift`` x 32 more right strings in front move every kind through the four tiles of a wave."""
    kinds = list(_KINDS) + ["all"]
    left, right, about = [], [], []
    right += [_runs(_kind_counts("excess61", s % 32)) for s in range(32 * shift)]  # (64 units: first in the table)
    for kind, b in itertools.product(kinds, range(32)):
        counts = _kind_counts(kind, b)
        about.append((kind, b, counts, len(left), len(right)))
        left.append(_runs(counts))
        right += [_runs(counts), _runs(_one_less(counts, b))]
    base = _check(dev, left, right, (0.8, 1.0))
    hits = {(i, j) for s, i, j in base if s >= 1.0}
    rounded_up = 0
    for kind, b, counts, i, j in about:
        less = _one_less(counts, b)
        need = _need(1.0, 2 * sum(counts))
        assert need == sum(counts) == _sum_min(counts, counts) and _sum_min(counts, less) == need - 1
        assert (i, j) in hits and (i, j + 1) not in hits
        assert _d(counts, counts) >= need
        assert (_d(counts, counts) > need) == (kind in _ROUNDED), kind
        if kind in _LESS_ROUNDED:  # (an excess of 5 counts as 6, of 11 as 12: the scan lets the pair through, the drain drops it)
            assert _d(counts, less) >= need, kind
            rounded_up += 1
        else:
            assert _d(counts, less) == need - 1, kind
    assert rounded_up == 96
    assert fp4.scale_of(_kind_counts("excess13", 0)) == 1 and fp4.scale_of(_kind_counts("excess61", 0)) == 3


# --- 2. the a >= 4 switch -----------------------------------------------------------------------------------------------------


def _switch_case():
    pad = [1] * 12
    left, right, info_l, info_r = [], [], [], []
    for b in (5, 21):  # a bucket of either lane half
        for a, f in itertools.product((3, 4, 5), range(8)):  # f units on symbols that no right string has
            counts = [0] * 32
            counts[b] = a
            for u in range(12):
                counts[(b + 1 + u) % 32] = pad[u]
            for u in range(f):
                counts[(b + 13 + u) % 32] = 1
            left.append(_runs(counts))
            info_l.append((b, a, counts))
        for r, g in itertools.product((2, 3, 4, 9), range(5)):  # g units on symbols that no left string has
            counts = [0] * 32
            counts[b] = r
            for u in range(12):
                counts[(b + 1 + u) % 32] = pad[u]
            for u in range(g):
                counts[(b + 20 + u) % 32] = 1
            right.append(_runs(counts))
            info_r.append((b, r, counts))
    # (one long string a side: the tables have a stride of 64)
    left.append(SYMS[0] * 64)
    right.append(SYMS[16] * 64)
    return left, right, info_l, info_r


_SWITCH_THRESHOLDS = (0.8, 0.85, 0.9, 0.95, 1.0)


def test_left_counts_across_the_switch(dev):
    """Left counts of 3, 4 and 5 in one bucket against right counts of 2, 3, 4 and 9, with pairs on their need and one below it
    for every combination: below the switch the bucket gives min(a, r), from a = 4 on it gives r (9 included, a = 4 and 5)."""
    left, right, info_l, info_r = _switch_case()
    _check(dev, left, right, _SWITCH_THRESHOLDS)
    seen = set()
    for (b, a, x), (b_right, r, y) in itertools.product(info_l, info_r):
        if b != b_right:
            continue
        d = _d(x, y)
        assert d == _sum_min(x, y) + (max(r - a, 0) if a >= 4 else 0)
        for thr in _SWITCH_THRESHOLDS:
            need = _need(thr, sum(x) + sum(y))
            if need is not None and min(sum(x), sum(y)) >= need and d - need in (0, -1):
                seen.add((a, r, d - need))
    assert seen >= set(itertools.product((3, 4, 5), (2, 3, 4, 9), (0, -1))), sorted(seen)


# --- 3. right strings with a scale ------------------------------------------------------------------------------------------


def _moved(counts, rng):
    out = list(counts)
    down = rng.choice([s for s in range(32) if out[s] > 0])
    up = rng.choice([s for s in range(32) if s != down])
    out[down] -= 1
    out[up] += 1
    return out


def test_scaled_right_strings(dev):
    """128 right strings of 60 units: tile 0 has strings with k = 1, 2 and 3 among ordinary ones, tile 1 only such strings,
    tiles 2 and 3 none, so a scale byte taken from another tile shows.  The left rows are the right strings and neighbours of
    them with one unit elsewhere, in three length classes."""
    rng = random.Random(77)

    def ordinary():
        counts = [0] * 32
        for s in rng.sample(range(32), 12):
            counts[s] = 5
        return counts

    def scaled(k):
        top = {1: rng.randint(16, 27), 2: rng.randint(28, 51), 3: rng.randint(52, 56)}[k]
        counts = [0] * 32
        spots = rng.sample(range(32), 1 + (60 - top + 3) // 4)
        counts[spots[0]] = top
        rest = 60 - top
        for s in spots[1:]:
            counts[s] = min(4, rest)
            rest -= counts[s]
        assert sum(counts) == 60 and fp4.scale_of(counts) == k
        return counts

    rows = [scaled(1 + u % 3) if u % 4 == 0 else ordinary() for u in range(32)]
    rows += [scaled(1 + u % 3) for u in range(32)]
    rows += [ordinary() for _ in range(64)]
    ks = [fp4.scale_of(c) for c in rows]
    assert {0, 1, 2, 3} == set(ks[:32]) and 0 not in ks[32:64] and set(ks[64:]) == {0}
    right = list(map(_runs, rows))
    left = []
    for c in rows[:80]:
        left.append(_runs(c))  # 60 units
    for c in rows[:80]:
        left.append(_runs(_moved(c, rng)))  # 60 units, LCS 59
    for c in rows[16:48]:
        less = list(c)
        less[less.index(max(less))] -= 1
        left.append(_runs(less))  # 59 units, LCS 59
    base = _check(dev, left, right, (0.8, 0.95, 1.0))
    exact = {(i, j) for s, i, j in base if s >= 1.0}
    assert {(u, u) for u in range(80)} <= exact
    # with the scale of an ordinary string (k = 0) the bound of these pairs would fall below their need
    lost = sum(sum(sum(fp4.bucket_parts(x, x, ks[u])) for x in rows[u]) < 60 for u in range(64) if ks[u])
    assert lost >= 32


# --- 4. class and table sizes ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_right", [1, 33, 129])
def test_class_and_table_sizes(dev, n_right):
    """Length classes of 65 (across the end of the first chunk of 64 rows), 33, 32, 31 and 1 rows whose LAST row is near every
    right string while every other row is far from them all: each of those pairs once, against right tables of 1, 33 and 129
    strings (a tile of one string, a second tile of one, a second wave of one)."""
    rng = random.Random(100 + n_right)
    right = [_runs(_moved([5] * 8 + [0] * 24, rng)) for _ in range(n_right)]
    left, hitting = [], []
    for length, n_rows in ((44, 65), (43, 33), (42, 32), (41, 31), (39, 1)):
        near = [5] * 8
        for u in range(abs(length - 40)):
            near[u % 8] += 1 if length > 40 else -1
        for k in range(n_rows):
            if k == n_rows - 1:
                hitting.append(len(left))
                left.append(_runs(_moved(near + [0] * 24, rng)))
            else:  # far: symbols 8 .. 15
                far = [length // 8 + (1 if u < length % 8 else 0) for u in range(8)]
                left.append(_runs(_far_row(far, rng)))
            assert len(left[-1]) == length
    base = _check(dev, left, right, (0.8,), in_order=True)
    pairs = [(i, j) for _, i, j in base]
    assert len(pairs) == len(set(pairs)) and set(pairs) == set(itertools.product(hitting, range(n_right)))


def _far_row(far, rng):
    """Eight runs on symbols 8 .. 15, one unit moved between two of them."""
    counts = list(far)
    up = rng.randrange(8)
    down = rng.choice([s for s in range(8) if s != up and counts[s] > 0])
    counts[up] += 1
    counts[down] -= 1
    return [0] * 8 + counts + [0] * 16


# --- 5. four letters ----------------------------------------------------------------------------------------------------------


def test_four_letters(dev):
    """A 4-letter alphabet, 96 left rows of one length (three blocks) x 161 right rows: every count is large, many right
    strings have a scale, most pairs pass the scan, a drain runs between the blocks and the B fragments and their scales are
    made again behind it."""
    rng = random.Random(96)
    word = lambda n: "".join(rng.choice("abcd") for _ in range(n))
    left = [word(40) for _ in range(96)]
    right = [word(rng.randint(24, 64)) for _ in range(161)]
    assert sum(max(y.count(c) for c in "abcd") >= 16 for y in right) >= 40
    base = _check(dev, left, right, (0.5, 0.8))
    assert len(base) > len(left) * len(right) // 3


# --- 6. thresholds ------------------------------------------------------------------------------------------------------------


def test_thresholds_zero_to_one(dev):
    """Threshold 0 (need 0: the bits of -1/2 are below those of every D, and empty rows on both sides hit everything), 0.8
    and 1.0 on a 40 x 40 grid."""
    rng = random.Random(5)
    word = lambda: _runs([rng.randint(0, 2) for _ in range(32)])
    left = [word() for _ in range(36)] + ["", "", SYMS[3] * 64, SYMS[4] * 20]
    right = ["", SYMS[3] * 64] + left[:8] + [word() for _ in range(30)]
    base = _check(dev, left, right, (0.0, 0.8, 1.0))
    assert len(base) == 1600 and {(i, j) for _, i, j in base} == set(itertools.product(range(40), range(40)))
    assert sum(s >= 1.0 for s, _, _ in base) >= 9
