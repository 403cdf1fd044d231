"""The software pipeline of the matrix-pipe scan (csrc/indel_raw_coarse.hpp): two accumulators, the MFMA chain of a tile
issued before the fold and the push of the tile before it -- across the tiles of a block, the blocks of a length class,
and emptied at a class's end and in front of a drain.

What that order can get wrong is WHICH tile an accumulator is read for: the wrong need (tiles of one wave hold right
strings of different lengths), the wrong block (first row, length, mask of the rows that exist) or a tile lost or
folded twice where the pipeline is filled or emptied.  As in test_gpu_indel_raw_mfma_scan.py the strings are SORTED
RUNS (LCS = sum of min over the symbols, so the scan's bound is tight where right counts stay below CAP or reach the
left ones), the test computes D and need itself and asserts where pairs with D == need and with D == need - 1 sit, and
every case is compared with the oracle, the one-stage kernel and the exhaustive kernel at thresholds 0.5 and 0.8, hits
bit for bit.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

CORE = "abcdefgh"  # the symbols of the run strings; "y" and "z" are fillers, "ijklmnop" belong to rows far from any other
FAR = "ijklmnop"
THRESHOLDS = (0.5, 0.8)


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


def _need(thr, s):
    """The smallest LCS with which strings of la + lb = s reach ``thr`` (csrc/indel_score.hpp, the same doubles), or None."""
    for lcs in range(s // 2 + 1):
        if (1.0 - float(s - 2 * lcs) / float(s)) * 100.0 / 100.0 >= thr:
            return lcs
    return None


def _dot(x, y, cap):
    """The scan's D of a pair (at most 32 distinct symbols: one bucket each)."""
    return sum(min(x.count(ch), y.count(ch)) if y.count(ch) < cap else x.count(ch) for ch in set(x))


def _fits(x, y, thr):
    """The exact length filter in front of the scan: can a pair of these lengths reach ``thr`` at all?"""
    need = _need(thr, len(x) + len(y)) if x and y else None
    return need is not None and min(len(x), len(y)) >= need


def _table_order(rows):
    """The tables' row order: by length, longest first, input order inside a length (tables.StrTable.from_codes)."""
    return sorted(range(len(rows)), key=lambda i: -len(rows[i]))


def _boundary_cover(left, right, l_order, r_order, key):
    """Where the pairs with D == need (kind 0) and with D == need - 1 (kind 1) sit, among those the length filter lets
    through, at either threshold and for CAP 3 and 4: {(cap, kind)} -> set of key(left position, right position), the
    positions being those of the tables' rows (``l_order`` / ``r_order``: indices into ``left`` / ``right``)."""
    cover = {(cap, k): set() for cap in (3, 4) for k in (0, 1)}
    for pi, i in enumerate(l_order):
        for pj, j in enumerate(r_order):
            x, y = left[i], right[j]
            for thr in THRESHOLDS:
                if not _fits(x, y, thr):
                    continue
                need = _need(thr, len(x) + len(y))
                for cap in (3, 4):
                    k = need - _dot(x, y, cap)
                    if k in (0, 1):
                        cover[cap, k].add(key(pi, pj))
    return cover


def _perturbed(base, rng):
    """``base`` with one count a unit up and another (not yet zero) a unit down: the length stays."""
    counts = list(base)
    up = rng.randrange(len(counts))
    down = rng.choice([s for s in range(len(counts)) if s != up and counts[s] > 0])
    counts[up] += 1
    counts[down] -= 1
    return counts


# --- accumulator / tile mix-up -------------------------------------------------------------------------------------------

# right strings of tile t: length, and the units missing from a row with every core count at 4 (left rows: 32 units, every
# core symbol 4 times but one 5 and one 3 times).  At threshold 0.8 need = ceil(0.4 (32 + lb)) = 30, 29, 28, 26: against a
# left count of 4 a right count of r < CAP gives 4 - r less than the 32 of a full row, so D = need where the left row's
# symbols with a short right run are at 4, need - 1 where one of them is at 5 and need + 1 where one is at 3.
_TILES = ((42, (2,)), (39, (1,)), (36, (0,)), (33, (0, 2)))


@pytest.fixture(scope="module")
def mixup_case():
    rng = random.Random(412)
    left = [_runs(_perturbed([4] * 8, rng)) for _ in range(96)]
    right = []
    for lb, short in _TILES:
        for _ in range(32):
            counts = [4 + rng.randrange(3) for _ in range(8)]  # (4..6 >= CAP: the bucket gives the left count)
            for s, r in zip(rng.sample(range(8), len(short)), short):
                counts[s] = r
            while sum(counts) > lb:  # (only the long runs shrink, and not below 4)
                s = rng.choice([s for s in range(8) if counts[s] > 4])
                counts[s] -= 1
            right.append(_runs(counts, tail="z" * (lb - sum(counts))))
    right.append(_runs([4, 4, 4, 4, 4, 4, 2, 0], tail="zzzz"))  # 30 units: the 129th row, alone in the second wave
    rng.shuffle(right)
    return left, right


def test_every_block_and_tile(dev, mixup_case):
    """96 left rows of one length (three full blocks: the pipeline runs from one block into the next twice, and is filled
    and emptied once) against 128 + 1 right rows whose four tiles have four lengths, so that need differs from tile to
    tile (30, 29, 28 and 26 at threshold 0.8).  For every one of the 3 x 4 (block, tile) combinations -- both parities of
    the block index, both accumulators -- and for both caps there are pairs with D == need and pairs with D == need - 1:
    an accumulator compared with another tile's need, or pushed with another tile's or block's tag, changes the hits."""
    left, right = mixup_case
    assert len(set(map(len, left))) == 1 and len(left) == 96 and len(right) == 129
    (base, lt), rt = _check(dev, left, right, THRESHOLDS, tables=True)
    l_order, r_order = lt.orig.cpu().tolist(), rt.orig.cpu().tolist()
    assert l_order == _table_order(left) and r_order == _table_order(right)
    assert [len(right[j]) for j in r_order[::32]] == [42, 39, 36, 33, 30]
    needs = [_need(0.8, 32 + len(right[j])) for j in r_order[:128:32]]
    assert needs == [30, 29, 28, 26]
    first_wave = lambda pi, pj: (pi >> 5, pj >> 5) if pj < 128 else None
    cover = _boundary_cover(left, right, l_order, r_order, first_wave)
    for (cap, k), cells in cover.items():
        missing = {(blk, t) for blk in range(3) for t in range(4)} - cells
        assert not missing, f"cap {cap}, D == need - {k}: no such pair in (block, tile) {sorted(missing)}"
    # (at threshold 0.5 every pair is a hit: every tile of every block pushes all its entries)
    assert 0 < sum(1 for h in base if h[0] >= 0.8) < len(base) == len(left) * len(right)


# --- class boundaries and ragged ends --------------------------------------------------------------------------------------

# left length classes in table order: (base counts of the core symbols, rows, rows FAR from every right row in front).
# 36 units: 64 rows, the first block far from everything, so that of this class only the LAST block holds boundary pairs;
# 32 units: 33 rows (a last block of one row); 20 units: 3 rows that NO right string fits at threshold 0.8 (the right
# strings have 40..44 units, which take 27..66 left ones, or 10, which take 7..15); 12 units: 32 rows (one block, first
# and last of its class); 11 units: 1 row.
_CLASSES = (
    ([5, 5, 5, 5, 4, 4, 4, 4], 64, 32),
    ([4, 4, 4, 4, 4, 4, 4, 4], 33, 0),
    ([3, 3, 3, 3, 2, 2, 2, 2], 3, 0),
    ([2, 2, 2, 2, 1, 1, 1, 1], 32, 0),
    ([2, 2, 2, 1, 1, 1, 1, 1], 1, 0),
)


@pytest.fixture(scope="module")
def classes_case():
    rng = random.Random(77)
    left = []
    for base, rows, far in _CLASSES:
        for k in range(rows):
            left.append(_runs(_perturbed(base, rng), syms=FAR if k < far else CORE))
    right = []
    for k in range(97):  # long rows: every run at 5 or 6 (>= CAP) but one or two short ones, 40..44 units
        counts = [5 + rng.randrange(2) for _ in range(8)]
        for s in rng.sample(range(8), 1 + k % 2):
            counts[s] = rng.randrange(3)
        lb = 40 + k % 5
        while sum(counts) > lb:
            s = rng.choice([s for s in range(8) if counts[s] > 4])
            counts[s] -= 1
        right.append(_runs(counts, tail="z" * (lb - sum(counts))))
    for k in range(32):  # short rows: 10 units, runs of 0..2 (< CAP: the bucket gives the minimum)
        counts = [0] * 8
        while sum(counts) < 8 + k % 3:
            s = rng.randrange(8)
            counts[s] = min(2, counts[s] + 1)
        right.append(_runs(counts, tail="z" * (10 - sum(counts))))
    rng.shuffle(right)
    assert len(right) == 129
    return left, right, _oracle(left, right, min(THRESHOLDS))


def _class_blocks():
    """(class, block of the class) of every left table row of ``classes_case``."""
    return [(c, k >> 5) for c, (_, rows, _) in enumerate(_CLASSES) for k in range(rows)]


def test_class_boundaries(dev, classes_case):
    """Left length classes of 64, 33, 3, 32 and 1 rows, each of its own length: the pipeline is emptied behind every class
    and filled again, a last block of ONE row (33 = 32 + 1, and the class of one row) puts the mask of the rows that exist
    on a tile that was issued while the block before was folded, and the class of 20 units, which no right string fits
    at threshold 0.8, is skipped between two classes that are scanned.  The pairs with D == need and D == need - 1 sit in
    the last block of a class and the first block of the next and nowhere else (the first block of the first class is far
    from every right row), in every such block."""
    left, right, base = classes_case
    (_, lt), rt = _check(dev, left, right, THRESHOLDS, base=base, tables=True)
    l_order, r_order = lt.orig.cpu().tolist(), rt.orig.cpu().tolist()
    assert l_order == list(range(len(left))) and r_order == _table_order(right)  # (left: built in table order)
    where = _class_blocks()
    fit = [any(_fits(left[i], y, 0.8) for y in right) for i in range(len(left))]
    assert [all(fit[i] for i in range(len(left)) if where[i][0] == c) for c in range(5)] == [True, True, False, True, True]
    assert not any(fit[i] for i in range(len(left)) if where[i][0] == 2)
    cover = _boundary_cover(left, right, l_order, r_order, lambda pi, pj: where[pi])
    at_a_boundary = {(0, 1), (1, 0), (1, 1), (3, 0), (4, 0)}
    for (cap, k), cells in cover.items():
        assert cells - {(2, 0)} == at_a_boundary, f"cap {cap}, D == need - {k}: (class, block) {sorted(cells)}"
    assert 0 < sum(1 for h in base if h[0] >= 0.8) < len(base) < len(left) * len(right)


@pytest.mark.parametrize("n_right", [1, 33, 129])
def test_ragged_ends(dev, classes_case, n_right):
    """The class-boundary left table against right tables of one string, of a tile and one string, and of a wave and one
    string: tiles without a right string run through the pipeline like the others and push nothing."""
    left, right, base = classes_case
    # (a right table of the first n_right rows keeps their indices: the oracle's hits are filtered, not recomputed)
    _check(dev, left, right[:n_right], THRESHOLDS, base=[h for h in base if h[2] < n_right])


# --- drain with a tile in flight ----------------------------------------------------------------------------------------


def test_drain_between_blocks_of_one_class(dev):
    """A 4-letter alphabet at threshold 0.5, 224 left rows of ONE length (seven blocks) x 300 right rows: more than a third
    of the pairs are hits, so a block pushes several hundred entries and the stack passes its drain level between full
    blocks of one class, where the scan has the next block's first tile to issue (test_stack_pressure of
    test_gpu_indel_raw_mfma_scan.py spreads its rows over 65 classes and never drains inside one)."""
    rng = random.Random(53)
    word = lambda n: "".join(rng.choice("abcd") for _ in range(n))
    left = [word(40) for _ in range(224)]
    right = [word(rng.randint(24, 64)) for _ in range(300)]
    base, _ = _check(dev, left, right, THRESHOLDS)
    assert len(base) > len(left) * len(right) // 3
