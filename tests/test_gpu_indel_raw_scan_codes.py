"""The mixed-weight codes of the matrix-pipe scan (csrc/indel_raw_coarse.hpp), its row mask and its two register sets.

The scan computes D' = 64 D on the matrix pipe, D the bound of test_gpu_indel_raw_mfma_scan.py (per bucket min(a, r)
where r < CAP and a where r >= CAP), and lets a pair through where D' >= 64 need.  The left operand's slots are
64 [a >= k] and, last, the count a itself; the right one's are [k <= r < CAP] and 64 [r >= CAP].  What can go wrong is
the weight of a slot (a hit at D == need sits exactly on the bound, whether D comes from the indicator slots, S = 0 below,
from the last slot alone, S = la, or from both; S = the sum of the left counts over the buckets with r >= CAP), an operand
byte read with the wrong sign or width (bytes of 64 in every bucket of both lane halves; last slots of 64 x 64), the
mask of the rows that exist, which is now made only for a class's last block where that is not full, and the two sets of
registers that the loaded words of a block alternate between.

As there the strings are SORTED RUNS over at most 32 symbols (one bucket each): LCS = sum of min, so a pair with
D == need whose left counts do not exceed the right ones where r >= CAP is a true hit, and a lost one shows.  The tests
compute D, S and need themselves and assert that the pairs they are about exist; the hits of the three kernels are
compared with the oracle's, bit for bit.
"""
import itertools
import random

import pytest

pytestmark = pytest.mark.gpu

SYMS = "".join(sorted("abcdefghijklmnopqrstuvwxyzABCDEF"))  # 32 symbols, ascending: bucket = position
CAPS = (3, 4)


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _runs(counts):
    """c0^a0 c1^a1 ... over SYMS (ascending)."""
    assert len(counts) <= 32
    return "".join(s * a for s, a in zip(SYMS, counts))


def _counts(x):
    return [x.count(s) for s in SYMS]


def _oracle(left, right, thr):
    from oracle import native

    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    return native.indel_raw(cp(left), cp(right), thr, cap=1 << 20)


def _check(dev, left, right, thresholds):
    """The three kernels against the oracle at every threshold; returns the oracle's hits at the lowest one and the tables."""
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd import tables as tb

    lt, rt = tb.encode_strings(left, right, dev)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None and lt.alphabet <= 32
    base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in ({}, {"two_stage": False}, {"prune": False}):
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return base, lt, rt


def _need(thr, s):
    """The smallest LCS with which strings of la + lb = s reach ``thr`` (csrc/indel_score.hpp, the same doubles), or None."""
    for lcs in range(s // 2 + 1):
        if (1.0 - float(s - 2 * lcs) / float(s)) * 100.0 / 100.0 >= thr:
            return lcs
    return None


def _d_s(a, r, cap):
    """The scan's D and S of a pair of count vectors."""
    d = sum(min(x, y) if y < cap else x for x, y in zip(a, r))
    return d, sum(x for x, y in zip(a, r) if y >= cap)


def _at_the_bound(left, right, thr, base):
    """{(cap, D - need, kind of S)} over the pairs one below and on the bound, and whether those on it are the oracle's hits.
    Kind of S: "zero", "la" (S == la), "d" (S == D < la) or "mixed"."""
    hits = {(i, j) for s, i, j in base if s >= thr}
    seen = set()
    for (i, x), (j, y) in itertools.product(enumerate(left), enumerate(right)):
        need = _need(thr, len(x) + len(y)) if x and y else None
        if need is None or min(len(x), len(y)) < need:
            continue
        a, r = _counts(x), _counts(y)
        lcs = sum(map(min, a, r))
        assert ((i, j) in hits) == (lcs >= need)  # (sorted runs)
        for cap in CAPS:
            d, s = _d_s(a, r, cap)
            if d - need in (0, -1):
                kind = "zero" if s == 0 else "la" if s == len(x) else "d" if s == d else "mixed"
                seen.add((cap, d - need, kind, (i, j) in hits))
    return seen


# --- 1. slack extremes -----------------------------------------------------------------------------------------------------


def _slack_case():
    """Three families of 64-unit (40-unit for S = 0) strings, each with right rows that step D across need at 1.0 and 0.8."""
    left, right = [], []
    # S = la: the right row has 8 runs of 8 (>= CAP).  Left rows with k units on symbols the right row lacks have
    # D = S = 64 - k: k = 0, 1 around need 64 (threshold 1.0), k = 12, 13 around need 52
    right.append(_runs([8] * 8))
    for k in (0, 1, 12, 13):
        counts, rest = [8] * 8, k
        for s in range(7, -1, -1):
            take = min(rest, counts[s])
            counts[s] -= take
            rest -= take
        left.append(_runs(counts + [0] * 8 + [1] * k))
    # mixed S: 6 runs of 8 and 8 runs of 2 on both sides (symbols 8..21); the right rows move k units from the short runs
    # to a long one: D = 64 - k with S = 48
    left.append(_runs([0] * 8 + [8] * 6 + [2] * 8))
    for k in (0, 1, 12, 13):
        short = [2] * 8
        for u in range(k):
            short[u % 8] -= 1
        right.append(_runs([0] * 8 + [8 + k] + [8] * 5 + short))
    # S = 0: all 32 symbols once or twice, 40 units; the right rows have k of the 8 doubled symbols elsewhere: D = 40 - k,
    # k = 0, 1 around need 40 and k = 8 at need 32; one below that with a symbol missing (and nine doubled)
    left.append(_runs([2] * 8 + [1] * 24))
    for k in (0, 1, 8):
        right.append(_runs([1] * k + [2] * 8 + [1] * (24 - k)))
    right.append(_runs([1] * 8 + [2] * 9 + [0] + [1] * 14))
    return left, right


def test_slack_extremes(dev):
    """Hits at D == need (D' exactly 64 need) with S = la = 64, with S = D, with S = 0 and with S in between, at
    thresholds 1.0 (need 64 and 40) and 0.8 (need 52 and 32), each with its neighbour at D == need - 1, which is no hit."""
    left, right = _slack_case()
    base, _, _ = _check(dev, left, right, (0.8, 1.0))
    seen = _at_the_bound(left, right, 1.0, base)
    for cap in CAPS:
        for kind in ("la", "mixed", "zero"):
            assert (cap, 0, kind, True) in seen, (cap, kind)
        for kind in ("d", "mixed", "zero"):
            assert (cap, -1, kind, False) in seen, (cap, kind)
    seen = _at_the_bound(left, right, 0.8, base)
    for cap in CAPS:
        for kind in ("d", "mixed", "zero"):
            assert (cap, 0, kind, True) in seen and (cap, -1, kind, False) in seen, (cap, kind)
    assert not any(hit for _, k, _, hit in seen if k == -1)


# --- 2. sign ------------------------------------------------------------------------------------------------------------------


def test_sign_of_the_operands(dev):
    """Counts of 1 and 2 in ALL 32 buckets on both sides: every byte of the first left slot is 64 and of the first right
    slot 1, in both lane halves.  One-symbol strings of 64 units, in a bucket of either lane half: the last slots are 64 and
    64 (D' = 4096 = 64 need, the largest product and the largest sum there is)."""
    rng = random.Random(12)

    def ones_and_twos(n_twos):
        counts = [1] * 32
        for s in rng.sample(range(32), n_twos):
            counts[s] = 2
        return _runs(counts)

    def moved(x):  # one doubled symbol elsewhere: D = need - 1 at threshold 1.0
        counts = _counts(x)
        counts[counts.index(2)] = 1
        counts[counts.index(1)] = 2
        return _runs(counts)

    left = [ones_and_twos(n) for n in (0, 8, 8, 16, 16, 24, 32) for _ in range(4)]
    right = [ones_and_twos(n) for n in (0, 8, 8, 16, 16, 24, 32) for _ in range(5)] + left[4:12] + list(map(moved, left[4:12]))
    for s in (0, 15, 16, 31):
        left += [SYMS[s] * 64, SYMS[s] * 63]
        right += [SYMS[s] * 64, SYMS[s] * 62]
    base, _, _ = _check(dev, left, right, (0.5, 0.8, 1.0))
    hits = {(i, j) for s, i, j in base if s >= 1.0}
    assert {(i, j) for i, x in enumerate(left) for j, y in enumerate(right) if x == y} == hits and len(hits) >= 12
    # every pair of the ones-and-twos rows has S = 0 and D = sum of min over 32 buckets that are all in use
    for x, y in itertools.product(left[:28], right[:35]):
        a, r = _counts(x), _counts(y)
        assert min(a) >= 1 and min(r) >= 1 and _d_s(a, r, 3) == (sum(map(min, a, r)), 0)
    seen = _at_the_bound(left, right, 0.8, base) | _at_the_bound(left, right, 1.0, base)
    assert {(3, 0, "zero", True), (3, -1, "zero", False), (3, 0, "la", True)} <= seen


# --- 3. the repeated row ------------------------------------------------------------------------------------------------------


def _perturbed(base, rng):
    counts = list(base)
    up = rng.randrange(len(counts))
    down = rng.choice([s for s in range(len(counts)) if s != up and counts[s] > 0])
    counts[up] += 1
    counts[down] -= 1
    return counts


_CLASS_GROUPS = {"long": ((43, 65), (42, 64), (41, 63)), "short": ((40, 33), (39, 32), (38, 31), (37, 1))}  # (length, rows)


@pytest.mark.parametrize("from_end", [1, 2])
@pytest.mark.parametrize("group", ["long", "short"])
def test_row_mask(dev, group, from_end):
    """Length classes of 65, 64, 63 rows and of 33, 32, 31 and 1 rows: last blocks of 1, 32, 31 rows, full blocks, which
    get no mask at all, and a class that is one short block.  In every class ONE row, the last (or the second to last: then
    the class of one row has none), is near all 33 right strings and every other row is far from them: the hits are that
    row against every right string, each pair once, so the repeated last row of a short block must not show."""
    rng = random.Random(33)
    right = [_runs(_perturbed([5] * 8, rng)) for _ in range(33)]
    left, hitting = [], []
    for length, rows in _CLASS_GROUPS[group]:
        near = [5] * 8
        for u in range(abs(length - 40)):
            near[u % 8] += 1 if length > 40 else -1
        for k in range(rows):
            if k == rows - from_end:
                hitting.append(len(left))
                left.append(_runs(_perturbed(near, rng)))
            else:  # far: symbols 8..15, no unit in common with a right string
                far = [length // 8 + (1 if u < length % 8 else 0) for u in range(8)]
                left.append(_runs([0] * 8 + _perturbed(far, rng)))
            assert len(left[-1]) == length
    assert len(hitting) == len(_CLASS_GROUPS[group]) - (1 if group == "short" and from_end == 2 else 0)
    base, lt, _ = _check(dev, left, right, (0.8,))
    assert lt.orig.cpu().tolist() == list(range(len(left)))  # (built in table order: longest class first)
    pairs = [(i, j) for _, i, j in base]
    assert len(pairs) == len(set(pairs)) and set(pairs) == set(itertools.product(hitting, range(33)))


# --- 4. the register sets -----------------------------------------------------------------------------------------------------


def _far_apart(n, rng):
    """n strings of 40 units, four runs of ten over four of the 32 symbols, any two with at most two symbols in common
    (LCS <= 20: a score of at most 0.5)."""
    chosen = []
    while len(chosen) < n:
        cand = frozenset(rng.sample(range(32), 4))
        if all(len(cand & c) <= 2 for c in chosen):
            chosen.append(cand)
    return [[10 if s in c else 0 for s in range(32)] for c in chosen]


@pytest.mark.parametrize("blocks", [2, 3, 4, 5])
def test_register_sets(dev, blocks):
    """One length class of 2, 3, 4 and 5 full blocks (the two register sets change places after every block, and the loop
    over them is left after an even or an odd number) against four tiles of right strings that are far from one another
    and from the left rows, but for ONE pair per block and tile, each at another row of its block and another column of
    its tile: a block scanned with another block's words, or a tile lost where the loop is left, changes the hits."""
    rng = random.Random(40 + blocks)
    rows = _far_apart(128 + 32 * blocks, rng)
    right, left = rows[:128], rows[128:]
    planned = set()
    for blk, t in itertools.product(range(blocks), range(4)):
        i = 32 * blk + (7 * blk + 9 * t + 3) % 32
        j = 32 * t + (11 * blk + 5 * t + 1) % 32
        left[i] = _perturbed(right[j], rng)  # LCS 39 of 40: a score of 0.975
        planned.add((i, j))
    assert len({i for i, _ in planned}) == len({j for _, j in planned}) == 4 * blocks
    left, right = list(map(_runs, left)), list(map(_runs, right))
    base, lt, rt = _check(dev, left, right, (0.8, 0.95))
    assert lt.orig.cpu().tolist() == list(range(len(left))) and rt.orig.cpu().tolist() == list(range(128))
    assert {(i, j) for _, i, j in base} == planned and len(base) == 4 * blocks


def test_drain_between_the_blocks(dev):
    """A 4-letter alphabet at threshold 0.5, 160 left rows of ONE length (five blocks) x 257 right rows: more than a third of
    the pairs are hits, the stack passes its drain level inside the class, and the words of the block after the drain have
    to be in the register set that the block reads."""
    rng = random.Random(54)
    word = lambda n: "".join(rng.choice("abcd") for _ in range(n))
    left = [word(40) for _ in range(160)]
    right = [word(rng.randint(24, 64)) for _ in range(257)]
    base, _, _ = _check(dev, left, right, (0.5, 0.8))
    assert len(base) > len(left) * len(right) // 3


# --- 5. threshold 0 and rows of no length -----------------------------------------------------------------------------------


def test_threshold_zero(dev):
    """need = 0 (64 x 0 - 1 < 0 <= D'): on a 40 x 40 grid with empty strings on both sides every pair is a hit."""
    rng = random.Random(5)
    word = lambda: _runs([rng.randint(0, 2) for _ in range(32)])
    left = [word() for _ in range(37)] + ["", "", SYMS[3] * 64]
    right = ["", SYMS[3] * 64] + [word() for _ in range(38)]
    base, _, _ = _check(dev, left, right, (0.0,))
    assert len(base) == 1600 and {(i, j) for _, i, j in base} == set(itertools.product(range(40), range(40)))
