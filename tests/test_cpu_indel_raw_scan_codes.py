"""The code slots of the matrix-pipe scan (csrc/indel_raw_coarse.hpp), restated in plain Python: the thermometer codes the
scan used first ("old": indicators on both sides and an excess slot) and the mixed-weight ones it uses now ("new").

Per bucket, with a the left count and r the right count, both codes compute the same bound: min(a, r) where r < CAP and a
where r >= CAP.  The new one computes it scaled, D' = 64 D exactly, and tests D' >= 64 need (as D' > 64 need - 1).
Nothing here needs a GPU: the slot values are checked for their range (i8 operands, none negative), the bucket identity
for every a, r in 0..64, the kernel's byte-parallel word arithmetic against the slot values, and the test's equivalence
on seeded histograms, for CAP 2..8.

A code scaled by 128 with slack (left -128 [a >= s + 1] and a, right -([r >= s + 1] - [r >= CAP]) and 127 [r >= CAP]:
D' = 128 D - S with S the sum of a over the buckets with r >= CAP, 0 <= S <= 64, tested as D' >= 128 need - 64) was
measured and not kept; its identities are checked here too, as the record of why it is exact.
"""
import functools
import random

import pytest

CAPS = range(2, 9)
NEVER = 255  # csrc/nsm_common.hpp: kNever, the need of a pair that cannot fit
NEEDS = list(range(65)) + [NEVER]


def old_left(a, cap):
    return [int(a >= s + 1) for s in range(cap - 1)] + [max(a - (cap - 1), 0)]


def old_right(r, cap):
    return [int(r >= s + 1) for s in range(cap)]


def new_left(a, cap):
    return [64 * int(a >= s + 1) for s in range(cap - 1)] + [a]


def new_right(r, cap):
    return [int(r >= s + 1) - int(r >= cap) for s in range(cap - 1)] + [64 * int(r >= cap)]


def slack_left(a, cap):
    return [-128 * int(a >= s + 1) for s in range(cap - 1)] + [a]


def slack_right(r, cap):
    return [-(int(r >= s + 1) - int(r >= cap)) for s in range(cap - 1)] + [127 * int(r >= cap)]


def dot(x, y):
    return sum(p * q for p, q in zip(x, y))


def bound(a, r, cap):
    """What a bucket gives to D."""
    return min(a, r) if r < cap else a


@pytest.mark.parametrize("cap", CAPS)
def test_slots_fit_i8(cap):
    for c in range(65):
        for slots in (old_left(c, cap), old_right(c, cap), slack_left(c, cap), slack_right(c, cap)):
            assert len(slots) == cap and all(-128 <= v <= 127 for v in slots), (cap, c, slots)
        for slots in (new_left(c, cap), new_right(c, cap)):
            assert len(slots) == cap and all(0 <= v <= 64 for v in slots), (cap, c, slots)


@pytest.mark.parametrize("cap", CAPS)
def test_bucket_identity(cap):
    """old = the bound, new = 64 old, the code with slack = 128 old - a [r >= CAP], for every pair of counts."""
    for a in range(65):
        for r in range(65):
            old = dot(old_left(a, cap), old_right(r, cap))
            assert old == bound(a, r, cap), (cap, a, r)
            assert dot(new_left(a, cap), new_right(r, cap)) == 64 * old, (cap, a, r)
            assert dot(slack_left(a, cap), slack_right(r, cap)) == 128 * old - a * int(r >= cap), (cap, a, r)


def _bytes_i8(word):
    return [((word >> (8 * k)) & 0xFF) - 256 * ((word >> (8 * k + 7)) & 1) for k in range(4)]


def _ge64(word, k):
    """64 [c >= k] per byte, the kernel's c3c_ge64."""
    total = word + (0x40 - k) * 0x01010101
    assert total < 1 << 32
    return total & 0x40404040


@pytest.mark.parametrize("cap", CAPS)
def test_word_arithmetic(cap):
    """Four counts to a 32-bit word, as the kernel holds them: the left indicator slots are (w + (0x40 - k) 0x01010101) &
    0x40404040 and the last slot is w; the right slots are ((ge64(k) ^ ge64(CAP)) >> 6 and ge64(CAP).  No carry leaves a
    byte, and read as i8 the bytes are the slot values."""
    rng = random.Random(cap)
    quads = [[rng.randint(0, 64) for _ in range(4)] for _ in range(500)] + [[0, 1, 63, 64], [64] * 4, [0] * 4]
    quads += [[cap - 1, cap, cap + 1, cap - 2 if cap > 2 else 0]]
    for q in quads:
        w = sum(c << (8 * k) for k, c in enumerate(q))
        full = _ge64(w, cap)
        for s in range(cap - 1):
            assert _bytes_i8(_ge64(w, s + 1)) == [new_left(c, cap)[s] for c in q]
            assert _bytes_i8((_ge64(w, s + 1) ^ full) >> 6) == [new_right(c, cap)[s] for c in q]
        assert _bytes_i8(w) == [new_left(c, cap)[cap - 1] for c in q]
        assert _bytes_i8(full) == [new_right(c, cap)[cap - 1] for c in q]


def _histogram(rng, total, lo, hi):
    """32 bucket counts in lo..hi where they are not zero, summing to at most ``total``."""
    h = [0] * 32
    left = total
    for b in rng.sample(range(32), 32):
        if left < max(lo, 1):
            break
        c = rng.randint(lo, min(hi, left))
        if rng.random() < 0.7:
            h[b] = c
            left -= c
    return h


@functools.lru_cache(maxsize=None)
def _pairs():
    rng = random.Random(20)
    pairs = []
    for _ in range(3000):
        la = rng.randint(0, 64)
        pairs.append((_histogram(rng, la, 1, rng.choice((2, 4, 9, 64))), _histogram(rng, rng.randint(0, 64), 1, rng.choice((2, 4, 9, 64)))))
    # S = 0: no right count reaches the smallest CAP
    for _ in range(200):
        pairs.append((_histogram(rng, 64, 1, 8), [rng.randint(0, 1) for _ in range(32)]))
    # S = la = 64: every bucket the left row uses has a right count of 8 (>= every CAP)
    for _ in range(200):
        a = [0] * 32
        for b in rng.sample(range(32), rng.randint(1, 8)):
            a[b] = 1
        while sum(a) < 64:
            a[rng.choice([b for b in range(32) if a[b]])] += 1
        pairs.append((a, [8 if c else 0 for c in a]))
    one = [64] + [0] * 31
    pairs.append((one, one))
    return pairs


@pytest.mark.parametrize("cap", CAPS)
def test_scaled_test_is_the_test(cap):
    """D' = 64 D, and D' > 64 need - 1 exactly where D >= need: every need in 0..64, and kNever.  The code with slack:
    D' = 128 D - S with 0 <= S <= la, and D' >= 128 need - 64 exactly where D >= need, S = 0 and S = la = 64 included."""
    slack = set()
    # (the slot products of every pair of counts, once)
    old_of = [[dot(old_left(x, cap), old_right(y, cap)) for y in range(65)] for x in range(65)]
    new_of = [[dot(new_left(x, cap), new_right(y, cap)) for y in range(65)] for x in range(65)]
    slack_of = [[dot(slack_left(x, cap), slack_right(y, cap)) for y in range(65)] for x in range(65)]
    for a, r in _pairs():
        assert sum(a) <= 64 and sum(r) <= 64
        d_old = sum(old_of[x][y] for x, y in zip(a, r))
        d_new = sum(new_of[x][y] for x, y in zip(a, r))
        d_slack = sum(slack_of[x][y] for x, y in zip(a, r))
        s = sum(x for x, y in zip(a, r) if y >= cap)
        assert d_old == sum(bound(x, y, cap) for x, y in zip(a, r)) <= sum(a)
        assert d_new == 64 * d_old <= 4096 < 64 * NEVER - 1
        assert d_slack == 128 * d_old - s and 0 <= s <= sum(a) and 0 <= d_slack <= 8192
        slack.add(s if s in (0, 64) else -1)
        # the kernel's form: D' > nm1 with nm1 = 64 need - 1
        assert all((d_new > 64 * need - 1) == (d_old >= need) for need in NEEDS), (cap, a, r)
        assert all((d_slack > 128 * need - 65) == (d_old >= need) for need in NEEDS), (cap, a, r)
    assert slack == {0, 64, -1}
