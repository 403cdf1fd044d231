"""The stop rule of the per-pair LCS (csrc/indel_raw.hip: raw_lcs_pair), restated in plain Python and checked against a
plain DP LCS.  Nothing here needs a GPU.

The kernel feeds the SHORTER string of a pair, as text, to the bit-parallel recurrence in words of four units, and after a
word (every ``STOP_EVERY`` words, never after the text's last) it stops where LCS so far + text units left < need.  Two
things must hold for the hits to stay what they were: a pair with LCS >= need is never stopped, and a call that is not
stopped returns the exact LCS.  (A stopped call returns the count so far, which is then below need: the callers only
compare with need.)  Checked on the families of tests/support/lcs_abandon.py (matches that come late, every pairing of
lengths around the word and the 32-lane edges, thresholds 1.0 and 0, a 4-letter alphabet) and on a seeded sample of the
C3 generators' pairs that survive the histogram filters (buckets = the generators' codes & 31), for a test after every word,
every second and every fourth word; the kernel ships ``support.lcs_abandon.STOP_EVERY``.
"""
import functools
import itertools
import random

import numpy as np
import pytest

from support import lcs_abandon as la

EVERY = (1, 2, 4)


def _check_pairs(pairs, thr, every):
    """The two properties on ``pairs`` of strings; returns (pairs stopped, text units processed, text units in all)."""
    stopped_n = done = total = 0
    for x, y in pairs:
        need = la.pair_need(thr, x, y)
        if need is None:
            continue
        exact = la.lcs_dp(x, y)
        got, stopped, units = la.model(x, y, need, every)
        if stopped:
            assert exact < need, (x, y, need, exact)
            assert got < need and got <= exact
        else:
            assert got == exact, (x, y, need)
            assert units == min(len(x), len(y))
        # need = 0 never stops
        assert not la.model(x, y, 0, every)[1]
        stopped_n += stopped
        done += units
        total += min(len(x), len(y))
    return stopped_n, done, total


def test_quick_lcs_is_the_dp():
    rng = random.Random(7)
    for _ in range(300):
        x = "".join(rng.choice("abcdef") for _ in range(rng.randint(0, 64)))
        y = "".join(rng.choice("abcdef") for _ in range(rng.randint(0, 64)))
        assert la.lcs_bits(x, y) == la.lcs_dp(x, y) == la.model(x, y, 0)[0]


def test_shipped_granularity_is_checked():
    assert la.STOP_EVERY in EVERY


@pytest.mark.parametrize("every", EVERY)
def test_late_matches(every):
    left, right, planned = la.late_matches()
    assert {d for _, _, d in planned} == {0, -1}
    for i, j, d in planned:
        x, y = left[i], right[j]
        need = la.pair_need(0.8, x, y)
        assert sorted(x) == sorted(y) and la.lcs_dp(x, y) == need + d and la.reaches_lcs(0.8, x, y)
    stopped, _, _ = _check_pairs([(left[i], right[j]) for i, j, _ in planned], 0.8, every)
    # (a pair one short of need is found out at the latest in front of the last word)
    assert stopped > 0
    rng = random.Random(every)
    _check_pairs(rng.sample(list(itertools.product(left, right)), 300), 0.8, every)


@pytest.mark.parametrize("every", EVERY)
def test_roles_and_word_edges(every):
    left, right, planned = la.roles_and_word_edges()
    combos = set()
    for i, j, d in planned:
        x, y = left[i], right[j]
        need = la.pair_need(0.4, x, y)
        assert la.lcs_dp(x, y) == need + d and la.reaches_lcs(0.4, x, y), (len(x), len(y), d)
        combos.add((len(x), len(y), d))
    assert combos == {(p, q, d) for p in la.ROLE_LENGTHS for q in la.ROLE_LENGTHS for d in (0, -1)}
    assert {min(p, q) % 4 for p, q, _ in combos} == {0, 1, 2, 3}
    _check_pairs([(left[i], right[j]) for i, j, _ in planned], 0.4, every)
    rng = random.Random(10 + every)
    for thr in (0.4, 0.8):
        _check_pairs(rng.sample(list(itertools.product(left, right)), 250), thr, every)


@pytest.mark.parametrize("every", EVERY)
def test_thresholds_one_and_zero(every):
    left, right, planned = la.threshold_one()
    assert {d for _, _, d in planned} == {0, -1}
    for i, j, d in planned:
        assert la.lcs_dp(left[i], right[j]) == len(left[i]) + d and la.reaches_lcs(1.0, left[i], right[j])
    _check_pairs(list(itertools.product(left, right)), 1.0, every)
    left, right = la.threshold_zero()
    pairs = list(itertools.product(left, right))
    stopped, done, total = _check_pairs(random.Random(3).sample(pairs, 300), 0.0, every)
    assert stopped == 0 and done == total


@pytest.mark.parametrize("every", EVERY)
def test_four_letters(every):
    left, right = la.crowded_drain()
    pairs = [(x, y) for x, y in itertools.product(left[:24], right[:60]) if la.reaches_lcs(0.8, x, y)]
    assert len(pairs) > 200
    stopped, done, total = _check_pairs(pairs[:400], 0.8, every)
    assert 0 < stopped < len(pairs[:400])


@functools.lru_cache(maxsize=None)
def _c3_survivors(n=4000):
    """The pairs of the seeded C3 generators at n x n that pass the length filter and the 32-bucket test at 0.8."""
    from napkon_string_matching_amd import synthetic

    (lc, ll), (rc, rl) = synthetic.c3_corpus(n, n)
    hist = lambda codes, length: np.stack([np.bincount(row[:k] & 31, minlength=32) for row, k in zip(codes, length)]).astype(np.int16)
    lh, rh = hist(lc, ll), hist(rc, rl)
    needs = np.array([la.need_of(0.8, s) if s >= 2 and la.need_of(0.8, s) is not None else 255 for s in range(129)], dtype=np.int32)
    out = []
    for i0 in range(0, n, 250):
        sl = slice(i0, i0 + 250)
        need = needs[ll[sl, None] + rl[None, :]]
        ok = np.minimum(ll[sl, None], rl[None, :]) >= need
        common = np.minimum(lh[sl, None, :], rh[None, :, :]).sum(axis=2)
        for i, j in zip(*np.nonzero(ok & (common >= need))):
            out.append((synthetic.decode_strings(lc[i0 + i : i0 + i + 1], ll[i0 + i : i0 + i + 1])[0],
                        synthetic.decode_strings(rc[j : j + 1], rl[j : j + 1])[0]))
    return out


@pytest.mark.parametrize("every", EVERY)
def test_c3_sample(every, capsys):
    """The seeded C3 sample: both properties, and (printed, not asserted) the share of text units that are processed,
    with the shorter string as text and, for comparison, with the right string as text as before."""
    pairs = _c3_survivors()
    assert len(pairs) >= 40
    stopped, done, total = _check_pairs(pairs, 0.8, every)
    right_done = right_total = 0
    for x, y in pairs:  # the roles of before: the right string is the text whatever its length
        need = la.pair_need(0.8, x, y)
        units = la.model(x, y, need, every, shorter_as_text=False)[2]
        right_done += units
        right_total += len(y)
    with capsys.disabled():
        print(f"\n[lcs abandon] C3 4000 x 4000, stop test every {every} word(s): {len(pairs)} pairs reach the LCS, {stopped} stopped; "
              f"text units processed {done / total:.2f} (shorter string as text; of the full right strings: {done / right_total:.2f}), "
              f"{right_done / right_total:.2f} (right string as text)")
