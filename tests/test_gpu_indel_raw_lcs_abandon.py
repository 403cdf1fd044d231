"""The per-pair LCS of the RAW fuzzy kernels (csrc/indel_raw.hip: raw_lcs_pair / raw_lcs_units) with its stop rule and its
roles, through the two-stage kernel's drain and through the one-stage kernel, against the exhaustive kernel and the oracle.

The LCS takes the SHORTER string of a pair as text, in words of four units, and stops after a word where LCS so far +
text units left < need.  What can go wrong: a hit stopped (matches that come late: the running count sits at the bound
until the common tail arrives), a count read where the chain had stopped and taken for a hit, the roles (la < lb, la > lb,
la == lb; the text's padding must match nothing whichever table it comes from), the last word of a text of 4 k + 1, 2, 3
units, patterns on both sides of 32 units, need = 0 (nothing may stop), and calls that follow one another in one drain
pass, stopped ones among them.  tests/support/lcs_abandon.py builds the strings; each test first works out on the host
that its pairs at LCS == need and at need - 1 really pass the length filter and the 32-bucket test, so that a stronger
filter in front cannot empty the test unseen.  Hits and scores are compared bit for bit.
"""
import itertools

import pytest

from support import lcs_abandon as la

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _oracle(left, right, thr):
    from oracle import native

    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    return native.indel_raw(cp(left), cp(right), thr, cap=1 << 20)


def _check(dev, left, right, thresholds):
    """The two-stage kernel, the one-stage kernel and the exhaustive kernel against the oracle at every threshold; returns the
    oracle's hits at the lowest one."""
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd import tables as tb

    lt, rt = tb.encode_strings(left, right, dev)
    # (at most 32 symbols: one symbol per bucket, the host's sum of minima is the kernels' 32-bucket bound)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None and lt.alphabet <= 32
    base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in ({}, {"two_stage": False}, {"prune": False}):
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return base


def _assert_planned(thr, left, right, planned, base):
    """The planned pairs reach the LCS with LCS == need + d, both d = 0 and d = -1 occur, and the oracle agrees."""
    hits = {(i, j) for s, i, j in base if s >= thr}
    seen = set()
    for i, j, d in planned:
        x, y = left[i], right[j]
        assert la.reaches_lcs(thr, x, y) and la.lcs_bits(x, y) == la.pair_need(thr, x, y) + d, (i, j, d)
        assert ((i, j) in hits) == (d == 0), (i, j, d)
        seen.add(d)
    assert seen == {0, -1}


def test_late_matches(dev):
    """J.T against J'.T (J' a rearrangement of J with LCS(J, J') = 1 or 3, T common): identical multisets, so both histogram
    tests pass, and the count stays at 1 or 3 through the head; lengths 17 to 64, LCS == need and need - 1.  And T.J against
    T.J', where the count runs ahead and a stop can only come at the end."""
    left, right, planned = la.late_matches()
    base = _check(dev, left, right, (0.8,))
    _assert_planned(0.8, left, right, planned, base)
    assert all(sorted(left[i]) == sorted(right[j]) for i, j, _ in planned)
    assert {len(left[i]) for i, _, _ in planned} >= {17, 32, 33, 63, 64}


def test_roles_and_word_edges(dev):
    """All 81 (la, lb) of {16, 17, 18, 31, 32, 33, 62, 63, 64}^2, one pair at need and one at need - 1 each (threshold 0.4, at
    which every pairing passes the length filter); the same table once more at 0.8, where only pairings of near lengths are
    left and nothing is planned."""
    left, right, planned = la.roles_and_word_edges()
    base = _check(dev, left, right, (0.4, 0.8))
    _assert_planned(0.4, left, right, planned, base)
    combos = {(len(left[i]), len(right[j]), d) for i, j, d in planned}
    assert combos == {(p, q, d) for p in la.ROLE_LENGTHS for q in la.ROLE_LENGTHS for d in (0, -1)}
    assert {min(p, q) % 4 for p, q, _ in combos} == {0, 1, 2, 3}


def test_threshold_one(dev):
    """Identical strings, strings that differ in their first or last unit only (stopped by the histograms), strings with
    their first or last two units exchanged (LCS == need - 1 with the same multiset: stopped by the LCS alone)."""
    left, right, planned = la.threshold_one()
    base = _check(dev, left, right, (1.0,))
    _assert_planned(1.0, left, right, planned, base)
    assert {(i, j) for _, i, j in base} == {(i, j) for i, x in enumerate(left) for j, y in enumerate(right) if x == y}


def test_threshold_zero(dev):
    """need = 0: nothing may stop, every pair of a 40 x 40 grid with empty rows on both sides is a hit with its exact score."""
    left, right = la.threshold_zero()
    base = _check(dev, left, right, (0.0,))
    assert len(base) == 1600 and {(i, j) for _, i, j in base} == set(itertools.product(range(40), range(40)))


def test_crowded_drain(dev):
    """A 4-letter alphabet, 96 left rows of one length (three blocks) x 161 right rows: most pairs reach the LCS, entries
    carry several pairs, the stack passes its drain level inside the class and a drain pass runs many LCS calls one after
    the other, most of them stopped, hits among them."""
    left, right = la.crowded_drain()
    reach = [(i, j) for (i, x), (j, y) in itertools.product(enumerate(left), enumerate(right)) if la.reaches_lcs(0.8, x, y)]
    assert len(reach) > len(left) * len(right) // 3
    base = _check(dev, left, right, (0.6, 0.8))
    hits = {(i, j) for s, i, j in base if s >= 0.8}
    assert 10 <= len(hits) < len(reach) // 4 and hits <= set(reach)
    assert set(la.boundary_pairs(0.8, left, right)) == {0, -1}
