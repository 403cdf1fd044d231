"""The FP4 codes of the matrix-pipe scan (csrc/indel_raw_coarse.hpp, NSM_C3C_FP4), checked without a GPU on their Python
restatement (tests/support/scan_fp4.py): the bucket bound for every pair of counts and every scale, the kernel's word
arithmetic (the v_perm_b32 byte table included) against a per-byte loop, the rounding of the excess, the scale choice, the
bound on a seeded sample of the benchmark's strings, and a model of the FP4 MFMA on exact data (what tools/mfma_fp4_probe
checks on the GPU).
"""
import functools
import random

import numpy as np
import pytest

from tests.support import scan_fp4 as fp4

NEVER = 255  # csrc/nsm_common.hpp: kNever


def _scales_of(r):
    """Every scale a right string with a count of r can have: its own smallest one, or a larger one from another bucket."""
    return range(fp4.scale_of([r]), 4)


def test_bucket_bound():
    """D_b >= min(a, r) for all counts and every scale; D_b = min(a, r) where a <= 3 and k = 0; D_b >= r where a >= 4."""
    for a in range(65):
        for r in range(65):
            for k in _scales_of(r):
                d = fp4.bucket(a, r, k)
                assert d >= min(a, r), (a, r, k, d)
                assert d * 2 == int(d * 2)  # a multiple of 1/2
                if a <= 3 and k == 0:
                    assert d == min(a, r), (a, r, d)
                if a <= 3:
                    assert d == min(a, r, 2) + (1 << k) * (a >= 3 and r >= 3), (a, r, k, d)
                else:
                    assert d >= r, (a, r, k, d)


def test_excess_rounds_up_and_is_monotone():
    for k in range(4):
        last = 0.0
        for r in range(65):
            if k < fp4.scale_of([r]):
                continue
            e = 2.0 * fp4.FP4[fp4.excess_nibble(r, k)] * (1 << k)  # the left indicator is 2.0
            assert e >= max(r - 3, 0) and e >= last, (r, k, e)
            assert e < max(r - 3, 0) + 4 * (1 << k) or r <= 3, (r, k, e)  # and never far above it
            last = e
    assert [fp4.excess_nibble(3 + q, 0) for q in range(13)] == [0, 1, 2, 3, 4, 5, 5, 6, 6, 7, 7, 7, 7]
    assert [2 * fp4.FP4[c] for c in range(8)] == [0, 1, 2, 3, 4, 6, 8, 12]


def test_scale_choice():
    """The smallest k at which the largest excess fits, and the kernel's word form of it (k = 0 from the OR of the words)."""
    for top in range(65):
        k = fp4.scale_of([top, 1, 0])
        assert top - 3 <= 12 << k and (k == 0 or top - 3 > 12 << (k - 1)), (top, k)
    assert [fp4.scale_of([t]) for t in (15, 16, 27, 28, 51, 52, 64)] == [0, 1, 1, 2, 2, 3, 3]
    rng = random.Random(7)
    for _ in range(3000):
        counts = [0] * 32
        left = 64
        for b in rng.sample(range(32), rng.randint(1, 8)):
            counts[b] = rng.randint(0, min(left, rng.choice((3, 15, 16, 28, 52, 64))))
            left -= counts[b]
        words = [sum(c << (8 * i) for i, c in enumerate(counts[4 * q : 4 * q + 4])) for q in range(8)]
        assert fp4.scale_of_words(words) == fp4.scale_of(counts), counts
    # a count of 8 and one of 7 in different words: their OR has no bit above 15 (k = 0), each alone neither
    assert fp4.scale_of_words([0x08, 0x07] + [0] * 6) == 0 and fp4.scale_of_words([0x10] + [0] * 7) == 1


def _word(c, pos, neighbour):
    return sum((c if i == pos else neighbour) << (8 * i) for i in range(4))


@pytest.mark.parametrize("form", [fp4.left_words_perm, fp4.left_words_plain])
def test_left_words(form):
    """Every count in every byte position, beside neighbours of 0 and of 64: no carry, no leak between the bytes."""
    for c in range(65):
        for pos in range(4):
            for neighbour in (0, 64):
                m1, m2 = form(_word(c, pos, neighbour))
                for i in range(4):
                    want = fp4.left_bytes(c if i == pos else neighbour)
                    assert ((m1 >> (8 * i)) & 0xFF, (m2 >> (8 * i)) & 0xFF) == want, (c, pos, neighbour, i)
    rng = random.Random(3)
    for _ in range(2000):
        q = [rng.randint(0, 64) for _ in range(4)]
        m1, m2 = form(sum(c << (8 * i) for i, c in enumerate(q)))
        assert [((m1 >> (8 * i)) & 0xFF, (m2 >> (8 * i)) & 0xFF) for i in range(4)] == [fp4.left_bytes(c) for c in q]


def test_perm_model():
    """The selector never takes a value of 4 .. 12 (table bytes the scan does not define, and the instruction's sign and
    zero selectors)."""
    for c in range(65):
        sel = (c + 0x3C) & 0x43
        assert sel == c if c < 4 else sel >= 0x40
    assert fp4.perm(0x07060504, 0x03020100, 0x0C0D0306) == 0x00FF0306 | 0x0000_0000
    assert fp4.perm(0x80000000, 0x00008000, 0x0B0A0908) == 0xFF0000FF


def test_right_words():
    for c in range(65):
        for pos in range(4):
            for neighbour in (0, 64):
                for k in range(max(fp4.scale_of([c]), fp4.scale_of([neighbour])), 4):
                    m1, m2 = fp4.right_words(_word(c, pos, neighbour), k)
                    for i in range(4):
                        want = fp4.right_bytes(c if i == pos else neighbour, k)
                        assert ((m1 >> (8 * i)) & 0xFF, (m2 >> (8 * i)) & 0xFF) == want, (c, pos, neighbour, k, i)
                        assert want[0] & 0x88 == 0 and want[1] & 0x88 == 0  # no nibble has the sign bit
    # k = 0, the byte tables: every count 0 .. 15 beside neighbours of 0 and 15, and random words
    rng = random.Random(9)
    words = [_word(c, pos, nb) for c in range(16) for pos in range(4) for nb in (0, 15)]
    words += [sum(rng.randint(0, 15) << (8 * i) for i in range(4)) for _ in range(2000)]
    for w in words:
        m1, m2 = fp4.right_words(w, 0)
        assert [((m1 >> (8 * i)) & 0xFF, (m2 >> (8 * i)) & 0xFF) for i in range(4)] == [fp4.right_bytes((w >> (8 * i)) & 0xFF, 0) for i in range(4)], hex(w)


def test_no_bound_reaches_never():
    """The largest D any right string of at most 64 units can give (every left count >= 4) is at most 128, below kNever - 1/2."""
    worst = 0.0
    for k in range(4):
        gain = [fp4.bucket(64, r, k) if fp4.scale_of([r]) <= k else None for r in range(65)]
        # a string has the scale k > 0 because ONE of its counts, `top`, needs it; the other buckets share what is left
        for top in [r for r in range(65) if fp4.scale_of([r]) == k] if k else [0]:
            best = [0.0] * (65 - top)  # best[u]: the largest sum with u units spent in the other buckets
            for _ in range(31):
                nxt = list(best)
                for u in range(65 - top):
                    for r in range(1, 65 - top - u):
                        if gain[r] is not None:
                            nxt[u + r] = max(nxt[u + r], best[u] + gain[r])
                best = nxt
            worst = max(worst, gain[top] + max(best))
    assert 64 <= worst <= 128 < NEVER - 0.5, worst  # (the kernel's comment says D <= 128)


@functools.lru_cache(maxsize=None)
def _sample():
    """2000 x 2000 strings of the benchmark's generator: histograms over code & 31, lengths, and the scan's operands."""
    from napkon_string_matching_amd import synthetic

    (lc, ll), (rc, rl) = synthetic.strings(2000, 1234), synthetic.strings(2000, 5678)

    def hist(codes, length):
        h = np.zeros((codes.shape[0], 32), dtype=np.int64)
        for i, (row, n) in enumerate(zip(codes, length)):
            np.add.at(h[i], row[:n] & 31, 1)
        return h

    return hist(lc, ll), ll.astype(np.int64), hist(rc, rl), rl.astype(np.int64)


def _need_table(thr):
    """need[s]: the smallest LCS with which strings of la + lb = s reach ``thr`` (csrc/indel_score.hpp, the same doubles)."""
    need = np.full(129, NEVER, dtype=np.int64)
    for s in range(1, 129):
        for lcs in range(s // 2 + 1):
            if (1.0 - float(s - 2 * lcs) / float(s)) * 100.0 / 100.0 >= thr:
                need[s] = lcs
                break
    return need


def test_sample_keeps_every_candidate_and_beats_cap3():
    """On the sample at threshold 0.8: no pair with sum of min >= need is dropped, and fewer pairs pass than with the i8
    CAP 3 code -- a condition on the design, not a timing."""
    lh, ll, rh, rl = _sample()
    need = _need_table(0.8)[ll[:, None] + rl[None, :]]
    fits = np.minimum(ll[:, None], rl[None, :]) >= need
    ks = np.array([fp4.scale_of(list(r)) for r in rh])
    # D as four matrix products of the decoded slot values, as the MFMAs compute it
    d = np.zeros((2000, 2000))
    for slot in range(4):
        left = np.array([[fp4.FP4[(fp4.left_bytes(int(c))[slot >> 1] >> (4 * (slot & 1))) & 0xF] for c in row] for row in lh])
        right = np.array([[fp4.FP4[(fp4.right_bytes(int(c), int(k))[slot >> 1] >> (4 * (slot & 1))) & 0xF] for c in row] for row, k in zip(rh, ks)])
        if slot >= 2:
            right = right * (2.0 ** ks)[:, None]
        d += left @ right.T
    sum_min = sum((lh >= t).astype(np.float64) @ (rh >= t).astype(np.float64).T for t in range(1, 65))
    # the i8 CAP 3 bound: min(a, r) where r < 3, a where r >= 3
    small = np.where(rh < 3, rh, 0)
    cap3 = sum((lh >= t).astype(np.float64) @ (small >= t).astype(np.float64).T for t in (1, 2)) + lh.astype(np.float64) @ (rh >= 3).astype(np.float64).T
    assert (d >= sum_min).all() and (cap3 >= sum_min).all()
    exact = fits & (sum_min >= need)
    pass_fp4 = fits & (d > need - 0.5)
    pass_cap3 = fits & (cap3 >= need)
    assert exact.sum() > 0 and not (exact & ~pass_fp4).any()
    assert pass_fp4.sum() < pass_cap3.sum(), (int(pass_fp4.sum()), int(pass_cap3.sum()))
    assert (ks == 0).all()  # no string of the benchmark needs a scale


def test_mfma_model_on_exact_data():
    """The model of the instruction (operand map, nibble order, block scale per lane) against a plain loop over decoded
    matrices: the data of tools/mfma_fp4_probe, A != B^T, one column with a B scale of 2."""
    a_code = [[(i * 5 + k * 3 + (k >> 4)) % 8 for k in range(64)] for i in range(32)]
    b_code = [[(j * 3 + k * 7 + (j >> 3) + 1) % 8 for j in range(32)] for k in range(64)]
    a_regs = [[0] * 4 for _ in range(64)]
    b_regs = [[0] * 4 for _ in range(64)]
    for lane in range(64):
        for j in range(32):
            k = 32 * (lane >> 5) + j
            a_regs[lane][j >> 3] |= a_code[lane & 31][k] << (4 * (j & 7))
            b_regs[lane][j >> 3] |= b_code[k][lane & 31] << (4 * (j & 7))
    scales = [128 if lane & 31 == 21 else 127 for lane in range(64)]
    plain, scaled = fp4.mfma_fp4(a_regs, b_regs), fp4.mfma_fp4(a_regs, b_regs, scales)
    for row in range(32):
        for col in range(32):
            want = sum(fp4.FP4[a_code[row][k]] * fp4.FP4[b_code[k][col]] for k in range(64))
            assert plain[row][col] == want and scaled[row][col] == want * (2 if col == 21 else 1), (row, col)
    assert sorted(fp4.c_layout(lane, reg) for lane in range(64) for reg in range(16)) == [(r, c) for r in range(32) for c in range(32)]
