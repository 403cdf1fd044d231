"""The OR fold of the FP4 scan (csrc/indel_raw_coarse.hpp, NSM_C3C_ORFOLD), checked without a GPU on its Python restatement
(tests/support/scan_orfold.py): the bias, the two fixed-point fields and their flag bits for every pair of results and every
need, in f32 arithmetic and in both accumulation orders; the carry guard; the block scales on either tile through the model
of the instruction; the per-lane minimum of the needs on a sample of the benchmark's strings; and the stack's bound with 128
pushes per tile pair.
"""
import functools
import random

import numpy as np
import pytest

from tests.support import scan_fp4 as fp4
from tests.support import scan_orfold as orf

NEEDS = list(range(65)) + [orf.NEVER]
D = np.arange(129, dtype=np.int64)


def test_bias_forms_agree():
    for nh in NEEDS:
        for nl in NEEDS:
            value = orf.bias(nh, nl)
            assert 1 << 23 <= value < 1 << 24
            assert int(np.array([value], dtype=np.float32).view(np.uint32)[0]) == orf.bias_bits(nh, nl)


@pytest.mark.parametrize("order", ["hi first", "lo first", "interleaved"])
def test_flags_for_every_result_and_need(order):
    """Every D_hi, D_lo in 0 .. 128 against every need in 0 .. 64 and kNever: the fields are D + 256 - need, the flags are
    D >= need, whatever the order of the four f32 additions (each D in two parts, as two MFMAs deliver it)."""
    d_hi, d_lo = D[:, None, None], D[None, :, None]
    nl = np.array(NEEDS, dtype=np.int64)[None, None, :]
    parts_hi = [(d_hi // 3) * 512.0, (d_hi - d_hi // 3) * 512.0]
    parts_lo = [(d_lo // 2) * 1.0, (d_lo - d_lo // 2) * 1.0]
    terms = {"hi first": parts_hi + parts_lo, "lo first": parts_lo + parts_hi,
             "interleaved": [parts_hi[0], parts_lo[0], parts_hi[1], parts_lo[1]]}[order]
    for nh in NEEDS:
        start = np.broadcast_to((1 << 23) + ((256 - nh) << 9) + (256 - nl), (129, 129, len(NEEDS))).astype(np.float32)
        assert (start.view(np.uint32) == (orf.F32_ONE_ULP | ((256 - nh) << 9) | (256 - nl))).all()
        bits = orf.accumulate(start, [np.broadcast_to(t, (129, 129, len(NEEDS))) for t in terms])
        f_hi, f_lo = orf.fields(bits)
        assert (f_hi == d_hi + 256 - nh).all() and (f_lo == d_lo + 256 - nl).all()
        p_hi, p_lo = orf.flags(bits)
        assert (p_hi == (d_hi >= nh)).all() and (p_lo == (d_lo >= nl)).all()


def test_no_carry_between_the_fields():
    """D = 128 and need = 0 is the largest field, 384 < 512: the neighbour's field and flag are its own."""
    for other_d, other_need in ((0, 1), (0, orf.NEVER), (63, 64), (64, 64), (128, 0)):
        for big_is_lo in (True, False):
            nh, nl = (other_need, 0) if big_is_lo else (0, other_need)
            dh, dl = (other_d, 128) if big_is_lo else (128, other_d)
            bits = orf.accumulate(np.float32(orf.bias(nh, nl)), [512.0 * dh, 1.0 * dl])
            f_hi, f_lo = (int(x) for x in orf.fields(bits))
            assert (f_hi, f_lo) == (dh + 256 - nh, dl + 256 - nl) and max(f_hi, f_lo) == 384
            p_hi, p_lo = orf.flags(bits)
            assert (bool(p_hi), bool(p_lo)) == (dh >= nh, dl >= nl)
    # never: the field of a column that cannot fit is at most 129
    assert 128 + 256 - orf.NEVER == 129 < 256


def test_scale_bytes():
    assert [orf.scale_bytes(t, 0) for t in range(4)] == [(0x88, 0x88), (0x7F, 0x7F), (0x88, 0x88), (0x7F, 0x7F)]
    assert orf.scale_bytes(2, 3) == (0x88, 0x8B) and orf.scale_bytes(3, 2) == (0x7F, 0x81)


def _hist(rng, top, length=64):
    """A 32-bucket histogram of `length` units with one count of `top`."""
    counts = [0] * 32
    counts[rng.randrange(32)] = top
    left = length - top
    while left:
        b = rng.randrange(32)
        if counts[b] == top:
            continue
        n = min(left, rng.randint(1, 5))
        counts[b] += n
        left -= n
    return counts


def test_chain_on_the_instruction_model():
    """A tile pair through the model of v_mfma_f32_32x32x64_f8f6f4: right strings with k = 0, 1, 2 and 3 in the even and in
    the odd tile, needs per column (kNever among them): every field is the sum of the bucket bounds + 256 - need and every
    flag the test the max fold made, and the fold of a lane is the OR over its 16 rows."""
    rng = random.Random(17)
    tops = (5, 16, 28, 52)  # k = 0 .. 3
    lefts = [_hist(rng, rng.choice((3, 4, 9, 30)), rng.randint(40, 64)) for _ in range(32)]
    hi = [_hist(rng, tops[c % 4]) for c in range(32)]
    lo = [_hist(rng, tops[(c // 4) % 4]) for c in range(32)]
    assert {fp4.scale_of(h) for h in hi} == {0, 1, 2, 3} == {fp4.scale_of(h) for h in lo}
    d = lambda a, r: sum(fp4.bucket(x, y, fp4.scale_of(r)) for x, y in zip(a, r))
    d_hi = [[d(a, r) for r in hi] for a in lefts]
    d_lo = [[d(a, r) for r in lo] for a in lefts]
    assert max(map(max, d_hi)) <= 128 and max(map(max, d_lo)) <= 128
    # needs around the results of the column, so that flags of both kinds occur; columns that cannot fit in one tile or in both
    need = []
    for c in range(32):
        col_hi, col_lo = sorted(row[c] for row in d_hi), sorted(row[c] for row in d_lo)
        need.append((orf.NEVER if c in (7, 11) else min(64, int(col_hi[24])), orf.NEVER if c in (9, 11) else min(64, int(col_lo[8]))))
    bits = orf.chain(lefts, hi, lo, need)
    seen = set()
    for lane in range(64):
        col = lane & 31
        want_hi = want_lo = False
        for reg in range(16):
            row = fp4.c_layout(lane, reg)[0]
            f_hi, f_lo = (int(x) for x in orf.fields(bits[lane][reg]))
            assert f_hi == d_hi[row][col] + 256 - need[col][0] and f_lo == d_lo[row][col] + 256 - need[col][1], (lane, reg)
            want_hi |= d_hi[row][col] >= need[col][0]
            want_lo |= d_lo[row][col] >= need[col][1]
        top = orf.fold(bits[lane])
        assert (bool(top & orf.FLAG_HI), bool(top & orf.FLAG_LO)) == (want_hi, want_lo), lane
        seen.add((want_hi, want_lo))
    assert len(seen) == 4  # lanes with no flag, with either and with both


def test_lane_needs():
    assert orf.lane_needs([10, 20, 12, 18]) == (10, 18)
    assert orf.lane_needs([orf.NEVER, 20, 12, orf.NEVER]) == (12, 20)
    assert orf.lane_needs([orf.NEVER, 0, orf.NEVER, orf.NEVER]) == (orf.NEVER, 0)


@functools.lru_cache(maxsize=None)
def _sample():
    """2000 x 2000 strings of the benchmark's generator in table order (longest first): histograms over code & 31, lengths."""
    from napkon_string_matching_amd import synthetic

    def table(n, seed):
        codes, length = synthetic.strings(n, seed)
        order = np.argsort(-length.astype(np.int64), kind="stable")
        codes, length = codes[order], length[order].astype(np.int64)
        h = np.zeros((n, 32), dtype=np.int64)
        for i, (row, k) in enumerate(zip(codes, length)):
            np.add.at(h[i], row[:k] & 31, 1)
        return h, length

    return table(2000, 1234) + table(2000, 5678)


def _need_table(thr):
    need = np.full(129, orf.NEVER, dtype=np.int64)
    for s in range(1, 129):
        for lcs in range(s // 2 + 1):
            if (1.0 - float(s - 2 * lcs) / float(s)) * 100.0 / 100.0 >= thr:
                need[s] = lcs
                break
    return need


def test_lane_minimum_keeps_every_pair_on_the_sample(capsys):
    """On the sample at threshold 0.8, right strings in waves of 128 in table order: with the need of a lane the minimum
    over its tiles of one parity, every pair that the per-tile test passes still passes; a wave whose strings straddle a
    length boundary passes a few more, which are reported."""
    lh, ll, rh, rl = _sample()
    assert all(fp4.scale_of(list(r)) == 0 for r in rh)
    # D with k = 0: min(a, r, 3) + [a >= 4] E(r), E the rounded excess
    excess = np.array([2 * fp4.FP4[fp4.excess_nibble(r, 0)] if r <= 15 else 0 for r in range(65)])
    d = sum((lh >= t).astype(np.float64) @ (rh >= t).astype(np.float64).T for t in (1, 2, 3)) + (lh >= 4).astype(np.float64) @ excess[rh].T
    need = _need_table(0.8)[ll[:, None] + rl[None, :]]
    need = np.where(np.minimum(ll[:, None], rl[None, :]) >= need, need, orf.NEVER)  # the exact length filter
    own = d >= need
    lane = np.full_like(need, orf.NEVER)
    mixed_waves = 0
    for j0 in range(0, 2000, 128):
        for parity in (0, 1):
            cols = [np.arange(j0 + 32 * t, min(j0 + 32 * t + 32, 2000)) for t in range(parity, orf.NT, 2)]
            cols = [c for c in cols if len(c)]
            width = max(len(c) for c in cols)
            stack = np.full((len(cols), 2000, width), orf.NEVER)
            for n, c in enumerate(cols):
                stack[n, :, : len(c)] = need[:, c]
            low = stack.min(axis=0)  # [left row][lane]: the lane's need in a class is that of any of its rows
            for c in cols:
                lane[:, c] = low[:, : len(c)]
        mixed_waves += len(set(rl[j0 : j0 + 128])) > 1
    assert (lane <= need).all()
    loose = d >= lane
    assert own.sum() > 0 and not (own & ~loose).any()
    extra = int(loose.sum() - own.sum())
    with capsys.disabled():
        print(f"\n  OR fold, per-lane minimum need on 2000 x 2000: {int(own.sum())} pairs pass the per-tile test, {extra} more "
              f"({100.0 * extra / own.sum():.2f} %) the per-lane one; {mixed_waves} of {(2000 + 127) // 128} waves hold more than one length")
    assert extra <= own.sum()  # a few more, not a different filter


def test_stack_bound():
    """The pipelined scan pushes at most NT x 64 entries between two checks and one tile pair's, 128, after the check that
    decides on a drain: with every pair full the stack is exactly full, and nothing exceeds it."""
    full = [[128, 128]] * 40
    top, _ = orf.high_water(full)
    assert top == orf.DRAIN_AT + (orf.NT + 2) * orf.WAVE == orf.STACK
    rng = random.Random(5)
    worst = 0
    for _ in range(300):
        blocks = [[rng.choice((0, 0, 3, 64, 127, 128)) for _ in range(2)] for _ in range(rng.randint(1, 60))]
        top, left = orf.high_water(blocks, q=rng.randint(0, orf.DRAIN_AT))
        assert top <= orf.STACK
        worst = max(worst, top)
    assert worst > orf.STACK - 2 * orf.WAVE
    # the stack of the per-tile scan, 7 x 64 entries, would not do
    assert orf.high_water(full)[0] > (orf.NT + 3) * orf.WAVE
