"""The value-table codes of the PACKED FP4 scan (csrc/indel_raw_coarse.hpp, NSM_C3C_CODES2), restated in plain Python on top
of tests/support/scan_fp4.py.

Per bucket, with a the left count, r the right count (0 .. 64) and k the right string's scale exponent (scan_fp4.scale_of),

    D_b = [a >= 1][r >= 1] + [a >= 2][r >= 2] + 2^k (x3(A) y3(R) + x4(A) y4(R)),    A = min(a, 15),  R = entry(r, k)

with the four tables below over the counts 0 .. 15 (E2M1 values; the output of tools/c3_code_search.py) and
entry(r, k) = r for k = 0, else 2 + ceil((max(r, 2) - 2) / 2^k).  Slots 1 and 2 are the first MFMA's, as before; the byte of a
count in the second MFMA's operand word is slot 3's code in the low nibble and slot 4's in the high one.  Products are
multiples of 1/4, so the OR fold keeps 4 D in 11-bit fields:

    BIAS = 2^23 + (1024 - 4 need_hi) 2^11 + (1024 - 4 need_lo),   B scale bytes 0x7f + 13 (+ k) and 0x7f + 2 (+ k),
    flag bits 21 and 10.
"""
from tests.support import scan_fp4 as fp4

X3 = (0, 0, 0, 4, 4, 4, 4, 4, 4, 4, 4, 5, 6, 6, 6, 7)  # E2M1 codes by count
X4 = (0, 0, 0, 0, 2, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4)
Y3 = (0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3)
Y4 = (0, 0, 0, 0, 2, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 5)
LEFT_WORDS = (0x04000000, 0x44342424, 0x45444444, 0x47464646)   # kC3cLeft2: counts 0 - 3, 4 - 7, 8 - 11, 12 - 15
RIGHT_WORDS = (0x01000000, 0x41414121, 0x52525151, 0x53535352)  # kC3cRight2
ONES = 0x01010101

NEVER = 255
FIELD_BITS, FIELD_FRAC = 11, 2
FLAG_LO, FLAG_HI = 1 << (FIELD_BITS - 1), 1 << (2 * FIELD_BITS - 1)
F32_ONE_ULP = 0x4B000000


def entry(r, k):
    """The right tables' index of a count."""
    return r if k == 0 else 2 + ((max(r, 2) - 2 + (1 << k) - 1) >> k)


def left_bytes(a):
    return fp4.left_bytes(a)[0], X3[min(a, 15)] | (X4[min(a, 15)] << 4)


def right_bytes(r, k):
    e = entry(r, k)
    assert e <= 15, (r, k)
    return fp4.right_bytes(r, k)[0], Y3[e] | (Y4[e] << 4)


def slots34(a, r, k):
    """x3 y3 + x4 y4, before the block scale."""
    (_, lb), (_, rb) = left_bytes(a), right_bytes(r, k)
    return fp4.FP4[lb & 15] * fp4.FP4[rb & 15] + fp4.FP4[lb >> 4] * fp4.FP4[rb >> 4]


def bucket(a, r, k):
    return min(a, r, 2) + (1 << k) * slots34(a, r, k)


def bound(left_counts, right_counts):
    k = fp4.scale_of(right_counts)
    return sum(bucket(a, r, k) for a, r in zip(left_counts, right_counts))


def _table_bytes(w, words):
    """c3c_codes2_bytes: four counts 0 .. 15 through two byte tables."""
    assert w & 0xF0F0F0F0 == 0
    sel = w & 0x07070707
    big = ((w >> 3) & ONES) * 0xFF
    return (big & fp4.perm(words[3], words[2], sel)) | (~big & 0xFFFFFFFF & fp4.perm(words[1], words[0], sel))


def left_words(w):
    """c3c_fp4_left_packed."""
    total = w + 0x70707070
    assert total < 1 << 32
    over = ((total >> 7) & ONES) * 0xFF
    return fp4.left_words_perm(w)[0], _table_bytes((w | over) & 0x0F0F0F0F, LEFT_WORDS)


def right_words(w, k):
    """c3c_codes2_right_k0 and c3c_codes2_right_scaled."""
    m1 = fp4.right_words(w, k)[0]
    if k == 0:
        return m1, _table_bytes(w, RIGHT_WORDS)
    lo, hi = RIGHT_WORDS[0] | (RIGHT_WORDS[1] << 32), RIGHT_WORDS[2] | (RIGHT_WORDS[3] << 32)
    m2 = 0
    for b in range(4):
        r = (w >> (8 * b)) & 0xFF
        e = min(2 + ((max(r, 2) - 2 + (1 << k) - 1) >> k), 15)
        m2 |= (((hi if e & 8 else lo) >> (8 * (e & 7))) & 0xFF) << (8 * b)
    return m1, m2


# --- the OR fold with 11-bit fields ----------------------------------------------------------------------------------------------


def bias(need_hi, need_lo):
    for need in (need_hi, need_lo):
        assert 0 <= need <= 64 or need == NEVER, need
    return (1 << 23) + (((256 - need_hi) << FIELD_FRAC) << FIELD_BITS) + ((256 - need_lo) << FIELD_FRAC)


def bias_bits(need_hi, need_lo):
    """The kernel's form: the f32 bit pattern, made with integer instructions."""
    return F32_ONE_ULP | (((256 - need_hi) << FIELD_FRAC) << FIELD_BITS) | ((256 - need_lo) << FIELD_FRAC)


def scale_bytes(tile, k):
    """The E8M0 B scale bytes of a tile's two MFMAs: (slots 1 and 2, slots 3 and 4)."""
    base = 0x7F + FIELD_FRAC + (FIELD_BITS if tile % 2 == 0 else 0)
    return base, base + k


def fields(bits):
    """(field hi, field lo) of an f32 bit pattern in [2^23, 2^24)."""
    assert bits & 0xFF800000 == F32_ONE_ULP
    n = bits & 0x7FFFFF
    assert n >> (2 * FIELD_BITS) == 0
    return n >> FIELD_BITS, n & ((1 << FIELD_BITS) - 1)


def operand_regs(hists, side, ks=None):
    """The two MFMAs' operand registers of 32 strings (32-bucket histograms): regs[m][lane][4], lane = string + 32 half."""
    regs = [[[0] * 4 for _ in range(64)] for _ in range(2)]
    for lane in range(64):
        s, half = lane & 31, lane >> 5
        for j in range(16):
            c = hists[s][16 * half + j]
            pair = left_bytes(c) if side == "left" else right_bytes(c, ks[s])
            for m in range(2):
                regs[m][lane][j >> 2] |= pair[m] << (8 * (j & 3))
    return regs


def chain(left_hists, hi_hists, lo_hists, lane_need):
    """The four MFMAs of a tile pair on scan_fp4's instruction model, f32 accumulation with one rounding per MFMA:
    bits[lane][reg].  lane_need[col] = (need_hi, need_lo).  Asserts that every partial sum is an integer below 2^24."""
    import numpy as np

    a = operand_regs(left_hists, "left")
    acc = np.array([[np.float32(bias(*lane_need[lane & 31]))] * 16 for lane in range(64)], dtype=np.float32)
    assert [int(x) for x in acc[:, 0].view(np.uint32)] == [bias_bits(*lane_need[lane & 31]) for lane in range(64)]
    exact = acc.astype(np.float64)
    for tile, hists in ((0, hi_hists), (1, lo_hists)):
        ks = [fp4.scale_of(list(h)) for h in hists]
        b = operand_regs(hists, "right", ks)
        for m in range(2):
            scales = [scale_bytes(tile, ks[lane & 31])[m] for lane in range(64)]
            out = fp4.mfma_fp4(a[m], b[m], scales)
            add = np.array([[out[fp4.c_layout(lane, reg)[0]][lane & 31] for reg in range(16)] for lane in range(64)])
            assert (add == np.floor(add)).all()
            exact = exact + add
            acc = (acc + add.astype(np.float32)).astype(np.float32)
            assert (acc.astype(np.float64) == exact).all() and (exact < 1 << 24).all()
    return acc.view(np.uint32)
