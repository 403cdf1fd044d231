"""The FP4 codes of the matrix-pipe scan (csrc/indel_raw_coarse.hpp, NSM_C3C_FP4), restated in plain Python.

Per bucket, with a the left count and r the right count (0 .. 64) and k the right string's scale exponent, the scan's two
MFMAs compute

    D_b = [a >= 1][r >= 1] + [a >= 2][r >= 2] + 2^k [a >= 3][r >= 3] + 2^k [a >= 4] E

with E the excess max(r - 3, 0) over 2^k, rounded UP to the next of 0, 1, 2, 3, 4, 6, 8, 12.  Every left indicator is the
E2M1 value 2.0 (nibble 4), every right indicator 0.5 (nibble 1), and the right excess nibble holds E / 2.  Slots 1 and 2 are
the low and the high nibble of a count's byte in the first MFMA's operand words, slots 3 and 4 those of the second, which
carries the right string's block scale 2^k.
"""

FP4 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # E2M1 codes 0 .. 7; bit 3 of a nibble is the sign, which the scan never sets
E_TABLE = 0x7777665543210  # nibble 4 q: the code of E / 2 for an excess (over 2^k) of q = 0 .. 12
ONES = 0x01010101


def scale_of(counts):
    """k of a right string: the smallest with max(r) - 3 <= 12 x 2^k."""
    top = max(counts, default=0)
    return 0 if top <= 15 else 1 if top <= 27 else 2 if top <= 51 else 3


def scale_of_words(words):
    """The kernel's form (c3c_fp4_scale): k = 0 exactly where no count has a bit above 15, else from the largest byte."""
    every = 0
    for w in words:
        every |= w
    if every & 0xF0F0F0F0 == 0:
        return 0
    top = max((w >> (8 * b)) & 0xFF for w in words for b in range(4))
    return 1 if top <= 27 else 2 if top <= 51 else 3


def excess_nibble(r, k):
    q = (max(r, 3) - 3 + (1 << k) - 1) >> k
    assert 0 <= q <= 12, (r, k)
    return (E_TABLE >> (4 * q)) & 0xF


def left_bytes(c):
    """The bytes of a count in the two left operand words."""
    return (0x04 if c >= 1 else 0) | (0x40 if c >= 2 else 0), (0x04 if c >= 3 else 0) | (0x40 if c >= 4 else 0)


def right_bytes(r, k):
    """The bytes of a count in the two right operand words."""
    return (0x01 if r >= 1 else 0) | (0x10 if r >= 2 else 0), (0x01 if r >= 3 else 0) | (excess_nibble(r, k) << 4)


def _ge64(word, k):
    """64 [c >= k] per byte (c3c_ge64)."""
    total = word + (0x40 - k) * ONES
    assert total < 1 << 32
    return total & 0x40404040


def perm(s0, s1, sel):
    """v_perm_b32: selector bytes 0 .. 3 pick a byte of s1, 4 .. 7 of s0, 8 .. 11 the sign of byte 1, 3, 5, 7, 12 is 0x00 and
    13 and above 0xff."""
    table = s1 | (s0 << 32)
    out = 0
    for pos in range(4):
        s = (sel >> (8 * pos)) & 0xFF
        if s <= 7:
            byte = (table >> (8 * s)) & 0xFF
        elif s <= 11:
            byte = 0xFF if (table >> (8 * (2 * (s - 8) + 1) + 7)) & 1 else 0x00
        else:
            byte = 0x00 if s == 12 else 0xFF
        out |= byte << (8 * pos)
    return out


def left_words_perm(w):
    """c3c_fp4_left with the byte table (NSM_C3C_FP4_PERM=1)."""
    total = w + 0x3C3C3C3C
    assert total < 1 << 32
    sel = total & 0x43434343
    return perm(0, 0x44440400, sel) & 0x44444444, perm(0, 0x04000000, sel) & 0x44444444


def left_words_plain(w):
    """c3c_fp4_left without it."""
    return (_ge64(w, 1) >> 4) | _ge64(w, 2), (_ge64(w, 3) >> 4) | _ge64(w, 4)


def right_words(w, k):
    """c3c_fp4_right_k0 (byte tables: every count <= 15) and c3c_fp4_right_scaled (byte by byte)."""
    if k == 0:
        assert w & 0xF0F0F0F0 == 0
        sel = w & 0x07070707
        big = ((w >> 3) & ONES) * 0xFF
        lo1 = perm(0x11111111, 0x11110100, sel)
        lo2, hi2 = perm(0x41312111, 0x01000000, sel), perm(0x71717171, 0x61615151, sel)
        return (big & 0x11111111) | (~big & lo1 & 0xFFFFFFFF), (big & hi2) | (~big & lo2 & 0xFFFFFFFF)
    m1 = (_ge64(w, 1) >> 6) | (_ge64(w, 2) >> 2)
    m2 = _ge64(w, 3) >> 6
    for b in range(4):
        m2 |= excess_nibble((w >> (8 * b)) & 0xFF, k) << (8 * b + 4)
    return m1, m2


def _nibbles(byte):
    assert byte & 0x88 == 0  # no sign bit
    return FP4[byte & 0xF], FP4[byte >> 4]


def bucket_parts(a, r, k):
    """What a bucket gives to the first MFMA and, before the block scale, to the second: products of decoded nibbles."""
    (l1, l2), (r1, r2) = left_bytes(a), right_bytes(r, k)
    return sum(x * y for x, y in zip(_nibbles(l1), _nibbles(r1))), sum(x * y for x, y in zip(_nibbles(l2), _nibbles(r2)))


def bucket(a, r, k):
    """D_b as the two MFMAs compute it: the second MFMA's part scaled by 2^k."""
    first, second = bucket_parts(a, r, k)
    return first + second * (1 << k)


def cap3_bucket(a, r):
    """What a bucket gives to the bound of the i8 scan (NSM_C3C_FP4=0, CAP 3)."""
    return min(a, r) if r < 3 else a


def mfma_fp4(a_regs, b_regs, b_scales=None):
    """v_mfma_f32_32x32x64_f8f6f4 on FP4 operands: a_regs[l], b_regs[l] are the four operand words of lane l (row or column
    l & 31, k = 32 (l >> 5) + j in nibble j & 1 of byte j >> 1), b_scales[l] the E8M0 byte of the lane's 32 k of B (None:
    the unscaled form).  Returns the 32 x 32 result, [row][column]."""
    def elem(regs, lane, j):
        return FP4[(regs[lane][j >> 3] >> (4 * (j & 7))) & 0xF]

    out = [[0.0] * 32 for _ in range(32)]
    for row in range(32):
        for col in range(32):
            for half in range(2):
                scale = 1.0 if b_scales is None else 2.0 ** (b_scales[col + 32 * half] - 127)
                out[row][col] += scale * sum(elem(a_regs, row + 32 * half, j) * elem(b_regs, col + 32 * half, j) for j in range(32))
    return out


def c_layout(lane, reg):
    """(row, column) of accumulator register reg of a lane (the 32x32 C/D map)."""
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31
