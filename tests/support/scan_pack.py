"""The packed left rows of the FP4 scan (csrc/indel_raw_coarse.hpp: c3c_pack_left_kernel and the PACKED scan), restated in
plain Python.

The pre-pass codes every left row once per call.  A row's 32-bucket histogram is eight 32-bit words (four counts each,
bucket 4 q + byte in word q); lane half h of the scan owns words 4 h .. 4 h + 3.  A packed row is 64 bytes,

    [half 0: m1 words 16 B | m2 words 16 B][half 1: m1 words 16 B | m2 words 16 B]

with (m1, m2) = c3c_fp4_left of a histogram word: the operand words of the first and of the second MFMA.  Rows are in
table order, so lane (col, half) of the block at row i reads the 32 contiguous bytes at (i + col) * 64 + half * 32, clamped
to the last row of the length class inside the chunk.
"""
from tests.support import scan_fp4 as fp4

ROW_BYTES = 64
HALF_BYTES = 32
BLOCK = 32


def hist_words(counts):
    """The eight histogram words of 32 bucket counts."""
    assert len(counts) == 32 and all(0 <= c <= 255 for c in counts)
    return [sum(counts[4 * q + b] << (8 * b) for b in range(4)) for q in range(8)]


def pack_half(words4):
    """The eight words of one (row, half): the m1 group first, then the m2 group."""
    coded = [fp4.left_words_perm(w) for w in words4]
    return [m1 for m1, _ in coded] + [m2 for _, m2 in coded]


def pack_row(words8):
    """The sixteen words of a packed row."""
    return pack_half(words8[:4]) + pack_half(words8[4:])


def pack_table(rows):
    """The packed rows of a table of count vectors, as one flat list of 32-bit words (16 a row, table order)."""
    out = []
    for counts in rows:
        out += pack_row(hist_words(counts))
    return out


def words_bytes(words):
    return b"".join(w.to_bytes(4, "little") for w in words)


def lane_offset(i, i0, b, col, half):
    """Byte offset, from the chunk's first packed row (table row i0), of what lane (col, half) loads for the block at table
    row i of a length class that ends (in this chunk) before row b."""
    return min((i - i0) * ROW_BYTES + col * ROW_BYTES + half * HALF_BYTES, (b - 1 - i0) * ROW_BYTES + half * HALF_BYTES)


def lane_words(packed, i, i0, b, lane):
    """(m1 words, m2 words) of a lane of the block at row i, read from the flat word list of the WHOLE table."""
    off = i0 * ROW_BYTES + lane_offset(i, i0, b, lane & 31, lane >> 5)
    assert off % 16 == 0 and 0 <= off and off + HALF_BYTES <= 4 * len(packed)
    w = off // 4
    return packed[w:w + 4], packed[w + 4:w + 8]
