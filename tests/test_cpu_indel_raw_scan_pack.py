"""The packed left rows of the FP4 scan (csrc/indel_raw_coarse.hpp: c3c_pack_left_kernel, indel_raw_coarse_kernel<.., true>),
checked without a GPU on their Python restatement (tests/support/scan_pack.py): the bytes of a packed (row, half), what a
block's packed words give on the matrix pipe, and the clamped offset a lane loads from."""
import random

import pytest

from tests.support import scan_fp4 as fp4
from tests.support import scan_pack as pk


@pytest.mark.parametrize("half", [0, 1])
def test_every_count_in_every_byte_position(half):
    """A count of 0 .. 64 in each of the 16 byte positions of a half, among counts that stay: the 32 bytes of (row, half) are
    c3c_fp4_left of the half's four words, the m1 group first; byte by byte they are the codes of the counts."""
    rng = random.Random(40 + half)
    for pos in range(16):
        for c in range(65):
            counts = [rng.randint(0, 6) for _ in range(32)]
            counts[16 * half + pos] = c
            words = pk.hist_words(counts)
            packed = pk.pack_row(words)
            mine = packed[8 * half:8 * half + 8]
            want = [fp4.left_words_perm(w) for w in words[4 * half:4 * half + 4]]
            assert mine[:4] == [m1 for m1, _ in want] and mine[4:] == [m2 for _, m2 in want]
            raw = pk.words_bytes(mine)
            assert len(raw) == pk.HALF_BYTES
            for u in range(16):
                b1, b2 = fp4.left_bytes(counts[16 * half + u])
                assert (raw[u], raw[16 + u]) == (b1, b2), (pos, c, u)
    # the other half's bytes are the other half's counts: the two halves of a row do not overlap
    counts = [0] * 32
    counts[16 * half] = 4
    row = pk.words_bytes(pk.pack_row(pk.hist_words(counts)))
    assert len(row) == pk.ROW_BYTES and row[32 * half] == 0x44 and row[32 * half + 16] == 0x44
    assert sum(row) == 2 * 0x44


def test_a_block_of_packed_words_on_the_matrix_pipe():
    """32 left rows (every count value among them, one row short of the class's end so that the clamp repeats a row) against
    32 right strings with scales 0 .. 3: the packed words of the block's lanes through the two MFMAs give, register by
    register of the C layout, the sum over the 32 buckets of scan_fp4.bucket."""
    rng = random.Random(7)
    pool = list(range(17)) + [27, 28, 51, 52, 61, 64]
    lrows = [[rng.choice(pool[:8]) for _ in range(32)] for _ in range(70)]
    for u, c in enumerate(pool):
        lrows[33 + u % 31][(5 * u) % 32] = c
    rrows = [[rng.choice(pool[:12]) for _ in range(32)] for _ in range(32)]
    rrows[3][9], rrows[11][30], rrows[20][0] = 20, 40, 64
    ks = [fp4.scale_of(r) for r in rrows]
    assert set(ks) == {0, 1, 2, 3}
    packed = pk.pack_table(lrows)
    i0, i, b = 32, 33, 64  # the chunk starts at table row 32; the block at row 33 of a class that ends before row 64
    a1, a2, b1, b2, scales = [], [], [], [], []
    for lane in range(64):
        m1, m2 = pk.lane_words(packed, i, i0, b, lane)
        a1.append(m1)
        a2.append(m2)
        rw = pk.hist_words(rrows[lane & 31])[4 * (lane >> 5):4 * (lane >> 5) + 4]
        coded = [fp4.right_words(w, ks[lane & 31]) for w in rw]
        b1.append([x for x, _ in coded])
        b2.append([y for _, y in coded])
        scales.append(127 + ks[lane & 31])
    first, second = fp4.mfma_fp4(a1, b1), fp4.mfma_fp4(a2, b2, scales)
    for lane in range(64):
        for reg in range(16):
            r, col = fp4.c_layout(lane, reg)
            row = min(i + r, b - 1)  # (the block's row 31 does not exist: the class's last row again)
            want = sum(fp4.bucket(x, y, ks[col]) for x, y in zip(lrows[row], rrows[col]))
            assert first[r][col] + second[r][col] == want, (lane, reg)


@pytest.mark.parametrize("n_class", [1, 31, 32, 33, 65])
def test_the_clamped_offset_stays_inside_the_table(n_class):
    """Classes of 1, 31, 32, 33 and 65 rows at every position in a table cut into chunks of 64 rows: every lane of every
    block reads 32 bytes inside [0, n_left * 64), of a row of its own class and chunk -- the row it stands for, or the
    class's last row in the chunk past its end -- and of its own half."""
    chunk_rows = 64
    for first in (0, 1, 31, 63, 64, 100):
        n_left = first + n_class  # (the class is the table's last: its last row is the table's)
        for i0 in range(0, n_left, chunk_rows):
            a, b = max(i0, first), min(i0 + chunk_rows, n_left)
            for i in range(a, b, pk.BLOCK):
                for lane in range(64):
                    col, half = lane & 31, lane >> 5
                    off = i0 * pk.ROW_BYTES + pk.lane_offset(i, i0, b, col, half)
                    assert 0 <= off and off + pk.HALF_BYTES <= n_left * pk.ROW_BYTES
                    assert off // pk.ROW_BYTES == min(i + col, b - 1) and off % pk.ROW_BYTES == half * pk.HALF_BYTES
                    assert pk.lane_offset(i, i0, b, col, half) < (1 << 15) * pk.ROW_BYTES < 1 << 32
