"""The OR fold of the FP4 scan (csrc/indel_raw_coarse.hpp, NSM_C3C_ORFOLD), restated in plain Python on top of
tests/support/scan_fp4.py.

Tiles 2 p (``hi``) and 2 p + 1 (``lo``) of a wave share one accumulator.  The C operand of the chain's first MFMA is

    BIAS = 2^23 + (256 - need_hi) 2^9 + (256 - need_lo)

and the four MFMAs add 2^9 D_hi + D_lo: the slots 1 and 2 of tile hi through a B scale byte of 0x7f + 9, its slots 3 and 4
through 0x7f + 9 + k_hi, those of tile lo through 0x7f and 0x7f + k_lo.  Every partial sum is an integer in [2^23, 2^24), so
the f32 result's mantissa bits are the integer: field lo = D_lo + 256 - need_lo in bits 0 .. 8, field hi in bits 9 .. 17,
and bit 8 of a field is [D >= need].  The fold is the OR of a lane's 16 registers under the mask FLAG_HI | FLAG_LO.

One bias serves all the tile pairs of a wave, so a lane's need_hi is the SMALLEST need of its even tiles and need_lo that of
its odd tiles (kNever where a column fits no row of the class or does not exist).
"""
import numpy as np

from tests.support import scan_fp4 as fp4

NEVER = 255                    # csrc/nsm_common.hpp: kNever
NT, WAVE = 4, 64               # tiles per wave, lanes
SHIFT = 9                      # the upper field starts here; the B scale of an even tile is 2^SHIFT
FLAG_LO, FLAG_HI = 1 << 8, 1 << (SHIFT + 8)
F32_ONE_ULP = 0x4B000000       # the bits of 2^23: exponent at which one unit in the last place is 1
DRAIN_AT = 2 * WAVE            # kC3cDrainAt
STACK = (NT + 2 + 2) * WAVE    # kC3cStack of the pipelined OR fold: NT x 64 between two checks and one more tile PAIR


def bias(need_hi, need_lo):
    """The integer the bias register holds (as an f32 of the same value)."""
    for need in (need_hi, need_lo):
        assert 0 <= need <= 64 or need == NEVER, need
    return (1 << 23) + ((256 - need_hi) << SHIFT) + (256 - need_lo)


def bias_bits(need_hi, need_lo):
    """The kernel's form: the f32 bit pattern, made with integer instructions."""
    return F32_ONE_ULP | ((256 - need_hi) << SHIFT) | (256 - need_lo)


def scale_bytes(tile, k):
    """The E8M0 B scale bytes of a tile's two MFMAs: (slots 1 and 2, slots 3 and 4)."""
    base = 0x7F + (SHIFT if tile % 2 == 0 else 0)
    return base, base + k


def accumulate(start, terms):
    """f32 accumulation, one rounding per term (numpy arrays or scalars); returns the f32 bit patterns."""
    acc = np.asarray(start, dtype=np.float32)
    for term in terms:
        acc = (acc + np.asarray(term, dtype=np.float32)).astype(np.float32)
    return acc.view(np.uint32) if acc.ndim else np.array([acc], dtype=np.float32).view(np.uint32)[0]


def fields(bits):
    """(field hi, field lo) of f32 bit patterns in [2^23, 2^24)."""
    bits = np.asarray(bits, dtype=np.uint32)
    assert ((bits & 0xFF800000) == F32_ONE_ULP).all()
    n = bits & 0x7FFFFF
    assert (n >> (2 * SHIFT) == 0).all()
    return (n >> SHIFT) & 0x1FF, n & 0x1FF


def flags(bits):
    """(tile hi passes, tile lo passes) as the scan reads them."""
    bits = np.asarray(bits, dtype=np.uint32)
    return (bits & FLAG_HI) != 0, (bits & FLAG_LO) != 0


def fold(lane_bits):
    """The scan's fold of a lane's 16 registers."""
    top = 0
    for b in lane_bits:
        top |= int(b)
    return top & (FLAG_HI | FLAG_LO)


def lane_needs(tile_needs):
    """(need_hi, need_lo) of a lane from the needs of its NT columns (kNever: does not fit, does not exist)."""
    return min(tile_needs[0::2]), min(tile_needs[1::2])


def operand_regs(hists, side, ks=None):
    """The two MFMAs' operand registers of 32 strings (32-bucket histograms): regs[m][lane][4], lane = string + 32 half."""
    regs = [[[0] * 4 for _ in range(64)] for _ in range(2)]
    for lane in range(64):
        s, half = lane & 31, lane >> 5
        for j in range(16):
            c = hists[s][16 * half + j]
            pair = fp4.left_bytes(c) if side == "left" else fp4.right_bytes(c, ks[s])
            for m in range(2):
                regs[m][lane][j >> 2] |= pair[m] << (8 * (j & 3))
    return regs


def chain(left_hists, hi_hists, lo_hists, lane_need):
    """The four MFMAs of a tile pair on the instruction model: bits[lane][reg] of the accumulator.  lane_need[col] =
    (need_hi, need_lo)."""
    a = operand_regs(left_hists, "left")
    bits = None
    acc = np.array([[np.float32(bias(*lane_need[lane & 31]))] * 16 for lane in range(64)], dtype=np.float32)
    assert [int(x) for x in acc[:, 0].view(np.uint32)] == [bias_bits(*lane_need[lane & 31]) for lane in range(64)]
    for tile, hists in ((0, hi_hists), (1, lo_hists)):
        ks = [fp4.scale_of(list(h)) for h in hists]
        b = operand_regs(hists, "right", ks)
        for m in range(2):
            scales = [scale_bytes(tile, ks[lane & 31])[m] for lane in range(64)]
            out = fp4.mfma_fp4(a[m], b[m], scales)
            add = np.array([[out[fp4.c_layout(lane, reg)[0]][lane & 31] for reg in range(16)] for lane in range(64)])
            assert (add == np.floor(add)).all()
            acc = (acc + add.astype(np.float32)).astype(np.float32)
    bits = acc.view(np.uint32)
    return bits


def high_water(blocks, q=0):
    """The wave's stack under the pipelined OR fold: ``blocks`` is a list of NT / 2 push counts (one per tile pair, at most
    128 each).  A run of blocks starts with a check (more than DRAIN_AT waiting: full passes of 64 until fewer than 64 are
    left); the check in front of a block's LAST pair decides on a flush, that pair's entries are still pushed, and the next
    run drains.  Returns (the largest number of entries the stack ever held, entries left)."""
    top, flush = q, True  # (the first block starts a run)
    for pushes in blocks:
        assert len(pushes) == NT // 2 and all(0 <= n <= 2 * WAVE for n in pushes)
        if flush:
            if q > DRAIN_AT:
                q %= WAVE
            flush = False
        for u, n in enumerate(pushes):
            if u == len(pushes) - 1:
                flush = q > DRAIN_AT
            q += n
            top = max(top, q)
    return top, q
