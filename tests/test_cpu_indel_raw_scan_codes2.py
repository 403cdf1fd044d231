"""The value-table codes of the packed FP4 scan (csrc/indel_raw_coarse.hpp, NSM_C3C_CODES2) on the CPU, through the
restatement in tests/support/scan_codes2.py: the bound for every count and scale, the kernel's word forms against per-byte
loops, the 11-bit fields of the OR fold on the instruction model, and the pass counts on a seeded sample."""
import importlib.util
import os

import numpy as np
import pytest

from tests.support import scan_codes2 as c2
from tests.support import scan_fp4 as fp4
from tests.support import scan_items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("c3_code_search", os.path.join(ROOT, "tools", "c3_code_search.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tables_are_the_tools(tool):
    assert {"x3": c2.X3, "x4": c2.X4, "y3": c2.Y3, "y4": c2.Y4} == tool.SHIPPED
    words = tool.byte_tables(tool.SHIPPED)
    assert tuple(words["left"]) == c2.LEFT_WORDS and tuple(words["right"]) == c2.RIGHT_WORDS
    assert tool.is_monotone(tool.SHIPPED) and tool.check_bound(tool.SHIPPED)
    for name in (c2.X3, c2.X4, c2.Y3, c2.Y4):
        assert all(0 <= code <= 7 for code in name)  # no sign bit


def test_bound_for_every_count_and_scale():
    """x3 y3 2^k + x4 y4 2^k >= max(min(a, r) - 2, 0) and D_b >= min(a, r) for every a, r in 0 .. 64 and every k that a string
    holding r can carry (its k comes from its largest count: every k from scale_of([r]) up)."""
    for k in range(4):
        for r in range(65):
            if fp4.scale_of([r]) > k:
                continue
            for a in range(65):
                assert (1 << k) * c2.slots34(a, r, k) >= max(min(a, r) - 2, 0), (a, r, k)
                assert c2.bucket(a, r, k) >= min(a, r), (a, r, k)
                assert (4 * c2.bucket(a, r, k)) % 1 == 0


def test_small_counts_are_exact():
    """Where both counts are 3 or less the bound is the minimum itself."""
    for a in range(4):
        for r in range(4):
            assert c2.bucket(a, r, 0) == min(a, r)


@pytest.mark.parametrize("others", [0, 1, 15, 64])
def test_left_words_every_count_every_byte(others):
    for c in range(65):
        for pos in range(4):
            w = (others * c2.ONES) & ~(0xFF << (8 * pos)) | (c << (8 * pos))
            m1, m2 = c2.left_words(w)
            for b in range(4):
                cb = (w >> (8 * b)) & 0xFF
                assert ((m1 >> (8 * b)) & 0xFF, (m2 >> (8 * b)) & 0xFF) == c2.left_bytes(cb), (c, pos, b)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_right_words_every_count_every_byte(k):
    top = (15, 27, 51, 64)[k]
    for others in (0, 2, 3, top):
        for c in range(top + 1):
            for pos in range(4):
                w = (others * c2.ONES) & ~(0xFF << (8 * pos)) | (c << (8 * pos))
                m1, m2 = c2.right_words(w, k)
                for b in range(4):
                    cb = (w >> (8 * b)) & 0xFF
                    assert ((m1 >> (8 * b)) & 0xFF, (m2 >> (8 * b)) & 0xFF) == c2.right_bytes(cb, k), (c, pos, b)


def test_no_bound_carries(tool):
    """The largest D over all pairs of histograms of at most 64 units each, by scale: below 256 + need for every need >= 0
    (a field 4 D + 1024 - 4 need stays below 2048) and, with need = kNever, 4 D + 4 below 1024: never flagged."""
    tops = tool.max_bound(tool.SHIPPED)
    assert max(tops) <= 254 and tops == [76.0, 106.0, 140.0, 162.0]
    assert 4 * max(tops) + 1024 < 2048 and 4 * max(tops) + 4 < 1024
    # the whole sum stays in [2^23, 2^24)
    assert c2.bias(0, 0) + (int(4 * max(tops)) << c2.FIELD_BITS) + int(4 * max(tops)) < 1 << 24
    assert c2.bias(c2.NEVER, c2.NEVER) >= 1 << 23


def _hists(rows):
    return [list(r) + [0] * (32 - len(r)) for r in rows]


def test_fields_on_the_instruction_model():
    """A tile pair through scan_fp4's MFMA model with the scale bytes of the 11-bit fields: every partial sum exact (asserted
    in chain), the fields 4 D + 1024 - 4 need, the flags [D >= need].  Rows and columns: small counts, quarter products
    (a = 6 against r = 4: 1 + 1.5), large bounds of k = 0 and k = 3, a scaled string beside an unscaled one."""
    big3 = [52, 4, 4, 4]                        # k = 3
    full0 = [15, 15, 15, 15, 4]                 # k = 0, 64 units
    rows = [[6, 6, 6, 5, 4, 3, 2, 1], [4] * 16, full0, big3, [64], [3] * 21, [7, 7, 7, 7], [11, 12, 13, 14]]
    cols_hi = [[4, 4, 4, 4, 4, 3, 2, 1], [5] * 12, full0, big3, [64], [3] * 21, [28, 28, 8], [10, 9, 8, 7]]
    cols_lo = [[16, 16, 16, 16], [6, 4, 6, 4], big3, full0, [2] * 32, [0] * 32, [5, 6, 7, 8], [13, 13, 13, 13]]
    left = _hists(rows + [[1]] * 24)
    hi = _hists(cols_hi + [[0]] * 24)
    lo = _hists(cols_lo + [[0]] * 24)
    needs = [(n % 65, (3 * n + 7) % 65) for n in range(32)]
    needs[3], needs[5] = (c2.NEVER, 0), (0, c2.NEVER)
    bits = c2.chain(left, hi, lo, needs)
    seen_quarter = False
    for lane in range(64):
        col = lane & 31
        for reg in range(16):
            row = fp4.c_layout(lane, reg)[0]
            d_hi, d_lo = c2.bound(left[row], hi[col]), c2.bound(left[row], lo[col])
            f_hi, f_lo = c2.fields(int(bits[lane][reg]))
            assert f_hi == 4 * d_hi + 1024 - 4 * needs[col][0] and f_lo == 4 * d_lo + 1024 - 4 * needs[col][1]
            assert bool(bits[lane][reg] & c2.FLAG_HI) == (d_hi >= needs[col][0])
            assert bool(bits[lane][reg] & c2.FLAG_LO) == (d_lo >= needs[col][1])
            seen_quarter = seen_quarter or d_hi % 1 != 0 or d_lo % 1 != 0
    assert seen_quarter
    assert c2.bound(left[2], hi[3]) == 152  # (the largest bound there is: 162, test_no_bound_carries)


# --- the seeded sample ----------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def sample():
    from napkon_string_matching_amd import synthetic

    def hist(seed):
        codes, length = synthetic.strings(4000, seed)
        return np.stack([np.bincount(codes[i, : length[i]] & 31, minlength=32) for i in range(4000)]), length.astype(np.int64)

    (lh, ll), (rh, rl) = hist(1234), hist(5678)
    top = int(max(lh.max(), rh.max()))
    assert top <= 15  # every right string has k = 0
    lcsmin, _ = scan_items.lcsmin_of(0.8)
    need = np.array(lcsmin)[ll[:, None] + rl[None, :]]
    fits = np.minimum(ll[:, None], rl[None, :]) >= need

    def d_of(bucket):
        table = np.array([[bucket(a, r, 0) for r in range(top + 1)] for a in range(top + 1)], dtype=np.float32)
        d = np.zeros((4000, 4000), dtype=np.float32)
        for a in range(1, top + 1):
            d += (lh == a).astype(np.float32) @ table[a][rh].T
        return d

    return {"need": need, "fits": fits, "new": d_of(c2.bucket), "old": d_of(fp4.bucket), "min": d_of(lambda a, r, k: min(a, r))}


def test_sample_drops_no_pair(sample):
    s = sample
    assert int(s["fits"].sum()) == 8585239
    assert (s["new"] >= s["min"]).all() and (s["old"] >= s["min"]).all()
    assert not ((s["min"] >= s["need"]) & s["fits"] & (s["new"] < s["need"])).any()


def test_sample_passes_at_most_045_of_the_present_code(sample):
    s = sample
    old = int(((s["old"] >= s["need"]) & s["fits"]).sum())
    new = int(((s["new"] >= s["need"]) & s["fits"]).sum())
    print(f"present code {old} pairs, new code {new} pairs, {new / old:.3f}")
    assert old == 1448  # 1.69e-4 of the pairs that pass the length filter
    assert new <= 0.45 * old
