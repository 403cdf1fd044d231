"""The premises of tests/test_gpu_sort_seams.py, checked without a GPU: the reference ordering on hand-written lists, the
case generators of tests/support/sort_seams.py (conditions on the INPUTS: distinct records where ids must decide, ids that
keep the promised limit and reach both of its ends, every seam size on every route that can take it), and a numpy
restatement of the key the header of ``nsm_sort_hits`` defines -- it round-trips and preserves the canonical order for every
id width from 1 to 32 bits over the three score families."""
from pathlib import Path

import numpy as np
import pytest

from support import sort_seams as ss


# ------------------------------------------------------------------------------------------------------- the reference
def _tuples(rec):
    score, i, j = ss.columns(rec)
    return [(float(s).hex(), int(a), int(b)) for s, a, b in zip(score, i, j)]


def test_reference_order_on_hand_written_lists():
    rec = ss.records([0.5, 1.0, 0.5, 0.5, 1.0], [3, 9, 3, 2, -1], [1, 0, 0, 7, 4])
    assert _tuples(ss.reference_order(rec)) == _tuples(ss.records([1.0, 1.0, 0.5, 0.5, 0.5], [-1, 9, 2, 3, 3], [4, 0, 7, 0, 1]))
    # the zeros are different records: +0.0 first, whatever the ids say; the subnormals around them on their sides
    rec = ss.records([-0.0, 0.0, -5e-324, 5e-324, 0.0, -0.0], [0, 5, 0, 0, 4, 0], [0, 5, 0, 0, 9, -1])
    want = ss.records([5e-324, 0.0, 0.0, -0.0, -0.0, -5e-324], [0, 4, 5, 0, 0, 0], [0, 9, 5, -1, 0, 0])
    assert _tuples(ss.reference_order(rec)) == _tuples(want)
    # infinities at the ends, negative scores behind the positive ones, int32 extremes as ids
    rec = ss.records([-np.inf, np.inf, -1.7e308, 1.7e308, -1.0, 1.0, 1.0], [0, 0, 0, 0, 0, ss.INT32_MAX, ss.INT32_MIN], [0] * 7)
    want = ss.records([np.inf, 1.7e308, 1.0, 1.0, -1.0, -1.7e308, -np.inf], [0, 0, ss.INT32_MIN, ss.INT32_MAX, 0, 0, 0], [0] * 7)
    assert _tuples(ss.reference_order(rec)) == _tuples(want)
    assert ss.reference_order(ss.records([], [], [])).shape == (0, 2)


def test_reference_order_agrees_with_a_python_sort():
    rng = np.random.default_rng(3)
    for family in ("few", "adjacent", "extremes"):
        score = ss.scores(family, 500, rng)
        i, j = rng.integers(-4, 4, 500), rng.integers(-4, 4, 500)
        key = lambda t: (-t[0], 0 if t[0] != 0 or np.copysign(1.0, t[0]) > 0 else 1, t[1], t[2])
        want = sorted(zip(score.tolist(), i.tolist(), j.tolist()), key=key)
        got = ss.columns(ss.reference_order(ss.records(score, i, j)))
        assert [(float(s).hex(), a, b) for s, a, b in want] == [(float(s).hex(), int(a), int(b)) for s, a, b in zip(*got)]


def test_multiset_sees_one_changed_bit():
    rng = np.random.default_rng(4)
    rec = ss.records(ss.scores("nan", 300, rng), *ss.ids(0, 300, rng))
    assert np.array_equal(ss.multiset(rec), ss.multiset(rec[rng.permutation(300)]))
    bad = rec.copy()
    bad.view(np.uint64)[17, 0] ^= np.uint64(1)  # a NaN payload bit, or the lowest bit of a score
    assert not np.array_equal(ss.multiset(rec), ss.multiset(bad))
    assert not np.array_equal(ss.multiset(rec), ss.multiset(np.concatenate([rec[:-1], rec[:1]])))


# ----------------------------------------------------------------------------------------------------------- the cases
def test_every_seam_size_runs_on_every_route_that_can_take_it():
    routes = {}
    for c in ss.CASES:
        if c.family == "few" and not c.name.startswith("limit"):
            routes.setdefault(c.n, set()).add((c.route, c.captured, c.n_hint == 0, c.n_hint == c.n, c.n_hint > c.n))
    assert set(ss.SEAM_SIZES) <= set(routes)
    for n in ss.SEAM_SIZES:
        got = {(route, hint0, exact, above) for route, _cap, hint0, exact, above in routes[n]}
        if n < 2:
            assert {r[0] for r in got} >= {"lds_unhinted", "lds_hinted", "lds_then_radix", "captured"}
            continue
        if n <= ss.LDS_MAX:
            assert {("lds_hinted", False, True, False), ("lds_unhinted", True, False, False),
                    ("lds_then_radix", True, False, False)} <= got, n
            caps = {c.capacity for c in ss.CASES if c.n == n and c.route == "lds_unhinted"}
            assert n in caps and (n >= ss.LDS_MAX - 1 or any(x > n and x & (x - 1) for x in caps)), (n, caps)
        else:
            assert {("radix", True, False, False), ("radix", False, True, False), ("radix", False, False, True)} <= got, n
        if n in ss.CAPTURED_SIZES:
            assert {("captured", True, False, False), ("captured", False, True, False), ("captured", False, False, True)} <= got, n
    assert set(ss.CAPTURED_SIZES) == {2048, 2049} | {n for n in ss.SEAM_SIZES if n >= 8191}


def test_the_routes_are_the_ones_the_entry_takes():
    """What the case calls its route follows from the entry's documented routing: geometry from n_hint or the capacity,
    one workgroup up to 8192 records of it, the network only on a capturing stream."""
    for c in ss.CASES:
        assert c.n == min(c.count, c.capacity) and c.capacity <= ss.BIG_CAPACITY + 1000
        assert c.n_hint == 0 or c.n_hint >= c.n, c.name  # the promise holds
        assert c.captured == (c.route == "captured" or c.name.endswith("_captured")), c.name
        if c.route in ("lds_hinted", "lds_unhinted"):
            assert c.bound <= ss.LDS_MAX and not c.scratch and not c.captured, c.name
            assert (c.n_hint != 0) == (c.route == "lds_hinted"), c.name
        if c.route == "lds_then_radix":
            assert c.n <= ss.LDS_MAX < c.bound and c.n_hint == 0 and c.scratch, c.name
        if c.route == "radix":
            assert c.n > ss.LDS_MAX and c.scratch and not c.captured, c.name
        if c.route == "overflow":
            assert c.count == c.capacity + ss.OVERFLOW and c.n_hint == 0 and c.capacity in (ss.LDS_MAX, ss.LDS_MAX + 1), c.name
        else:
            assert c.count == c.n, c.name
        if c.bound > ss.LDS_MAX:
            assert c.scratch, c.name
    overflow = {(c.capacity, c.captured) for c in ss.CASES if c.route == "overflow"}
    assert overflow == {(8192, False), (8192, True), (8193, False), (8193, True)}  # LDS, LDS captured, radix, network


def test_every_family_meets_every_route_on_both_sides_of_the_lds_limit():
    for family in ss.FAMILIES:
        seen = {(c.route, c.n > ss.LDS_MAX) for c in ss.CASES if c.family == family and not c.name.startswith("limit")}
        assert {("lds_hinted", False), ("lds_unhinted", False), ("lds_then_radix", False), ("radix", True), ("captured", False),
                ("captured", True)} <= seen, (family, seen)
        hints = {c.n_hint == 0 for c in ss.CASES if c.family == family and c.route in ("radix", "captured") and c.n > ss.LDS_MAX}
        assert hints == {True, False}


def test_id_limit_cases():
    for n in ss.ID_LIMIT_SIZES:
        got = {c.id_limit: c for c in ss.CASES if c.name.startswith("limit") and c.n == n and not c.name.endswith("_adjacent")}
        assert tuple(sorted(got)) == tuple(sorted(ss.ID_LIMITS))
        assert all(c.route == "radix" and not c.captured for c in got.values())
        tight = {c.id_limit for c in ss.CASES if c.n == n and c.name.endswith("_adjacent")}
        assert tight == set(ss.TIGHT_LIMITS)
    assert [ss.id_bits(v) for v in ss.ID_LIMITS] == [32, 1, 1, 2, 2, 3, 15, 15, 16, 16, 21, 31, 31, 32, 32]


@pytest.mark.parametrize("name", ss.NAMES)
def test_case_inputs(name):
    c = ss.BY_NAME[name]
    rec = ss.buffer(c)
    assert rec.shape == (c.capacity, 2) and np.array_equal(ss.buffer(c).view(np.uint64), rec.view(np.uint64))  # (deterministic)
    score, i, j = ss.columns(rec[: c.n])
    # the promise holds and both of its ends occur in both columns
    if c.id_limit == 0:
        lo, hi = ss.INT32_MIN, ss.INT32_MAX
    else:
        lo, hi = 0, min(c.id_limit, 1 << 31) - 1
    if c.n:
        assert lo <= int(i.min()) and int(i.max()) <= hi and lo <= int(j.min()) and int(j.max()) <= hi
    if c.n >= 2:
        assert {lo, hi} <= set(i.tolist()) and {lo, hi} <= set(j.tolist()), name
    if c.id_limit == 1 and c.n:
        assert not i.any() and not j.any()
    # the records are distinct: where scores tie the ids decide, and no two records tie in all three
    w = ss.words(rec[: c.n])
    assert len(np.unique(w, axis=0)) == c.n, f"{name}: {c.n - len(np.unique(w, axis=0))} repeated records"
    if c.family == "adjacent":
        assert len(np.unique(score.view(np.uint64))) == c.n and not np.isnan(score).any()
        gaps = np.diff(np.sort(ss.ascending_bits(score)))
        assert c.n < 10 or np.median(gaps) == 1  # neighbours in value are neighbours in the key's lowest bit
    if c.family == "few" and c.n > 100:
        assert len(np.unique(score)) <= 7  # ids decide most neighbours
    if c.family == "extremes" and c.n >= len(ss.EXTREMES):
        assert {float(v).hex() for v in ss.EXTREMES} == {float(v).hex() for v in score}
    assert np.isnan(score).any() == (c.family == "nan" and c.n > 0)
    if c.family == "nan":
        assert len({int(b) for b in score[np.isnan(score)].view(np.uint64)}) == len(ss.NAN_BITS) and not c.ordered
    # the filler behind the live records is nothing the sort could have produced from them
    assert (rec.view(np.uint8).reshape(-1)[c.n * 16:] != 0).all()
    # check() accepts the reference's answer and nothing that differs from it in one record
    if c.n >= 2:
        done = rec.copy()
        done[: c.n] = ss.reference_order(rec[: c.n])
        ss.check(c, rec, done)
        bad = done.copy()
        bad[[0, c.n - 1]] = bad[[c.n - 1, 0]]
        if c.ordered:
            with pytest.raises(AssertionError):
                ss.check(c, rec, bad)
        else:
            ss.check(c, rec, bad)
            bad.view(np.int32).reshape(-1, 4)[c.n // 2, 3] ^= 1
            with pytest.raises(AssertionError):
                ss.check(c, rec, bad)
        if c.bound < c.capacity:
            bad = done.copy()
            bad.view(np.uint8).reshape(-1)[c.bound * 16] ^= 1
            with pytest.raises(AssertionError):
                ss.check(c, rec, bad)


# ------------------------------------------------------------------------------------------------------- the key codec
@pytest.mark.parametrize("bits", range(1, 33))
def test_key_codec_round_trips_and_keeps_the_order(bits):
    """The header's key for every id width: the smallest and the largest id_limit that give ``bits`` bits, and for 32 bits
    "no promise" (any int32, sign bit flipped)."""
    if bits == 32:
        limits = (0, (1 << 31) + 1, (1 << 32) - 1)
    else:
        limits = tuple(sorted({max(1, (1 << (bits - 1)) + 1) if bits > 1 else 1, 1 << bits}))
    for limit in limits:
        assert ss.id_bits(limit) == bits, (limit, bits)
        for family in ("few", "adjacent", "extremes"):
            rng = np.random.default_rng(bits * 10 + len(family))
            n = 600
            i, j = ss.ids(limit, n, rng)
            rec = ss.records(ss.scores(family, n, rng), i, j)
            keys = ss.pack(*ss.columns(rec), limit)
            assert max(keys) < 1 << (64 + 2 * bits)
            assert np.array_equal(ss.words(ss.unpack(keys, limit)), ss.words(rec)), (limit, family)
            order = sorted(range(n), key=keys.__getitem__)
            assert np.array_equal(ss.words(rec[order]), ss.words(ss.reference_order(rec))), (limit, family)
            # equal keys are equal records
            assert len(set(keys)) == len(np.unique(ss.words(rec), axis=0))
    if bits < 32:  # one more would not fit: the promise is what makes the narrow key valid
        with pytest.raises(AssertionError):
            ss.pack([0.5], [1 << bits], [0], 1 << bits)


def test_key_codec_is_the_headers():
    """K, A and the fields as include/nsm_hip.h writes them, on values worked out by hand."""
    assert ss.score_key([np.inf, 1.0, 0.0, -0.0, -np.inf]).tolist() == [
        0x000FFFFFFFFFFFFF, 0x400FFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0xFFF0000000000000]
    assert ss.pack([1.0], [5], [3], 8) == [(0x400FFFFFFFFFFFFF << 6) | (5 << 3) | 3]
    assert ss.pack([1.0], [-1], [0], 0) == [(0x400FFFFFFFFFFFFF << 64) | (0x7FFFFFFF << 32) | 0x80000000]
    header = (Path(__file__).resolve().parent.parent / "include" / "nsm_hip.h").read_text()
    for phrase in ("K(score) : I(i) : I(j)", "+0.0 sorts before -0.0", "NaN scores are", "ceil(log2(id_limit))"):
        assert phrase in header, phrase


# --------------------------------------------------------------------------------------------------------- relabelings
def test_relabelings():
    maps = ss.relabelings()
    assert tuple(maps) == ss.RELABELINGS and maps["identity"] == (None, None)
    for name, (lo, ro) in maps.items():
        for arr, n in ((lo, ss.N_LEFT), (ro, ss.N_RIGHT)):
            if arr is not None:
                assert arr.dtype == np.int32 and arr.shape == (n,) and (np.diff(arr.astype(np.int64)) > 0).all(), name
    assert int(maps["max_2p14m1_left"][0].max()) == (1 << 14) - 1 and int(maps["max_2p14_left"][0].max()) == 1 << 14
    assert int(maps["max_2p14m1_right"][1].max()) == (1 << 14) - 1 and int(maps["max_2p14_right"][1].max()) == 1 << 14
    assert int(maps["far_left"][0].min()) == 1_000_003 and int(maps["far_right"][1].max()) == 1_000_003 + 7 * (ss.N_RIGHT - 1)
    assert int(maps["negative_left"][0].min()) < 0 <= int(maps["negative_left"][0][1])
    assert int(maps["negative_right"][1].min()) < 0
    assert ss.N_LEFT * ss.N_RIGHT > ss.LDS_MAX and ss.N_LEFT * min(ss.TOP_K, ss.N_RIGHT) > ss.LDS_MAX
    # relabelled(): ids mapped, then the canonical order again
    score, i, j = ss.relabelled([0.5, 0.5, 1.0], [0, 1, 2], [2, 0, 1], maps["far_left"][0], None)
    assert score.tolist() == [1.0, 0.5, 0.5] and i.tolist() == [1_000_017, 1_000_003, 1_000_010] and j.tolist() == [1, 2, 0]


def test_wrapper_items():
    it = ss.wrapper_items()
    assert len(it["left_sets"]) == len(it["left_strings"]) == ss.N_LEFT and len(it["right_sets"]) == ss.N_RIGHT
    for row in it["left_sets"] + it["right_sets"]:
        assert 1 <= len(row) <= 8 and len(set(row)) == len(row)
    for s in it["left_strings"] + it["right_strings"]:
        assert 2 <= len(s) <= 20 and s == s.lower().strip()
    for levels in it["left_set_levels"] + it["right_set_levels"]:
        assert len(levels) == 2 and levels[1][: len(levels[0])] == levels[0] and levels[0]
