"""Cases and references for ``nsm_sort_hits`` (csrc/hits_sort.hip) at the seams of its three code paths, and for the
``id_limit`` the Python wrappers promise it (tests/test_gpu_sort_seams.py runs them, tests/test_cpu_sort_seams.py checks
this file without a GPU).  Nothing here imports torch or the library at module level.

A record is 16 bytes: the double ``score``, then the int32 ``i`` and ``j``; a list is a ``[n, 2]`` float64 array whose second
column holds the two ids.  The canonical order is the one the header states: ascending in the integer key
K(score) : I(i) : I(j), i.e. score descending BY ITS BITS (+0.0 before -0.0), then i, then j ascending as int32 values.
``reference_order`` is that order with numpy's lexsort; results are compared as ``uint64`` views, byte for byte.

A ``Case`` names one call: how many records are live, what the counter says, the buffer's capacity, the two promises, whether
the stream is capturing, and which records go in.  ``expectation`` states what the header defines for it:

  * records [0, live) in canonical order (NaN families: the same multiset, nothing more);
  * records [live, bound) unspecified, bound = n_hint if 0 < n_hint < capacity else capacity;
  * records [bound, capacity) byte-identical.
"""
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

LDS_MAX = 8192        # records one workgroup orders in LDS
TILE = 2048           # records of one LDS tile of the captured network
BIG_CAPACITY = 20000  # "capacity far above the live count": the benchmark's call shape, and the LDS-then-radix route
SEAM_SIZES = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 10239, 10240,
              10241, 12287, 12288, 12289, 16383, 16384, 16385)
CAPTURED_SIZES = (2048, 2049) + tuple(n for n in SEAM_SIZES if n >= 8191)
FAMILY_SIZES = (4097, 12289)  # one on each side of LDS_MAX, neither a power of two nor a multiple of the tile
ID_LIMIT_SIZES = (8193, 12289)
ID_LIMITS = (0, 1, 2, 3, 4, 5, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, 1 << 16, (1 << 20) + 1, (1 << 31) - 1, 1 << 31,
             (1 << 31) + 1, (1 << 32) - 1)
TIGHT_LIMITS = ((1 << 15) - 1, 1 << 15, (1 << 15) + 1)
OVERFLOW = 37
ROUTES = ("lds_hinted", "lds_unhinted", "lds_then_radix", "radix", "captured", "overflow")
FAMILIES = ("few", "adjacent", "extremes", "nan")
EXTREMES = (0.0, -0.0, 5e-324, -5e-324, 1.7e308, -1.7e308, np.inf, -np.inf, 1.0, -1.0, 0.5, -0.5, 2.5, -3.75, 1e-300, -1e-300)
NAN_BITS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
            0xFFFFFFFFFFFFFFFF, 0x7FF8000000000123)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


# ------------------------------------------------------------------------------------------------------------- records
def records(score, i, j) -> np.ndarray:
    score = np.asarray(score, dtype=np.float64)
    rec = np.zeros((len(score), 2), dtype=np.float64)
    rec[:, 0] = score
    ij = rec.view(np.int32).reshape(-1, 4)
    ij[:, 2], ij[:, 3] = np.asarray(i, dtype=np.int32), np.asarray(j, dtype=np.int32)
    return rec


def columns(rec: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    rec = np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 2)
    ij = rec.view(np.int32).reshape(-1, 4)
    return rec[:, 0].copy(), ij[:, 2].copy(), ij[:, 3].copy()


def words(rec: np.ndarray) -> np.ndarray:
    """The records as ``[n, 2]`` uint64: what "byte-exact" compares."""
    return np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 2).view(np.uint64)


def ascending_bits(score) -> np.ndarray:
    """A of the header: an integer image of the doubles that ascends with the score."""
    b = np.ascontiguousarray(score, dtype=np.float64).view(np.uint64)
    flip = np.where(b >> np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1) << np.uint64(63))
    return b ^ flip


def reference_order(rec: np.ndarray) -> np.ndarray:
    """The records in canonical order: score descending by its bits, then i, then j ascending."""
    score, i, j = columns(rec)
    order = np.lexsort((j, i, ~ascending_bits(score)))
    return np.ascontiguousarray(rec, dtype=np.float64).reshape(-1, 2)[order]


def multiset(rec: np.ndarray) -> np.ndarray:
    """The records in an order that depends on their bytes alone (for lists whose canonical order is out of contract)."""
    w = words(rec)
    return w[np.lexsort((w[:, 1], w[:, 0]))]


# --------------------------------------------------------------------------------------------------------------- scores
def _from_bits(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def adjacent_scores(n: int, rng) -> np.ndarray:
    """n DISTINCT doubles in ``np.nextafter`` chains around 0.5, 1.0 and 0.0 (below 0.0: the negative subnormals), shuffled:
    neighbours differ in the lowest bits of the score key only."""
    m = -(-n // 3)
    half = m // 2 + 1
    steps = np.arange(-half, half + 1, dtype=np.int64)
    out = []
    for centre in (0.5, 1.0):
        base = int(np.float64(centre).view(np.uint64))
        out.append(_from_bits((base + steps).astype(np.uint64)))
    mag = np.abs(steps).astype(np.uint64)  # around zero: k ulps up are the bits k, k ulps down the bits k with the sign
    out.append(_from_bits(np.where(steps < 0, mag | (np.uint64(1) << np.uint64(63)), mag)))
    pool = np.concatenate(out)
    assert len(np.unique(pool.view(np.uint64))) == len(pool) >= n
    return rng.permutation(pool)[:n]


def scores(family: str, n: int, rng) -> np.ndarray:
    if family == "few":
        return rng.integers(0, 7, n).astype(np.float64) / 6.0
    if family == "adjacent":
        return adjacent_scores(n, rng)
    if family == "extremes":
        s = np.asarray(EXTREMES, dtype=np.float64)[rng.integers(0, len(EXTREMES), n)]
        s[: min(n, len(EXTREMES))] = EXTREMES[: min(n, len(EXTREMES))]  # every value occurs
        return s
    if family == "nan":
        s = np.asarray(EXTREMES, dtype=np.float64)[rng.integers(0, len(EXTREMES), n)]
        nans = _from_bits(np.asarray(NAN_BITS, dtype=np.uint64))
        at = rng.random(n) < 0.3
        s[at] = nans[rng.integers(0, len(nans), int(at.sum()))]
        s[: min(n, len(nans))] = nans[: min(n, len(nans))]
        return s
    raise ValueError(family)


# ------------------------------------------------------------------------------------------------------------------ ids
def id_bits(id_limit: int) -> int:
    """Bits per id in the sort key: 32 (sign bit flipped) for 0 = unknown and beyond 2^31, else max(1, ceil(log2))."""
    if id_limit <= 0 or id_limit > (1 << 31):
        return 32
    return max(1, int(id_limit - 1).bit_length())


def ids(id_limit: int, n: int, rng) -> Tuple[np.ndarray, np.ndarray]:
    """(i, j) that keep the promise ``id_limit`` and reach both of its ends in both columns: 0 and id_limit - 1 (beyond
    2^31: up to 2^31 - 1; no promise: any int32, both extremes in both columns).  The pairs are distinct whenever the
    range holds n pairs: every record draws from a stripe of the pair space that is its own."""
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    perm = rng.permutation(n).astype(np.int64)
    if id_limit == 0:
        i = rng.integers(INT32_MIN, INT32_MAX + 1, n, dtype=np.int64)
        for k, v in enumerate((INT32_MIN, INT32_MAX, 0, -1)[:n]):
            i[k] = v
        j = perm * ((1 << 32) // n) + INT32_MIN  # (distinct, so the pairs are)
        j[perm == n - 1] = INT32_MAX
        return i.astype(np.int32), j.astype(np.int32)
    top = min(id_limit, 1 << 31)
    space = top * top
    if space >= n:
        stripe = space // n
        flat = perm * stripe + rng.integers(0, stripe, n, dtype=np.int64)
        flat[perm == 0] = 0
        flat[perm == n - 1] = space - 1
        i, j = flat // top, flat % top
    else:  # fewer pairs than records: such cases carry distinct scores
        i, j = rng.integers(0, top, n, dtype=np.int64), rng.integers(0, top, n, dtype=np.int64)
        i[0] = j[0] = 0
        i[1] = j[1] = top - 1
    return i.astype(np.int32), j.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    route: str
    n: int             # records that go in as live ones (min(count, capacity))
    count: int         # what *hit_count says
    capacity: int
    n_hint: int
    id_limit: int
    family: str = "few"
    captured: bool = False
    scratch: bool = True  # False: scratch = NULL (at most LDS_MAX records can be live)

    @property
    def bound(self) -> int:
        return self.n_hint if 0 < self.n_hint < self.capacity else self.capacity

    @property
    def ordered(self) -> bool:
        return self.family != "nan"


def _cap_above(n: int) -> Optional[int]:
    """A capacity above n that is no power of two and still within one workgroup's reach, or None."""
    c = n + n // 3 + 3
    if c > LDS_MAX:
        c = LDS_MAX - 2 if n < LDS_MAX - 2 else None
    if c is not None and c & (c - 1) == 0:
        c += 1
    return c


def _hints(n: int) -> List[Tuple[str, int, int]]:
    """(tag, n_hint, capacity) of the three promises: exact, generous, none (the benchmark's)."""
    return [("hint_n", n, n + 300), ("hint_n1000", n + 1000, n + 2000), ("hint_0", 0, BIG_CAPACITY)]


def _build() -> List[Case]:
    out: List[Case] = []
    add = lambda name, route, n, cap, hint, limit, **kw: out.append(
        Case(name, route, n, kw.pop("count", n), cap, hint, limit, **kw))
    # the two sizes no route has to order
    for n in (0, 1):
        add(f"n{n}_exact_capacity", "lds_unhinted", n, n, 0, 0, scratch=False)
        add(f"n{n}_lds", "lds_unhinted", n, 300, 0, 0, scratch=False)
        add(f"n{n}_hinted", "lds_hinted", n, 300, max(n, 1), 0, scratch=False)
        add(f"n{n}_radix", "lds_then_radix", n, BIG_CAPACITY, 0, 1000)
        add(f"n{n}_captured", "captured", n, BIG_CAPACITY, 0, 1000, captured=True)
    for n in SEAM_SIZES:
        if n < 2:
            continue
        if n <= LDS_MAX:
            add(f"n{n}_lds_hinted", "lds_hinted", n, n + 300, n, 1000, scratch=False)
            add(f"n{n}_lds_cap_n", "lds_unhinted", n, n, 0, 1000, scratch=False)
            if _cap_above(n):
                add(f"n{n}_lds_cap_{_cap_above(n)}", "lds_unhinted", n, _cap_above(n), 0, 1000, scratch=False)
            add(f"n{n}_lds_then_radix", "lds_then_radix", n, BIG_CAPACITY, 0, 1000)
        else:
            for tag, hint, cap in _hints(n):
                for limit in (0, 1000):
                    add(f"n{n}_radix_{tag}_limit{limit}", "radix", n, cap, hint, limit)
        if n in CAPTURED_SIZES:
            for tag, hint, cap in _hints(n):
                add(f"n{n}_captured_{tag}", "captured", n, cap, hint, 1000, captured=True)
    # a counter that ran past the capacity: every record of the buffer is live
    for cap in (LDS_MAX, LDS_MAX + 1):
        add(f"overflow_cap{cap}_eager", "overflow", cap, cap, 0, 1000, count=cap + OVERFLOW)
        add(f"overflow_cap{cap}_captured", "overflow", cap, cap, 0, 1000, count=cap + OVERFLOW, captured=True)
    # the score families on every route, at a size on each side of LDS_MAX
    for family in FAMILIES:
        small, large = FAMILY_SIZES
        kw = dict(family=family)
        add(f"{family}_n{small}_lds_hinted", "lds_hinted", small, small + 300, small, 1000, scratch=False, **kw)
        add(f"{family}_n{small}_lds_cap_n", "lds_unhinted", small, small, 0, 1000, scratch=False, **kw)
        add(f"{family}_n{small}_lds_cap_{_cap_above(small)}", "lds_unhinted", small, _cap_above(small), 0, 1000, scratch=False, **kw)
        for limit in (0, 1000):
            add(f"{family}_n{small}_lds_then_radix_limit{limit}", "lds_then_radix", small, BIG_CAPACITY, 0, limit, **kw)
        for tag, hint, cap in _hints(large):
            for limit in (0, 1000):
                add(f"{family}_n{large}_radix_{tag}_limit{limit}", "radix", large, cap, hint, limit, **kw)
        for n in FAMILY_SIZES:
            for tag, hint, cap in (_hints(n)[0], _hints(n)[2]):
                add(f"{family}_n{n}_captured_{tag}", "captured", n, cap, hint, 1000, captured=True, **kw)
    # the key codec's field widths (radix route only)
    for n in ID_LIMIT_SIZES:
        for limit in ID_LIMITS:
            add(f"limit{limit}_n{n}", "radix", n, n + 300, n, limit, family="few" if limit == 0 or limit >= n else "adjacent")
        for limit in TIGHT_LIMITS:
            add(f"limit{limit}_n{n}_adjacent", "radix", n, n + 300, n, limit, family="adjacent")
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES: List[Case] = _build()
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
NAMES: List[str] = [c.name for c in CASES]


def buffer(c: Case) -> np.ndarray:
    """The ``capacity`` records the case hands to the sort: c.n live ones, then bytes no generator above would produce
    (random, none zero) so that "left as it was" can be told from "sorted" and from "zeroed"."""
    import zlib

    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    i, j = ids(c.id_limit, c.n, rng)
    rec = np.zeros((c.capacity, 2), dtype=np.float64)
    rec[: c.n] = records(scores(c.family, c.n, rng), i, j)
    tail = rng.integers(1, 256, size=(c.capacity - c.n) * 16, dtype=np.uint8)
    rec.view(np.uint8).reshape(-1)[c.n * 16:] = tail
    return rec


def check(c: Case, before: np.ndarray, after: np.ndarray) -> None:
    """What the header defines for the case, on the buffer's bytes before and after the call."""
    got, src = words(after), words(before)
    assert got.shape == src.shape == (c.capacity, 2)
    if c.ordered:
        want = words(reference_order(before[: c.n]))
        wrong = np.flatnonzero((got[: c.n] != want).any(axis=1))
        if wrong.size:
            r = int(wrong[0])
            raise AssertionError(
                f"{c.name}: {wrong.size} of {c.n} records differ from the canonical order, first at {r}: got "
                f"{tuple(v[0] for v in columns(after[r:r + 1]))}, want {tuple(v[0] for v in columns(want.view(np.float64)[r:r + 1]))}")
    else:
        assert np.array_equal(multiset(after[: c.n]), multiset(before[: c.n])), f"{c.name}: a record was lost or altered"
    if c.bound < c.capacity:
        moved = np.flatnonzero((got[c.bound:] != src[c.bound:]).any(axis=1))
        assert moved.size == 0, f"{c.name}: {moved.size} records behind n_hint = {c.bound} written, first {c.bound + int(moved[0])}"


# ------------------------------------------------------------------------------------------------------- the key codec
def score_key(score) -> np.ndarray:
    """K of the header: ~A."""
    return ~ascending_bits(score)


def pack(score, i, j, id_limit: int) -> List[int]:
    """The header's key of every record as a Python integer of 64 + 2 * bits bits."""
    bits = id_bits(id_limit)
    flip = 0x80000000 if bits == 32 else 0
    field = lambda v: (int(v) & 0xFFFFFFFF) ^ flip
    out = []
    for k, a, b in zip(score_key(score).tolist(), np.asarray(i).tolist(), np.asarray(j).tolist()):
        fa, fb = field(a), field(b)
        assert fa < (1 << bits) and fb < (1 << bits), "an id outside the promised range"
        out.append((k << (2 * bits)) | (fa << bits) | fb)
    return out


def unpack(keys: List[int], id_limit: int) -> np.ndarray:
    bits = id_bits(id_limit)
    flip = 0x80000000 if bits == 32 else 0
    mask = (1 << bits) - 1
    k = np.asarray([key >> (2 * bits) for key in keys], dtype=np.uint64)
    a = ~k
    b = a ^ np.where(a >> np.uint64(63), np.uint64(1) << np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF))
    as_i32 = lambda vals: np.asarray(vals, dtype=np.uint32).view(np.int32)
    return records(b.view(np.float64), as_i32([((key >> bits) & mask) ^ flip for key in keys]),
                   as_i32([(key & mask) ^ flip for key in keys]))


# --------------------------------------------------------------------------------------- the id_limit of the wrappers
N_LEFT, N_RIGHT, TOP_K = 103, 100, 100  # 10 300 records at threshold 0.0: beyond LDS_MAX, so the sort reads id_limit
WRAPPERS = ("jaccard_raw_grid", "indel_raw_grid", "jaccard_levels_grid", "indel_levels_grid",
            "jaccard_raw_floor_grid", "indel_raw_floor_grid", "jaccard_levels_floor_grid", "indel_levels_floor_grid",
            "jaccard_raw_top_k", "indel_raw_top_k",
            "jaccard_raw_assign", "indel_raw_assign", "jaccard_levels_assign", "indel_levels_assign")
REFUSES_NEGATIVE_IDS = tuple(w for w in WRAPPERS if w.endswith("_assign"))  # (taken items are marked in arrays by caller id)
REFUSAL = "assign: caller ids must be >= 0"


def _ending_at(top: int, n: int) -> np.ndarray:
    return (top - 3 * (n - 1 - np.arange(n))).astype(np.int32)


def relabelings() -> Dict[str, Tuple[Optional[np.ndarray], Optional[np.ndarray]]]:
    """name -> (left orig, right orig), None = the default row numbers.  Every map is strictly increasing, so that it
    commutes with everything that breaks ties by id (top-k: j ascending; assignment: the canonical order)."""
    far = lambda n: (1_000_003 + 7 * np.arange(n)).astype(np.int32)
    neg = lambda n: np.concatenate([[-3], np.arange(1, n)]).astype(np.int32)
    return {
        "identity": (None, None),
        "far_left": (far(N_LEFT), None),
        "far_right": (None, far(N_RIGHT)),
        "max_2p14m1_left": (_ending_at((1 << 14) - 1, N_LEFT), None),
        "max_2p14_left": (_ending_at(1 << 14, N_LEFT), None),
        "max_2p14m1_right": (None, _ending_at((1 << 14) - 1, N_RIGHT)),
        "max_2p14_right": (None, _ending_at(1 << 14, N_RIGHT)),
        "negative_left": (neg(N_LEFT), None),
        "negative_right": (None, neg(N_RIGHT)),
    }


RELABELINGS = tuple(relabelings())


def relabelled(score, i, j, left_orig, right_orig):
    """The identity run's hits under the relabeling, in canonical order: (score, i, j)."""
    i = np.asarray(i, dtype=np.int32) if left_orig is None else np.asarray(left_orig, dtype=np.int32)[np.asarray(i)]
    j = np.asarray(j, dtype=np.int32) if right_orig is None else np.asarray(right_orig, dtype=np.int32)[np.asarray(j)]
    return columns(reference_order(records(score, i, j)))


def wrapper_items(seed: int = 5):
    """The items of both sides for all four table kinds, none empty: ``sets`` (token ids, <= 8 of 40), ``strings``
    (lower-case words), and two-level items of each (level 0 = the first half, level 1 = the whole)."""
    rng = np.random.default_rng(seed)

    def side(n):
        sets = [sorted(rng.choice(40, size=int(rng.integers(1, 9)), replace=False).tolist()) for _ in range(n)]
        strings = ["".join(rng.choice(list("abcdefgh"), size=int(rng.integers(2, 21)))) for _ in range(n)]
        return sets, strings

    (lsets, lstr), (rsets, rstr) = side(N_LEFT), side(N_RIGHT)
    halves = lambda row: [row[: max(1, len(row) // 2)], row]
    return dict(left_sets=lsets, right_sets=rsets, left_strings=lstr, right_strings=rstr,
                left_set_levels=[halves(r) for r in lsets], right_set_levels=[halves(r) for r in rsets],
                left_string_levels=[halves(s) for s in lstr], right_string_levels=[halves(s) for s in rstr])
