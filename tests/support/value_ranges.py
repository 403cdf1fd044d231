"""Column VALUES at the edges of their ranges, shared by tests/test_cpu_value_ranges.py (the premises, with the oracle and
plain Python alone) and tests/test_gpu_value_ranges.py (every entry against the oracle, bit for bit).

* Part A -- token ids over the whole int32 range.  The levels Jaccard kernels keep ``id << 6`` in 32 bits, i.e. they compare
  ids modulo 2^26 (include/nsm_hip.h: ``NSM_LEVELS_ID_LIMIT``); the RAW kernels compare whole ids.  ``LOW`` holds the ids a
  levels table may carry, the two largest of which shift to the bit patterns of the padding; ``IMAGES`` holds ids that are
  congruent to a ``LOW`` id.  An ALIAS PAIR is a left and a right item whose id sets are disjoint as integers and equal
  modulo 2^26: its true score is 0, a 26-bit compare scores it like a copy.
* Part B -- strings over two or three symbols: runs, blocks and periodic strings whose 32-bucket histogram counts pass the
  ``uint8`` ceiling of the ``hist`` column (two symbols share a bucket), next to the lengths at which the LCS kernels change
  their word count.
* Part C -- a per-row restatement of what include/nsm_hip.h says ``nsm_build_set_table`` / ``nsm_build_str_table`` produce:
  loops over plain ints, nothing from ``tables.py``.
* Part D -- the strings of Part B over alphabets on either side of a multiple of 64 symbols, for the Levenshtein sweeps
  (tests/test_gpu_edit_ranges.py): their match masks are laid out by ``pm_stride``, the alphabet and its pad code rounded up
  to a multiple of 64, and at stride 512 they pass the 64 KB of LDS a kernel gets without asking.  The yardstick there is
  the two-row programme of tests/support/edit_distance.py, not the oracle.

The grids are ``tp.ProbeGrid`` objects, so ``tp.all_scores`` / ``tp.expectation`` / ``tp.RowRanks`` serve them as they
serve the threshold probes.  Every generator is deterministic: its own ``random.Random(seed)``.
"""
import random
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from support import threshold_probes as tp

# =========================================================================================================== Part A
P26 = 1 << 26
LEVELS_ID_LIMIT = P26        # include/nsm_hip.h: NSM_LEVELS_ID_LIMIT
GLOBAL_INDEX_LIMIT = 1 << 25  # ids of a table that carries the global inverted index are below it (builders.hip)
INT32_MAX = (1 << 31) - 1
INT32_MIN = -(1 << 31)
N_LEFT, N_RIGHT = 70, 130    # more than 64 left rows; two full right tiles of 64 and a ragged one
JACCARD_THRESHOLDS = (0.0, 0.3, 0.6, 1.0)

# (2^26 - 1) << 6 and (2^26 - 2) << 6 are the bit patterns of -1 << 6 and -2 << 6: the left and the right padding
LOW = (0, 1, 5, 63, 1 << 16, (1 << 24) - 1, 1 << 24) + tuple(range(P26 - 60, P26))
BASES = tuple(b for b in LOW if b <= 1 << 24)
IMAGES = tuple(sorted({b + k * P26 for b in BASES for k in (1, 2, 31)} | {INT32_MAX}))
# residue -> the ids of LOW + IMAGES that have it (INT32_MAX = 2^26 - 1 + 31 * 2^26)
CLASSES: Dict[int, Tuple[int, ...]] = {b: (b, b + P26, b + 2 * P26, b + 31 * P26) for b in BASES}
CLASSES[P26 - 1] = (P26 - 1, INT32_MAX)
SMALL = (0, 1, 5, 63, 1 << 16, (1 << 22) - 1, 1 << 22) + tuple(range((1 << 22) + 1, (1 << 22) + 61))  # ids a global index takes
# (a partitioned levels table keys its postings by (category, id): 64 key spaces, so its ids stay below 2^17 here)
SMALL_LEVELS = (0, 1, 5, 63, 1 << 16) + tuple(range((1 << 16) - 62, 1 << 16))


def jaccard(a: Sequence[int], b: Sequence[int]) -> float:
    a, b = set(a), set(b)
    return len(a & b) / len(a | b)


def levels_score(x: Sequence, y: Sequence, ratio: Callable) -> float:
    """compare_terms over two level lists: step s compares level min(s, L - 1) of either item and weighs 2^-s."""
    score, factor = 0.0, 1.0
    for s in range(1, max(len(x), len(y)) + 1):
        factor *= 0.5
        score += ratio(x[min(s, len(x) - 1)], y[min(s, len(y) - 1)]) * factor
    return score


def category_match(cl: int, cr: int, mode: int) -> bool:
    return mode == tp.CAT_NONE or (cl & cr) != 0 or (mode == tp.CAT_INTERSECT_OR_BOTH_EMPTY and cl == 0 and cr == 0)


def set_scores(g: tp.ProbeGrid, key: Callable[[int], int] = lambda v: v) -> list:
    """The hit list of a Jaccard grid at threshold 0.0 from Python sets alone, in the canonical order.  ``key`` maps every
    id before it is compared: ``lambda v: v % 2**26`` is what a kernel that keeps ``id << 6`` in 32 bits computes, as long
    as no row holds two ids of one residue (the generators see to that for the levels grids)."""
    out = []
    for i, x in enumerate(g.left):
        for j, y in enumerate(g.right):
            if g.raw:
                s = jaccard([key(v) for v in x], [key(v) for v in y])
            else:
                if g.cat_l is not None and not category_match(int(g.cat_l[i]), int(g.cat_r[j]), g.mode):
                    continue
                s = levels_score([[key(v) for v in lv] for lv in x], [[key(v) for v in lv] for lv in y], jaccard)
            out.append((s, i, j))
    return sorted(out, key=lambda h: (-h[0], h[1], h[2]))


def residue(v: int) -> int:
    return v % P26


def _alias_of(rng, row: Sequence[int]) -> List[int]:
    """Every id of ``row`` replaced by another id of its residue class."""
    return [rng.choice([v for v in CLASSES[residue(x)] if v != x]) for x in row]


def _class_row(rng, size: int, low_only: bool = False) -> List[int]:
    """``size`` ids of distinct residue classes."""
    return [CLASSES[r][0] if low_only else rng.choice(CLASSES[r]) for r in rng.sample(sorted(CLASSES), size)]


def padded(rows: Sequence[Sequence[int]], width: int) -> np.ndarray:
    ids = np.full((len(rows), width), -1, dtype=np.int32)
    for r, row in enumerate(rows):
        ids[r, : len(row)] = row
    return ids


def raw_ids(width: int, pool_name: str = "both") -> tp.ProbeGrid:
    """RAW id rows of one width.  ``both``: ids from LOW and IMAGES (any int32 >= 0 is a RAW id), 24 alias pairs among them;
    ``small``: ids below 2^25 only, for a right table that carries the global inverted index (no alias pairs: nothing is
    congruent there).  Rows of 1 .. ``width`` ids, full rows on both sides, copies and near-copies of left rows."""
    rng = random.Random(3100 + width + (7 if pool_name == "small" else 0))
    pool = list(LOW + IMAGES) if pool_name == "both" else list(SMALL)
    row = lambda: rng.sample(pool, rng.choice((1, 2, 3, rng.randint(1, min(width, len(pool))), min(width, len(pool)))))
    left = [row() for _ in range(N_LEFT)]
    right = [row() for _ in range(N_RIGHT)]
    alias, planted = [], []
    slots = list(range(N_RIGHT))
    rng.shuffle(slots)
    if pool_name == "both":
        for k in range(24):  # sizes 1 .. 8: every residue class at once in the largest
            i = 2 + 2 * k
            left[i] = _class_row(rng, 1 + k % 8)
            j = slots.pop()
            right[j] = _alias_of(rng, left[i])
            rng.shuffle(right[j])
            alias.append((i, j))
        # the issue's own example
        left[0], right[slots.pop()] = [5, 63, 1 << 16], [5 + P26, 63 + 2 * P26, (1 << 16) + 31 * P26]
        alias.append((0, [j for j in range(N_RIGHT) if right[j] == [5 + P26, 63 + 2 * P26, (1 << 16) + 31 * P26]][0]))
    for k in range(30):  # copies (1.0), one id fewer, one id more or swapped (0.3 .. 0.9 depending on the size)
        i = rng.randrange(N_LEFT)
        j = slots.pop()
        src = list(left[i])
        if k % 3 == 1 and len(src) > 1:
            src.pop(rng.randrange(len(src)))
        elif k % 3 == 2:
            extra = [v for v in pool if v not in src]
            if len(src) < width:
                src.append(rng.choice(extra))
            else:
                src[rng.randrange(len(src))] = rng.choice(extra)
        rng.shuffle(src)
        right[j] = src
        planted.append((i, j))
    g = tp.ProbeGrid(f"value_raw_ids_{pool_name}_{width}", "jaccard", True, left, right, size=width, subset=planted)
    g.tight = {"alias": alias}
    return g


def _levels_of(row: Sequence[int], cuts: Sequence[int]) -> List[List[int]]:
    return [list(row[:c]) for c in cuts]


def _cuts(rng, total: int, depth: int) -> List[int]:
    """``depth`` non-decreasing prefix lengths in 1 .. total, the last one ``total``."""
    return sorted(rng.randint(1, total) for _ in range(depth - 1)) + [total]


def nested_arrays(items: Sequence[Sequence[Sequence[int]]], width: int, max_levels: int = 4):
    """(ids [n][width] padded with -1, plen uint8 [n][max_levels], nlev int32 [n]) of suffix-nested items: what
    ``SetTable.from_nested_arrays`` takes, raw ids, no vocabulary."""
    n = len(items)
    ids = np.full((n, width), -1, dtype=np.int32)
    plen = np.zeros((n, max_levels), dtype=np.uint8)
    nlev = np.zeros(n, dtype=np.int32)
    for k, it in enumerate(items):
        ids[k, : len(it[-1])] = it[-1]
        nlev[k] = len(it)
        for l in range(max_levels):
            plen[k, l] = len(it[min(l, len(it) - 1)])
    return ids, plen, nlev


def levels_ids(pool_name: str, width: int, variant: str = "plain") -> tp.ProbeGrid:
    """Nested id sets of 1 .. 4 levels in rows of ``width``.

    * ``low``: ids from LOW (all below 2^26) -- the ids a levels table may hold, the two that look like padding included in
      many rows.  No two ids of LOW are congruent, so there is nothing to alias.
    * ``small``: ids from SMALL_LEVELS, for tables that carry the global inverted index.
    * ``images``: ids from LOW and IMAGES, every row with distinct residues, and 24 alias pairs.  Twelve alias "at every
      level": the right item is the left item with every id replaced by a congruent one (the shifted compare sees a copy).
      Twelve "at the last level only" (depth 3 or 4): the right row lists the congruent ids in reverse order, so that every
      level before the last is disjoint from its partner even modulo 2^26 and only the last level aliases.
    Copies and near-copies of left items give true hits at 0.3 and 0.6 (a levels score is below 1.0: its weights sum to
    1 - 2^-steps)."""
    rng = random.Random(3200 + width + {"low": 0, "small": 1, "images": 2}[pool_name])
    pool = list({"low": LOW, "small": SMALL_LEVELS}.get(pool_name, ()))
    most = min(width, len(pool) if pool else len(LOW))

    def item(depth=None, total=None):
        depth = depth or rng.randint(1, 4)
        total = total or rng.choice((depth, rng.randint(depth, most), rng.randint(depth, most), most))
        # (images: one id per residue -- a LOW id or, where it has any, one of its images)
        row = rng.sample(pool, total) if pool else [rng.choice(CLASSES.get(r, (r,))) for r in rng.sample(LOW, total)]
        return _levels_of(row, _cuts(rng, total, depth))

    left = [item() for _ in range(N_LEFT)]
    right = [item() for _ in range(N_RIGHT)]
    if pool_name == "low":  # the two padding look-alikes, alone and together, on either side
        for k, row in enumerate(([P26 - 1], [P26 - 2], [P26 - 2, P26 - 1], [P26 - 1, P26 - 2, 0])):
            left[60 + k] = _levels_of(row, [len(row)] * (1 + k % 2))
            right[120 + k] = _levels_of(row[::-1], [len(row)])
    slots = [j for j in range(N_RIGHT) if j < 120]
    rng.shuffle(slots)
    alias, planted = [], []
    if pool_name == "images":
        for k in range(24):
            i = 1 + 2 * k
            depth = 1 + k % 4 if k < 12 else 3 + k % 2
            total = max(depth, 2 + k % 7) if k < 12 else 6 + k % 3
            row = _class_row(rng, total)
            if k < 12:
                cuts = _cuts(rng, total, depth)
                left[i], twin = _levels_of(row, cuts), _levels_of(_alias_of(rng, row), cuts)
            else:  # prefixes of at most half the row: the levels before the last never meet, the last ones alias
                cuts = sorted(rng.randint(1, total // 2) for _ in range(depth - 1)) + [total]
                left[i], twin = _levels_of(row, cuts), _levels_of(_alias_of(rng, row)[::-1], cuts)
            j = slots.pop()
            right[j] = twin
            alias.append((i, j))
    for k in range(36):  # copies, the last level cut off, the step-1 level one id short
        i = rng.randrange(N_LEFT) if pool_name != "low" or k % 6 else 60 + (k // 6) % 4
        j = slots.pop()
        src = [list(lv) for lv in left[i]]
        if k % 3 == 1 and len(src) > 1:
            src = src[:-1]
        elif k % 3 == 2 and len(src[-1]) > 1:
            x = src[-1][-1]
            src = [[v for v in lv if v != x] for lv in src]
            src = [lv for lv in src if lv] or [[x]]
        right[j] = src
        planted.append((i, j))
    g = tp.ProbeGrid(f"value_levels_ids_{pool_name}_{width}", "jaccard", False, left, right, size=width, subset=planted + alias)
    g = tp._categories(rng, g, variant)
    g.tight = {"alias": alias}
    g.subset = planted
    return g


JACCARD_RAW = [f"value_raw_ids_both_{w}" for w in (16, 32, 64)]
JACCARD_RAW_SMALL = [f"value_raw_ids_small_{w}" for w in (16, 64)]
_VARIANT = lambda v: "" if v == "plain" else f"-{v}"
LEVELS_LOW = [f"value_levels_ids_low_16{_VARIANT(v)}" for v in tp.VARIANTS] + ["value_levels_ids_low_32", "value_levels_ids_low_64"]
LEVELS_SMALL = [f"value_levels_ids_small_16{_VARIANT(v)}" for v in tp.VARIANTS]
LEVELS_IMAGES = [f"value_levels_ids_images_16{_VARIANT(v)}" for v in tp.VARIANTS] + \
    ["value_levels_ids_images_32", "value_levels_ids_images_64"]

_BUILT: Dict[str, tp.ProbeGrid] = {}


def grid(name: str) -> tp.ProbeGrid:
    if name not in _BUILT:
        base, _, variant = name.partition("-")
        parts = base.split("_")
        if base.startswith("value_raw_ids_"):
            g = raw_ids(int(parts[4]), parts[3])
        elif base.startswith("value_levels_ids_"):
            g = levels_ids(parts[3], int(parts[4]), variant or "plain")
        elif base.startswith("value_raw_sat_"):
            g = raw_saturated(int(parts[3]))
        elif base.startswith("value_raw_str_"):
            g = raw_strings(int(parts[3]), int(parts[4]))
        elif base.startswith("value_levels_str_"):
            g = levels_strings(int(parts[3])) if len(parts) == 4 else levels_strings(int(parts[3]), int(parts[4]), *EDIT_LEVELS_ITEMS)
        else:
            raise KeyError(name)
        assert g.name == name, (g.name, name)
        _BUILT[name] = g
    return _BUILT[name]


def alias_pairs(g: tp.ProbeGrid) -> List[Tuple[int, int]]:
    return list(g.tight.get("alias", []))


def shifted_compare_scores(g: tp.ProbeGrid) -> list:
    """What kernels that compare ``id << 6`` in 32 bits answer at threshold 0.0: the set scorer on ids modulo 2^26."""
    for it in g.left + g.right:
        for lv in ([it] if g.raw else it):
            assert len({residue(v) for v in lv}) == len(lv), "two ids of one residue in a row: the model does not cover it"
    return set_scores(g, residue)


# =========================================================================================================== Part B
INDEL_THRESHOLDS = (0.0, 0.5, 2 / 3, 0.75, 1.0)  # runs of m and 2 m units score exactly 2/3
RUNS = (1, 63, 64, 65, 127, 128, 129, 254, 255, 256, 257, 300, 511, 512)
BLOCKS = ((200, 200), (255, 1), (256, 256), (100, 412))  # the shared bucket passes 255 although neither symbol does
# (alphabet, a, b, c, d): b shares a's 32-bucket (b = a + 32 = a mod 32); c has its own; d shares a's 16-bucket only
SYMBOLS = {40: (3, 35, 4, 19), 255: (254, 222, 253, 238)}
# the alphabets on either side of a multiple of 64 symbols + the pad code (Part D): a = alphabet - 1 is the highest legal
# code (the pad code is ``alphabet``), b = a - 32 shares a's 32-bucket, c = a - 1, d = a - 16
SEAM_ALPHABETS = (63, 64, 127, 128, 191, 192)
SYMBOLS.update({n: (n - 1, n - 33, n - 2, n - 17) for n in SEAM_ALPHABETS})
STR_LEFT, STR_RIGHT = 32, 72  # two right tiles


def indel_ratio(m: int, n: int, lcs: int) -> float:
    """include/nsm_hip.h: ((1 - (la + lb - 2 LCS) / (la + lb)) * 100) / 100, 0 when either string is empty."""
    if m == 0 or n == 0:
        return 0.0
    return ((1 - (m + n - 2 * lcs) / (m + n)) * 100) / 100


def string_pool(stride: int, alphabet: int) -> Dict[str, List[int]]:
    """label -> code units, cut to what fits ``stride``."""
    a, b, c, d = SYMBOLS[alphabet]
    pool: Dict[str, List[int]] = {"empty": []}
    for n in RUNS:
        if n <= stride:
            pool[f"a^{n}"] = [a] * n
    blocks = BLOCKS if stride > 64 else ((32, 32), (63, 1), (1, 63), (20, 44))
    if stride == 256:
        blocks = BLOCKS + ((128, 128), (1, 255), (56, 200))
    for m, n in blocks:
        if m + n <= stride:
            pool[f"a^{m}b^{n}"] = [a] * m + [b] * n
            pool[f"a^{m}c^{n}"] = [a] * m + [c] * n
            if stride == 64:  # a and d meet in one bucket of the 16-bucket histogram only
                pool[f"a^{m}d^{n}"] = [a] * m + [d] * n
    for n in (stride // 2, stride // 4):
        pool[f"(ab)^{n}"] = [a, b] * n
        pool[f"(ba)^{n}"] = [b, a] * n
    for n in (stride // 3, stride // 6):
        pool[f"(abc)^{n}"] = [a, b, c] * n
    if stride == 64:
        for n in (2, 31, 32, 33):
            pool[f"a^{n}"] = [a] * n
    rng = random.Random(3300 + stride + alphabet)
    for k in range(8):
        n = rng.choice((stride, stride - 1, rng.randint(stride // 2, stride), rng.randint(1, stride)))
        pool[f"random{k}"] = [rng.choice((a, a, a, b, b, c)) for _ in range(n)]
    return pool


def raw_strings(stride: int, alphabet: int = 40) -> tp.ProbeGrid:
    """At most 32 x 72 strings of the pool.  Left: the runs, the blocks, a periodic string of each kind, the empty string,
    random strings.  Right: the whole pool, then second copies of the runs (equal lengths: exact ties across rows and
    length classes), reversed blocks, and one-unit edits of left strings."""
    rng = random.Random(3400 + stride + alphabet)
    a, b, c, _ = SYMBOLS[alphabet]
    pool = string_pool(stride, alphabet)
    labels = list(pool)
    runs = [k for k in labels if k.startswith("a^") and k[2:].isdigit()]
    blocks = [k for k in labels if "^" in k and not k.startswith("(") and k not in runs]
    periodic = [k for k in labels if k.startswith("(")]
    rand = [k for k in labels if k.startswith("random")]
    pick = runs + blocks + periodic[::2] + ["empty"] + rand
    left = [list(pool[k]) for k in pick[:STR_LEFT]]
    while len(left) < STR_LEFT:
        left.append([rng.choice((a, b, c)) for _ in range(rng.randint(1, stride))])
    right = [list(pool[k]) for k in labels[:STR_RIGHT]]
    extra = [list(pool[k]) for k in runs] + [list(pool[k])[::-1] for k in blocks] + [[], []]
    while len(right) < STR_RIGHT:
        if extra:
            right.append(extra.pop(0))
        else:
            src = list(left[rng.randrange(len(left))])
            if src:
                src[rng.randrange(len(src))] = c
            right.append(src)
    rng.shuffle(right)
    return tp.ProbeGrid(f"value_raw_str_{stride}_{alphabet}", "indel", True, left, right[:STR_RIGHT], size=stride)


TAIL_RUNS = tuple(range(248, 256))  # the right rows of the last, partial tile of ``raw_saturated``


def raw_saturated(stride: int) -> tp.ProbeGrid:
    """The RAW grid of strings beyond 64 units skips a left row only when the histogram bound fails in EVERY lane of a right
    tile of 64 length-sorted rows, so a mixed tile hides a wrong bound.  Here the right side is 64 rows of at least 256
    units (the first tile) and the runs a^248 .. a^255 (the second tile, nothing else in it): against the left rows a^256
    and a^255 b -- bucket count 256 -- all eight are hits near 0.99, with clipped counts a distance of at most 8 apart, with
    wrapped counts 248 and more.  Left: the saturated strings of the pool first, then the rest of it."""
    rng = random.Random(3450 + stride)
    a, b, c, _ = SYMBOLS[40]
    pool = string_pool(stride, 40)
    full = [s for s in pool.values() if saturated(s)]
    left = (full + [s for s in pool.values() if not saturated(s)])[:STR_LEFT]
    long_rows = [list(s) for s in pool.values() if len(s) >= 256]
    while len(long_rows) < 64:
        long_rows.append([rng.choice((a, a, b, c)) for _ in range(rng.randint(256, stride))])
    right = long_rows[:64] + [[a] * n for n in TAIL_RUNS]
    rng.shuffle(right)
    return tp.ProbeGrid(f"value_raw_sat_{stride}_40", "indel", True, [list(s) for s in left], right, size=stride)


def _one_of_each_removed(s: Sequence[int]) -> List[int]:
    """``s`` without the first occurrence of each of its symbols: a^256 -> a^255, a^256 c^256 -> a^255 c^255."""
    out, seen = [], set()
    for u in s:
        if u in seen:
            out.append(u)
        seen.add(u)
    return out


def levels_strings(stride: int, alphabet: int = 40, n_left: int = 24, n_right: int = 70) -> tp.ProbeGrid:
    """24 x 70 items of 1 .. 3 levels, every level a string of the pool of ``stride`` (alphabet 40).  A third of the right
    items are left items, some with one level exchanged.  Twelve left items of depth 3 carry a string with a saturated
    bucket as their step-1 level; each has two right partners that differ from it in that level alone, by one unit per
    symbol -- near-copies (score about 0.87) whose step-1 histograms are far apart once a count wraps.  ``alphabet``,
    ``n_left``, ``n_right``: the same over another alphabet's symbols and with fewer items (half as many saturated ones as
    left items); the grid's name then ends in the alphabet."""
    rng = random.Random(3500 + stride + (0 if alphabet == 40 else alphabet))
    pool = [s for s in string_pool(stride, alphabet).values() if s]  # (an empty level string is fine, but scores 0 everywhere)
    pool_e = pool + [[]]
    item = lambda: [list(rng.choice(pool_e if rng.random() < 0.1 else pool)) for _ in range(rng.randint(1, 3))]
    left = [item() for _ in range(n_left)]
    right = [item() for _ in range(n_right)]
    for k in range(0, n_right, 3):
        src = [list(lv) for lv in left[rng.randrange(n_left)]]
        if k % 2:
            src[rng.randrange(len(src))] = list(rng.choice(pool))
        right[k] = src
    full = sorted((s for s in pool if saturated(s)), key=lambda s: (max(bucket_counts(s)) % 256, len(s)))
    for k in range(n_left // 2):
        x = full[k % len(full)]
        y = _one_of_each_removed(x)
        left[2 * k] = [list(rng.choice(pool)), list(x), list(rng.choice(pool))]
        right[5 * k + 1] = [list(rng.choice(pool)), list(y), list(left[2 * k][2])]
        right[5 * k + 2] = [list(y), list(y), list(left[2 * k][2])]
    name = f"value_levels_str_{stride}" + ("" if alphabet == 40 else f"_{alphabet}")
    return tp.ProbeGrid(name, "indel", False, left, right, size=stride)


def levels_wrap_witnesses(g: tp.ProbeGrid, all_hits: Sequence[tuple]) -> List[Tuple[int, int, float]]:
    """(i, j, threshold) of the hits of a levels grid that a step-1 histogram bound over WRAPPED counts would prune:
    score <= ratio_1 / 2 + (1 - 2^-steps - 1/2), with ratio_1 bounded by the histograms of the step-1 strings."""
    out = []
    for s, i, j in all_hits:
        x, y = (it[min(1, len(it) - 1)] for it in (g.left[i], g.right[j]))
        if not (saturated(x) or saturated(y)):
            continue
        rest = 1.0 - 0.5 ** max(len(g.left[i]), len(g.right[j])) - 0.5
        bound = histogram_bound(x, y, lambda v: v % 256) / 2 + rest
        for thr in INDEL_THRESHOLDS:
            if thr > 0.0 and s >= thr and bound < thr:
                out.append((i, j, thr))
                break
    return out


RAW_STRINGS = ["value_raw_str_64_40", "value_raw_str_128_40", "value_raw_str_256_40", "value_raw_str_512_40",
               "value_raw_str_256_255", "value_raw_str_512_255"]
RAW_SATURATED = ["value_raw_sat_256_40", "value_raw_sat_512_40"]
LEVELS_STRINGS = ["value_levels_str_256", "value_levels_str_512"]

# =========================================================================================================== Part D
# The Levenshtein sweeps (csrc/edit_raw.hip, edit_levels.hip) keep one match mask per symbol in LDS: ``pm_stride`` symbols,
# the alphabet and its pad code rounded up to a multiple of 64.  The RAW sweep holds the masks of ``TOP_G`` left rows at
# once, 8 bytes per symbol and 64 code units of the stride: from 64 KB on the launcher has to raise the kernel's limit.
TOP_G = 8  # csrc: kTopG, the left rows of one block of the RAW per-item sweeps
EDIT_CUT = (19, 40)  # rows of the grids at strides 256 and 512: three groups of TOP_G with a ragged last one
EDIT_LEVELS_ITEMS = (12, 40)
EDIT_LENGTH_SEAMS = (0, 1, 255, 256, 257, 511, 512)


def pm_stride(alphabet: int) -> int:
    return ((alphabet + 1) + 63) // 64 * 64


def edit_lds_bytes(stride: int, alphabet: int) -> int:
    """Dynamic LDS of the RAW sweep: TOP_G rows x pm_stride symbols x (stride / 64) words of 8 bytes."""
    return TOP_G * pm_stride(alphabet) * (stride // 64) * 8


def _spread(rows: Sequence, limit: int, wanted_lengths: Sequence[int]) -> List:
    """At most ``limit`` of ``rows``: the first row of every wanted length, then the others evenly spread, input order."""
    first = []
    for n in wanted_lengths:
        hit = [k for k, r in enumerate(rows) if len(r) == n and k not in first]
        first += hit[:1]
    rest = [k for k in range(len(rows)) if k not in first]
    need = max(0, min(limit, len(rows)) - len(first))
    picked = first + [rest[(q * len(rest)) // need] for q in range(need)]
    return [rows[k] for k in sorted(picked)]


def edit_raw_strings(stride: int, alphabet: int) -> tp.ProbeGrid:
    """``raw_strings`` for the Levenshtein sweeps.  Strides 64 and 128: the grid as it is (32 x 72).  Strides 256 and 512: at
    most 19 x 40 of its rows (the DP yardstick is quadratic in the length) -- on both sides the empty string, the lengths
    1, 255, 256, 257, 511, 512 and the runs of stride / 2 and stride units, the other rows evenly spread."""
    g = raw_strings(stride, alphabet)
    left, right = g.left, g.right
    if stride >= 256:
        wanted = [n for n in EDIT_LENGTH_SEAMS + (stride // 2, stride) if n <= stride]
        left, right = _spread(left, EDIT_CUT[0], wanted), _spread(right, EDIT_CUT[1], wanted)
    return tp.ProbeGrid(f"value_edit_str_{stride}_{alphabet}", "indel", True, left, right, size=stride)


EDIT_RAW = [f"value_edit_str_64_{a}" for a in SEAM_ALPHABETS] + \
    ["value_edit_str_128_255", "value_edit_str_256_255", "value_edit_str_512_128", "value_edit_str_512_255"]
EDIT_RAW_W8 = EDIT_RAW[-2:]  # the two whose match masks need more than 64 KB
EDIT_LEVELS = ["value_levels_str_256_255", "value_levels_str_512_255"]
EDIT_METRICS = ("edit", "edit_within")

# query x prune x metric -> the instantiation of edit_top_k_kernel<W, PRUNE, HIST, GROUPED, Sink> that csrc/edit_raw.hip
# launches for it (W = stride / 64).  The threshold grid is the floor grid without floors; ``best`` is a profile and a floor
# grid.  The histogram filter runs under NSM_FLAG_PRUNE and NSM_METRIC_EDIT alone (``edit_hist``).
EDIT_SINKS = {"top_k": "TopLists<false>", "top_k_grouped": "TopLists<true>", "profile": "ScoreTally", "floor_grid": "FloorGate"}


def edit_instantiation(query: str, prune: bool, metric: str, words: int = 8) -> Tuple[int, bool, bool, str]:
    return words, prune, prune and metric == "edit", EDIT_SINKS[query]


EDIT_LAUNCHES = {(q, prune, m): edit_instantiation(q, prune, m) for q in EDIT_SINKS for prune in (True, False) for m in EDIT_METRICS}
# test of tests/test_gpu_edit_ranges.py -> the sinks it runs, each pruned and unpruned under either metric
EDIT_QUERIES = {"threshold_grid": ("floor_grid",), "top_k": ("top_k", "top_k_grouped"), "profile_and_best": ("profile", "floor_grid"),
                "floor_grid": ("floor_grid",)}

_EDIT_DW: Dict[str, dict] = {}
_EDIT_ALL: Dict[tuple, list] = {}


def edit_grid(name: str) -> tp.ProbeGrid:
    if name not in _BUILT:
        parts = name.split("_")
        _BUILT[name] = edit_raw_strings(int(parts[3]), int(parts[4])) if name.startswith("value_edit_str_") else grid(name)
    return _BUILT[name]


def edit_categories(g: tp.ProbeGrid, mode: int):
    """(left masks, right masks) of a levels grid for the category modes of Part D; none at mode 0."""
    from support import edit_distance as ed

    return ed.levels_categories(len(g.left), len(g.right)) if mode else (None, None)


def edit_records(g: tp.ProbeGrid, metric: str, mode: int = 0) -> list:
    """Every pair's record under a Levenshtein metric from the definitions (tests/support/edit_distance.py): d and w of
    two strings from ONE pass of the two-row programme (``ed.distance_table``, cached per grid: both metrics share it), RAW
    ``ed.score`` of them, levels ``compare_terms`` with that as score_func over the pairs the category masks admit.
    Canonical order; cached; never modified."""
    from oracle.compare import compare_terms
    from support import edit_distance as ed

    if (g.name, metric, mode) not in _EDIT_ALL:
        known = _EDIT_DW.setdefault(g.name, {})
        if not known:
            flat = lambda side: sorted({tuple(s) for it in side for s in ([it] if g.raw else it)})
            ed.distance_table(flat(g.left), flat(g.right), known)
        f = lambda a, b: ed.plain_score(metric, len(a), len(b), *known[tuple(a), tuple(b)])
        cl, cr = edit_categories(g, mode)
        hits = [((f(x, y) if g.raw else compare_terms(x, y, f)), i, j) for i, x in enumerate(g.left) for j, y in enumerate(g.right)
                if not mode or ed.category_match(int(cl[i]), int(cr[j]), mode)]
        _EDIT_ALL[g.name, metric, mode] = sorted(hits, key=lambda h: (-h[0], h[1], h[2]))
    return _EDIT_ALL[g.name, metric, mode]


def edit_thresholds(all_hits: Sequence[tuple]) -> Tuple[float, ...]:
    """The thresholds of a Part D grid, each with a pair exactly on it: 0.5 and 1.0 (a run of m units against one of 2 m:
    0.5 under "edit", 1.0 and 0.5 in the two orientations under "edit_within") and the distinct score two thirds of the way
    up.  A levels grid (no score reaches 1.0) has its distinct scores one third and two thirds of the way up."""
    distinct = sorted({h[0] for h in all_hits})
    mid = distinct[2 * len(distinct) // 3]
    return (0.5, mid, 1.0) if distinct[-1] == 1.0 else (distinct[len(distinct) // 3], mid)


def around(bases: Sequence[float]) -> List[float]:
    """Every base with its two neighbouring doubles."""
    import math

    return sorted({t for b in bases for t in (math.nextafter(b, -1.0), b, math.nextafter(b, 2.0))})


def alphabet_of(g: tp.ProbeGrid) -> int:
    parts = g.name.partition("-")[0].split("_")
    return int(parts[4]) if len(parts) > 4 else 40


def codes_of(rows: Sequence[Sequence[int]], stride: int, fill: int = 0):
    """(codes uint8 [n][stride], lengths int32 [n]): what ``StrTable.from_codes`` takes; unused slots hold ``fill``."""
    codes = np.full((len(rows), stride), fill, dtype=np.uint8)
    lengths = np.zeros(len(rows), dtype=np.int32)
    for r, row in enumerate(rows):
        codes[r, : len(row)] = row
        lengths[r] = len(row)
    return codes, lengths


def level_codes_of(items: Sequence[Sequence[Sequence[int]]], stride: int):
    """(codes, lengths, first, nlev) of one side: what ``tables.encode_level_codes`` takes."""
    rows = [lv for it in items for lv in it]
    nlev = np.array([len(it) for it in items], dtype=np.int32)
    first = np.concatenate([[0], np.cumsum(nlev)[:-1]]).astype(np.int32)
    return codes_of(rows, stride) + (first, nlev)


def bucket_counts(s: Sequence[int]) -> List[int]:
    h = [0] * 32
    for u in s:
        h[u & 31] += 1
    return h


def histogram_bound(x: Sequence[int], y: Sequence[int], counts: Callable[[int], int]) -> float:
    """The largest score the histogram bound LCS <= (la + lb - L1) / 2 allows, with every bucket count passed through
    ``counts``: ``lambda v: min(v, 255)`` is the ``hist`` column (clipping is 1-Lipschitz: L1 can only shrink, the bound
    stays valid), ``lambda v: v % 256`` a column whose counts wrap."""
    l1 = sum(abs(counts(p) - counts(q)) for p, q in zip(bucket_counts(x), bucket_counts(y)))
    return indel_ratio(len(x), len(y), (len(x) + len(y) - l1) // 2) if l1 <= len(x) + len(y) else -1.0


def saturated(s: Sequence[int]) -> bool:
    return max(bucket_counts(s)) > 255


def wrap_witnesses(g: tp.ProbeGrid, all_hits: Sequence[tuple]) -> List[Tuple[int, int, float]]:
    """(i, j, threshold) of the pairs with a saturated bucket on either side that are hits at ``threshold`` (one of
    INDEL_THRESHOLDS) and that a histogram bound over WRAPPED counts would prune there: hits a wrapping builder loses."""
    out = []
    for s, i, j in all_hits:
        x, y = g.left[i], g.right[j]
        if not (saturated(x) or saturated(y)):
            continue
        bound = histogram_bound(x, y, lambda v: v % 256)
        for thr in INDEL_THRESHOLDS:
            if thr > 0.0 and s >= thr and bound < thr:
                out.append((i, j, thr))
                break
    return out


# =========================================================================================================== Part C
_M1, _M2 = 0x9E3779B1, 0xC2B2AE35


def signature_model(ids: Sequence[int], multiplier: int) -> int:
    """include/nsm_hip.h, ``sig``: bits 0..57 = OR of 1 << ((((id * multiplier) >> 16) & 0xffff) * 58 >> 16) in 32-bit
    arithmetic; bits 58..63 = the low c of them set, c = ids that collided; c > 6: all 64 bits."""
    word = 0
    for v in ids:
        h16 = (((v * multiplier) & 0xFFFFFFFF) >> 16) & 0xFFFF
        word |= 1 << ((h16 * 58) >> 16)
    c = len(ids) - bin(word).count("1")
    return 0xFFFFFFFFFFFFFFFF if c > 6 else word | (((1 << c) - 1) << 58)


def set_table_model(rows: Sequence[Sequence[int]], width: int, side: int, nlev: Optional[Sequence[int]] = None,
                    plen: Optional[Sequence[Sequence[int]]] = None, cat: Optional[Sequence[int]] = None,
                    orig: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
    """The columns ``nsm_build_set_table`` is documented to produce (no partition, no inverted index), row by row.
    ``rows``: the caller's slots, negative = unused, anywhere.  RAW (``nlev`` None): a repeated id counts once, ids
    ascending.  Levels: first-appearance order kept; ``plen`` rows of ``max_levels`` bytes, entries past the last level
    ignored and rewritten to the last level's."""
    n = len(rows)
    levels = nlev is not None
    packed = []
    for row in rows:
        out: List[int] = []
        for v in row:
            if v < 0 or (not levels and v in out):
                continue
            out.append(v)
        assert len(out) <= width and len(set(out)) == len(out)
        packed.append(out if levels else sorted(out))
    order = sorted(range(n), key=lambda i: -len(packed[i]))  # (sorted() is stable: ties stay in the caller's order)
    pad = -1 if side == 0 else -2
    max_levels = len(plen[0]) if levels else 0
    cols = dict(ids=np.full((n, width), pad, dtype=np.int32), cnt=np.zeros(n, np.int32), sig=np.zeros(n, np.uint64),
                sig2=np.zeros(n, np.uint64), orig=np.zeros(n, np.int32), size_start=np.zeros(width + 2, np.int32))
    if levels:
        cols.update(nlev=np.zeros(n, np.int32), plen=np.zeros((n, max_levels), np.uint8), filt=np.zeros((n, 8), np.uint32))
        if cat is not None:
            cols["cat"] = np.zeros(n, np.uint64)
    for r, i in enumerate(order):
        ids = packed[i]
        cols["ids"][r, : len(ids)] = ids
        cols["cnt"][r] = len(ids)
        s1 = signature_model(ids, _M1)
        cols["sig"][r] = s1
        cols["sig2"][r] = signature_model(ids, _M2)
        cols["orig"][r] = i if orig is None else orig[i]
        if levels:
            L = nlev[i]
            cols["nlev"][r] = L
            for l in range(max_levels):
                cols["plen"][r, l] = plen[i][min(l, L - 1)]
            c = 0 if cat is None else int(cat[i])
            if cat is not None:
                cols["cat"][r] = c
            plen1 = plen[i][min(1, L - 1, max_levels - 1)]
            sl1 = signature_model(ids[:plen1], _M1)
            cols["filt"][r] = [s1 & 0xFFFFFFFF, s1 >> 32, c & 0xFFFFFFFF, c >> 32, plen1 | (len(ids) << 8) | (L << 16),
                               sl1 & 0xFFFFFFFF, sl1 >> 32, 0]
    for c in range(width + 2):  # rows with cnt == width - c are [size_start[c], size_start[c + 1])
        cols["size_start"][c] = sum(1 for i in range(n) if width - len(packed[i]) < c)
    return cols


def str_table_model(codes: Sequence[Sequence[int]], lengths: Sequence[int], alphabet: int, sort: bool,
                    orig: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
    """The columns ``nsm_build_str_table`` is documented to produce.  ``codes``: rows of ``stride`` bytes, anything at
    positions >= len."""
    n, stride = len(codes), len(codes[0])
    order = sorted(range(n), key=lambda i: -lengths[i]) if sort else list(range(n))
    cols = dict(codes=np.full((n, stride), alphabet, dtype=np.uint8), len=np.zeros(n, np.int32), orig=np.zeros(n, np.int32),
                hist=np.zeros((n, 32), np.uint8), hist16=np.zeros((n, 16), np.uint8))
    for r, i in enumerate(order):
        L = lengths[i]
        h = [0] * 32
        for p in range(L):
            cols["codes"][r, p] = codes[i][p]
            h[codes[i][p] & 31] += 1
        h = [min(v, 255) for v in h]
        cols["len"][r] = L
        cols["orig"][r] = i if orig is None else orig[i]
        cols["hist"][r] = h
        cols["hist16"][r] = [min(255, h[b] + h[b + 16]) for b in range(16)]
    if sort:  # rows with len == stride - c are [len_start[c], len_start[c + 1])
        cols["len_start"] = np.array([sum(1 for L in lengths if stride - L < c) for c in range(stride + 2)], dtype=np.int32)
    return cols


NEGATIVES = (-1, -2, -7, INT32_MIN)
BUILDER_ROWS = 300


def set_builder_case(width_in: int, width: int, levels: bool, max_levels: int = 4, n: int = BUILDER_ROWS, seed: int = 0,
                     holes: bool = True, repeats: bool = True):
    """Inputs of ``nsm_build_set_table`` that use every clause of its comment: ``rows`` [n][width_in] with valid ids in any
    slots and assorted negative values between them (``holes``), RAW rows with repeated ids, an immediate repeat among
    them (``repeats``), ids up to 2^31 - 1 (RAW) / 2^26 - 1 (levels), empty rows, full rows; levels: ``nlev``, ``plen``
    with garbage past the last level, ``cat``; ``orig`` with INT32_MAX among its values."""
    rng = random.Random(3600 + 1000 * width_in + 10 * width + levels + 7 * seed)
    pool = list(LOW) + ([] if levels else list(IMAGES)) + list(range(100, 140))
    most = min(width, width_in)
    rows, nlev, plen, cat = [], [], [], []
    for k in range(n):
        cnt = rng.choice((0, 1, most, rng.randint(0, most), rng.randint(0, most)))
        ids = rng.sample(pool, cnt)
        if not levels and repeats and cnt >= 1 and width_in - cnt >= 2 and k % 3 == 0:
            at = rng.randrange(cnt)
            ids = ids[: at + 1] + [ids[at]] + ids[at + 1:] + [ids[0]]  # (an immediate repeat, and one of the first id)
        slots = [rng.choice(NEGATIVES) for _ in range(width_in)]
        where = sorted(rng.sample(range(width_in), len(ids))) if holes else list(range(len(ids)))
        for p, v in zip(where, ids):
            slots[p] = v
        rows.append(slots)
        L = rng.randint(1, max_levels)
        lens = sorted(rng.randint(0, cnt) for _ in range(L))
        nlev.append(L)
        plen.append(lens + [rng.choice((0, 255, 3, cnt)) for _ in range(max_levels - L)])
        cat.append(rng.choice((0, 1, 5, (1 << 63) | 2, (1 << 64) - 1)))
    orig = rng.sample(range(INT32_MAX - 5 * n, INT32_MAX + 1), n)
    orig[rng.randrange(n)] = INT32_MAX
    return dict(rows=rows, nlev=nlev if levels else None, plen=plen if levels else None, cat=cat if levels else None, orig=orig)


def str_builder_case(stride: int, alphabet: int, n: int = BUILDER_ROWS, seed: int = 0):
    """Inputs of ``nsm_build_str_table``: lengths 0 .. stride with the edges, codes up to ``alphabet - 1``, rows that
    saturate a histogram bucket, and bytes >= alphabet at the positions past the length."""
    rng = random.Random(3700 + stride + alphabet + 7 * seed)
    codes, lengths = [], []
    for k in range(n):
        L = rng.choice((0, 1, stride, stride - 1, rng.randint(0, stride), rng.randint(0, stride)))
        few = [rng.randrange(alphabet) for _ in range(rng.choice((1, 2, 3, 40)))]
        codes.append([rng.choice(few) for _ in range(L)] + [rng.choice((0, alphabet, 255, 17)) for _ in range(stride - L)])
        lengths.append(L)
    orig = rng.sample(range(INT32_MAX - 5 * n, INT32_MAX + 1), n)
    orig[rng.randrange(n)] = INT32_MAX
    return dict(codes=codes, lengths=lengths, orig=orig)
