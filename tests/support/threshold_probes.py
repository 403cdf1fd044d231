"""Seeded grids and threshold probes for the FAST-PATH kernels (RAW and levels grids, top-k), shared by
tests/test_gpu_threshold_probes.py (every route of every kernel against the oracle, thresholds put exactly on oracle scores
and one ulp to either side) and tests/test_cpu_threshold_probes.py (the same grids through the oracle alone: do they hold
the shared scores, ulp twins and tight families that the GPU file relies on?).

A pair is a hit iff ``score >= threshold``; nearly every fast path decides from a bound derived from the threshold whether
to compute the score at all.  The grids are small (70 .. 90 left items, 64 * 3 + 37 right items: several row batches, three
full right tiles and a partial one) and hold plain ints: code units of strings, token ids of sets.  Every generator is
deterministic: its own ``random.Random(seed)``.

* RAW grids: one string / one id row per item.
* Levels grids: item -> level -> ints.  They plant TIGHT FAMILIES: right items copied from a left item with only the level
  that step 1 compares edited.  Every later step then compares identical operands (ratio 1.0, and every histogram / size
  bound of steps >= 2 is met with equality), so the pair's score sits exactly on what a pruning bound computes for it.  All
  copies of one family get the same kind of edit at different positions, hence one common score.
* ANAGRAM pairs (fuzzy levels): a later level is a permutation of its partner -- the histogram bound says 1.0, the ratio is
  below it.
"""
import bisect
import math
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

CAT_NONE, CAT_INTERSECT, CAT_INTERSECT_OR_BOTH_EMPTY = 0, 1, 2
N_RIGHT = 64 * 3 + 37
VARIANTS = ("plain", "cat1_partition", "cat2_lanes")  # no categories / CAT_INTERSECT partitioned / OR_BOTH_EMPTY per lane
FAMILY_SIZE = 12  # right copies per tight family
Pair = Tuple[int, int]


@dataclass
class ProbeGrid:
    name: str
    kind: str  # "indel" | "jaccard"
    raw: bool
    left: list   # raw: item -> ints; levels: item -> level -> ints
    right: list
    size: int = 0  # row stride (indel) / row width (jaccard) the encoders must choose
    cat_l: Optional[np.ndarray] = None
    cat_r: Optional[np.ndarray] = None
    mode: int = CAT_NONE
    partition: bool = False
    tight: Dict[str, List[Pair]] = field(default_factory=dict)  # family -> (i, j) pairs, all of one score
    anagram: List[Pair] = field(default_factory=list)
    subset: List[Pair] = field(default_factory=list)            # Jaccard: one side a subset of the other (at every level)
    duplicates: List[int] = field(default_factory=list)         # right items that are copies of one right item

    @property
    def pairs(self) -> int:
        return len(self.left) * len(self.right)

    def family_pairs(self) -> List[Pair]:
        return [p for fam in self.tight.values() for p in fam] + list(self.anagram)


def text(units: Sequence[int]) -> str:
    """The kernel side's string of a list of code units."""
    return "".join(map(chr, units))


# ------------------------------------------------------------------------------------------------------------ oracle
_ALL: Dict[str, list] = {}


def oracle_call(g: ProbeGrid, thr: float) -> list:
    from oracle import native

    if g.raw:
        fn = native.indel_raw if g.kind == "indel" else native.jaccard_raw
        return fn(native.csr(g.left), native.csr(g.right), thr, cap=g.pairs + 1)
    return native.levels(g.kind == "indel", g.left, g.right, thr, g.cat_l, g.cat_r, g.mode, cap=g.pairs + 1)


def all_scores(g: ProbeGrid) -> list:
    """The oracle's hit list at threshold 0.0 (a ratio is never negative: every pair the category masks allow), in the
    canonical order (score descending, i, j).  Cached per grid; never modified."""
    if g.name not in _ALL:
        _ALL[g.name] = oracle_call(g, 0.0)
    return _ALL[g.name]


def expectation(all_hits: Sequence[tuple], thr: float) -> list:
    """``[h for h in all_hits if h[0] >= thr]``: the list is ordered by score descending, so that is a prefix."""
    lo, hi = 0, len(all_hits)
    while lo < hi:
        mid = (lo + hi) // 2
        if all_hits[mid][0] >= thr:
            lo = mid + 1
        else:
            hi = mid
    return list(all_hits[:lo])


# ------------------------------------------------------------------------------------------------------------ probes
def _ulps_apart(a: float, b: float) -> int:
    ia, ib = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return int(ib - ia)


def shared_scores(all_hits: Sequence[tuple], n: int = 8) -> List[float]:
    """The ``n`` positive scores shared by the most pairs."""
    count: Dict[float, int] = {}
    for s, _, _ in all_hits:
        if s > 0.0:
            count[s] = count.get(s, 0) + 1
    return [s for s, _ in sorted(count.items(), key=lambda kv: (-kv[1], kv[0]))[:n]]


def ulp_twins(all_hits: Sequence[tuple], n: int = 8, ulps: int = 4) -> List[Tuple[float, float]]:
    """Up to ``n`` pairs (lower, upper) of distinct positive scores at most ``ulps`` ulps apart, spread over the score range."""
    distinct = sorted({h[0] for h in all_hits if h[0] > 0.0})
    twins = [(a, b) for a, b in zip(distinct, distinct[1:]) if _ulps_apart(a, b) <= ulps]
    if len(twins) <= n:
        return twins
    return [twins[(k * (len(twins) - 1)) // (n - 1)] for k in range(n)]


def landmark_scores(all_hits: Sequence[tuple]) -> List[float]:
    """The lowest positive score, the 10 / 25 / 50 / 75 / 90 % quantiles of the distinct scores, the highest below 1.0 and
    the highest."""
    distinct = sorted({h[0] for h in all_hits if h[0] > 0.0})
    if not distinct:
        return []
    below_one = [s for s in distinct if s < 1.0]
    picks = [distinct[0], distinct[-1]] + below_one[-1:]
    return picks + [distinct[(q * (len(distinct) - 1)) // 100] for q in (50, 10, 90, 25, 75)]


def family_scores(all_hits: Sequence[tuple], pairs: Sequence[Pair]) -> List[float]:
    wanted = set(pairs)
    return sorted({s for s, i, j in all_hits if (i, j) in wanted})


def probes(all_hits: Sequence[tuple], cap: int = 40, family: Sequence[Pair] = ()) -> List[float]:
    """Distinct scores to cut at, at most ``cap``.  Filled in this order, so that a smaller cap drops the landmarks first
    and never a tight-family score or an ulp twin: family scores, ulp twins (both members), shared scores, landmarks.  The
    grids plant at most 8 family scores (7 Jaccard families; 6 fuzzy ones and 2 anagram pairs), so with 16 twin members,
    8 shared scores and 8 landmarks the default cap of 40 holds every class whole (the CPU file asserts it)."""
    ordered: List[float] = list(family_scores(all_hits, family)) if family else []
    for a, b in ulp_twins(all_hits):
        ordered += [a, b]
    ordered += shared_scores(all_hits)
    ordered += landmark_scores(all_hits)
    out: List[float] = []
    for s in ordered:
        if s not in out and len(out) < cap:
            out.append(s)
    return sorted(out)


def thresholds_around(scores: Sequence[float]) -> List[float]:
    """One ulp below, on, and one ulp above every probe; deduplicated, ascending."""
    out = set()
    for s in scores:
        out |= {math.nextafter(s, 0.0), s, math.nextafter(s, 2.0)}
    return sorted(out)


# ----------------------------------------------------------------------------------------------------- top-k by rows
class RowRanks:
    """Per left item its records in the order (score descending, j ascending), and -- for a grouping of the right items --
    the representatives: a record is its group's best iff no earlier record of the row has that group, whatever the
    threshold (a threshold keeps a prefix of the row).  ``cut`` is then the definition of the top-k queries (the rank cut
    of the top-k tests; tests/support/grouped.py ``group_cut``) without sorting anything again."""

    def __init__(self, all_hits: Sequence[tuple], groups: Optional[Sequence[int]] = None) -> None:
        rows: Dict[int, list] = {}
        for h in all_hits:
            rows.setdefault(h[1], []).append(h)
        self.rows = {}
        for i, lst in rows.items():
            lst.sort(key=lambda t: (-t[0], t[2]))
            if groups is not None:
                seen, reps = set(), []
                for r in lst:
                    if groups[r[2]] not in seen:
                        seen.add(groups[r[2]])
                        reps.append(r)
                lst = reps
            self.rows[i] = (lst, [-r[0] for r in lst])

    def cut(self, thr: float, k: int) -> list:
        kept = []
        for lst, neg in self.rows.values():
            kept += lst[: min(k, bisect.bisect_right(neg, -thr))]
        return sorted(kept, key=lambda t: (-t[0], t[1], t[2]))

    def kth_tie(self, k: int) -> Optional[float]:
        """The score of some row's k-th record, preferably one whose (k + 1)-th record scores the same."""
        fallback = None
        for i in sorted(self.rows):
            lst = self.rows[i][0]
            if len(lst) > k and lst[k - 1][0] == lst[k][0] and lst[k][0] > 0.0:
                return lst[k][0]
            if len(lst) >= k and fallback is None and lst[k - 1][0] > 0.0:
                fallback = lst[k - 1][0]
        return fallback


def groups_of(g: ProbeGrid) -> np.ndarray:
    """Group ids of the right items for the grouped top-k calls: about a quarter as many groups as rows, arbitrary values."""
    rng = random.Random(len(g.right) * 31 + len(g.left))
    return np.array([rng.randrange(max(1, len(g.right) // 4)) * 3 - 5 for _ in g.right], dtype=np.int32)


# ------------------------------------------------------------------------------------------------------- generators
def _units(rng, n: int, alphabet: Sequence[int]) -> List[int]:
    return [rng.choice(alphabet) for _ in range(n)]


LETTERS = [ord(c) for c in "abcdefgh"]


def _edit_size(kind: str, length: int) -> int:
    return length // 2 if kind.endswith("half") else int(kind[3:])


def _edit(s: Sequence[int], kind: str, pos: int, fresh: int) -> List[int]:
    """One edit of ``size`` units at ``pos``: kind = "add1" | "add3" | "del1" | "del2" | "sub1" | "sub2" | "subhalf" (half
    of the string substituted: ratio_1 about 0.5, so that a family WITH later steps scores below the routing thresholds).  ``fresh``: a code
    unit that no string of the grid holds -- an added or substituted one never matches, so the LCS of every copy of a family
    is the same whatever the position."""
    s = list(s)
    size = _edit_size(kind, len(s))
    if kind.startswith("add"):
        return s[:pos] + [fresh] * size + s[pos:]
    if kind.startswith("del"):
        return s[:pos] + s[pos + size:]
    return s[:pos] + [fresh] * size + s[pos + size:]


def _one_edit(rng, s: Sequence[int], alphabet: Sequence[int], limit: int) -> List[int]:
    s = list(s)
    roll = rng.random()
    if not s or (roll < 0.34 and len(s) < limit):
        pos = rng.randint(0, len(s))
        return s[:pos] + [rng.choice(alphabet)] + s[pos:]
    pos = rng.randrange(len(s))
    return s[:pos] + ([] if roll < 0.67 else [rng.choice(alphabet)]) + s[pos + 1:]


def raw_indel(stride: int) -> ProbeGrid:
    """RAW strings of one stride.  Stride 64: 0 .. 64 units, empty strings and full rows on both sides (la + lb = 128, the
    last entry of the launcher's table of smallest LCS).  Wider strides: lengths at 65, 128, 129, 256, 257, 512 as far as the
    stride holds them, on both sides, among shorter strings.  A third of the right side is one-edit copies of left strings."""
    rng = random.Random(2100 + stride)
    alphabet = LETTERS[:6]
    edges = [64] if stride == 64 else [e for e in (65, 128, 129, 256, 257, 512) if e <= stride]

    def length():
        roll = rng.random()
        if roll < 0.08:
            return 0
        if roll < 0.2:
            return rng.choice(edges)
        if stride == 64:
            return rng.randint(1, 64) if roll < 0.6 else rng.randint(1, 12)
        return rng.randint(65, stride) if roll < 0.35 else rng.randint(1, 90)

    left = [_units(rng, length(), alphabet) for _ in range(80)]
    right = [_units(rng, length(), alphabet) for _ in range(N_RIGHT)]
    for k, e in enumerate(edges * 2):
        left[k], right[3 * k + 1] = _units(rng, e, alphabet), _units(rng, e, alphabet)
    left[len(edges) * 2], right[0] = [], []
    for k in range(2, N_RIGHT, 3):
        right[k] = _one_edit(rng, left[rng.randrange(len(left))], alphabet, stride)
    return ProbeGrid(f"raw_indel_{stride}", "indel", True, left, right, size=stride)


def raw_jaccard(width: int) -> ProbeGrid:
    """Rows of 0 .. ``width`` ids (no empty row on the left: empty against empty is the host's ZeroDivisionError), rows of
    exactly ``width`` on both sides, most rows small and over six ids, so that 1/2, 1/3, 2/3 are shared by hundreds of
    pairs; right rows that are subsets of a left row."""
    rng = random.Random(2200 + width)
    small, vocab = list(range(6)), list(range(2 * width))

    def row(allow_empty):
        roll = rng.random()
        if allow_empty and roll < 0.05:
            return []
        if roll < 0.6:
            return rng.sample(small, rng.randint(1, 3))
        if roll < 0.7:
            return rng.sample(vocab, width)
        return rng.sample(vocab, rng.randint(1, width))

    left = [row(False) for _ in range(80)]
    right = [row(True) for _ in range(N_RIGHT)]
    left[0], left[1], right[0], right[1] = (rng.sample(vocab, width) for _ in range(4))
    right[2] = []
    subset = []
    for k in range(3, N_RIGHT, 4):
        i = rng.randrange(len(left))
        right[k] = rng.sample(left[i], rng.randint(1, len(left[i])))
        subset.append((i, k))
    return ProbeGrid(f"raw_jaccard_{width}", "jaccard", True, left, right, size=width, subset=subset)


def _categories(rng, g: ProbeGrid, variant: str) -> ProbeGrid:
    """The grid with category masks: random small masks (empty ones among them); every planted right item carries its left
    source's mask, which is never empty, so that the planted pairs are visited in every variant."""
    if variant == "plain":
        return g
    cat_l = np.array([rng.choice([0, 1, 2, 3, 6]) for _ in g.left], dtype=np.uint64)
    cat_r = np.array([rng.choice([0, 1, 2, 4, 5]) for _ in g.right], dtype=np.uint64)
    for i, j in g.family_pairs() + g.subset:
        if cat_l[i] == 0:
            cat_l[i] = 3
    for i, j in g.family_pairs() + g.subset:
        cat_r[j] = cat_l[i]
    cat_r[g.duplicates] = 7  # (meets every left item that has a category at all)
    g.cat_l, g.cat_r = cat_l, cat_r
    g.mode = CAT_INTERSECT if variant == "cat1_partition" else CAT_INTERSECT_OR_BOTH_EMPTY
    g.partition = variant == "cat1_partition"
    g.name = f"{g.name}-{variant}"
    return g


def step1_level(item: Sequence) -> int:
    """The level step 1 compares: level 1, or the only level of a one-level item."""
    return min(1, len(item) - 1)


def _plant_fuzzy(rng, left, right, slots, sources, kinds, limit):
    """Tight families and anagram pairs of a fuzzy levels grid, written into ``right[slot]``.  ``sources``: left items of a
    depth other than 2 (at depth 2 the level of step 1 is also the level of step 2) whose step-1 string has room."""
    tight: Dict[str, List[Pair]] = {}
    slots = list(slots)
    fresh = 1 + max(u for it in left + right for lv in it for u in lv)
    for i, kind in zip(sources, kinds):
        src = left[i]
        lv = step1_level(src)
        s = src[lv]
        size = _edit_size(kind, len(s))
        assert len(src) != 2 and len(s) >= FAMILY_SIZE + size and (not kind.startswith("add") or len(s) + size <= limit)
        places = rng.sample(range(len(s) - size + 1), FAMILY_SIZE)
        fam = []
        for pos in places:
            j = slots.pop()
            right[j] = [list(x) if q != lv else _edit(s, kind, pos, fresh) for q, x in enumerate(src)]
            fam.append((i, j))
        tight[f"{kind}@left{i}"] = fam
    anagram = []
    deep = [i for i in range(len(left)) if len(left[i]) >= 3 and len(set(left[i][2])) > 2]
    for i in rng.sample(deep, min(2, len(deep))):
        j = slots.pop()
        twin = [list(x) for x in left[i]]
        twin[2] = twin[2][::-1] if twin[2][::-1] != twin[2] else twin[2][1:] + twin[2][:1]
        right[j] = twin
        anagram.append((i, j))
    return tight, anagram


KINDS = ("add1", "del1", "sub1", "add3", "del2", "subhalf")


def levels_indel_one_word(variant: str) -> ProbeGrid:
    """Suffix-nested items of 1 .. 6 levels, level strings of at most 64 code units (words over eight letters joined with
    blanks, the generator of the split-path test), tight families on eight left items and anagram pairs."""
    rng = random.Random(2300)
    words = [_units(rng, rng.randint(2, 5), LETTERS) for _ in range(40)]
    blank = ord(" ")

    def item(depth=None, extra=0):
        n = depth or rng.randint(1, 6)
        toks = [rng.choice(words) for _ in range(n + 1 + extra)]
        out = []
        for k in range(n):
            s: List[int] = []
            for w in sorted({tuple(t) for t in toks[: k + 2 + extra]}):
                s += ([blank] if s else []) + list(w)
            out.append(s[:63] if s[63:64] == [blank] else s[:64])
        return out

    left = [item(extra=rng.choice((0, 0, 6))) for _ in range(83)]
    right = [item(extra=rng.choice((0, 0, 6))) for _ in range(N_RIGHT)]
    sources = []
    for k, depth in enumerate((1, 3, 4, 5, 6, 3)):  # planted sources: step-1 strings of 24 .. 61 units
        while True:
            it = item(depth, extra=rng.choice((2, 4, 6)))
            if 24 <= len(it[step1_level(it)]) <= 61:
                break
        left[5 + 9 * k] = it
        sources.append(5 + 9 * k)
    for k in range(1, N_RIGHT, 9):  # loose near-copies: the last level changed
        src = [list(x) for x in left[rng.randrange(len(left))]]
        src[-1] = (src[-1] + [blank, LETTERS[0], LETTERS[0]])[:64]
        right[k] = src
    slots = rng.sample([k for k in range(N_RIGHT) if k % 9 != 1], len(sources) * FAMILY_SIZE + 2)
    tight, anagram = _plant_fuzzy(rng, left, right, slots, sources, KINDS, 64)
    g = ProbeGrid("levels_indel_one_word", "indel", False, left, right, size=64, tight=tight, anagram=anagram)
    return _categories(rng, g, variant)


TERM_SHAPES = {128: ((2, 4), (1, 3)), 256: ((3, 5), (2, 5)), 512: ((4, 8), (3, 6))}


def levels_indel_multi_word(stride: int, variant: str) -> ProbeGrid:
    """Term-shaped items (``synthetic.term_cohort`` / ``term_levels``, as the shared-tile test builds them) of one stride,
    with tight families; two of their sources have a step-1 string that fills the row, so that a substituted copy gives
    ``n1 = 2 * stride`` (1024 at stride 512: where the float rounding of the kernels' smallest-LCS bound is largest)."""
    from napkon_string_matching_amd import synthetic
    from napkon_string_matching_amd.compare import score_functions as sf

    rng = random.Random(2400 + stride)
    entries, words = TERM_SHAPES[stride]
    # (strides 256 and 512: part of either side has the short shape, as a real Term column mixes lengths)
    n_long = (72, N_RIGHT) if stride == 128 else (30, 90) if stride == 256 else (18, 56)
    short = TERM_SHAPES[128]
    a = synthetic.term_cohort(n_long[0], 2400 + stride, vocab=300, entries=entries, words=words)
    a += synthetic.term_cohort(72 - n_long[0], 2402 + stride, vocab=300, entries=short[0], words=short[1]) if n_long[0] < 72 else []
    b = synthetic.term_cohort(n_long[1], 2401 + stride, vocab=300, entries=entries, words=words, plant_from=a, plant_fraction=0.05)
    if n_long[1] < N_RIGHT:
        b += synthetic.term_cohort(N_RIGHT - n_long[1], 2403 + stride, vocab=300, entries=short[0], words=short[1], plant_from=a,
                                   plant_fraction=0.05)
    ops = lambda items: [[[ord(c) for c in sf.fuzzy_operand(lv)[:stride].strip()] for lv in it] for it in synthetic.term_levels(items)]
    left, right = ops(a), ops(b)
    pool = [u for it in left for lv in it for u in lv]

    def filled(n):  # text of exactly n units drawn from the cohort's own
        at = rng.randrange(len(pool) - n)
        s = pool[at: at + n]
        s[0] = s[-1] = LETTERS[0]  # (no blank at either end)
        return s

    deep = [i for i in range(len(left)) if len(left[i]) >= 3 and 24 <= len(left[i][1]) <= stride - 3]
    sources = deep[:4]
    full = [i for i in range(len(left)) if len(left[i]) >= 3 and i not in sources][:2]
    for i in full:
        left[i][1] = filled(stride)
    longest = max(len(lv) for it in left + right for lv in it)
    if not stride // 2 < longest:
        left[full[0]][2] = filled(stride)
    kinds = ("add1", "del1", "subhalf", "add3", "sub1", "del1")
    slots = rng.sample(range(1, N_RIGHT), 6 * FAMILY_SIZE + 2 + 23)
    duplicates = [0] + [slots.pop() for _ in range(23)]
    for j in duplicates[1:]:  # one right item 24 times over: every left item has a score that 24 pairs share
        right[j] = [list(lv) for lv in right[0]]
    tight, anagram = _plant_fuzzy(rng, left, right, slots, sources + full, kinds, stride)
    g = ProbeGrid(f"levels_indel_multi_word_{stride}", "indel", False, left, right, size=stride, tight=tight, anagram=anagram,
                  duplicates=duplicates)
    return _categories(rng, g, variant)


def _nested_item(rng, vocab: int, max_levels: int, max_new: int, first: int = 0) -> List[List[int]]:
    base: List[int] = []
    out = []
    for _ in range(rng.randint(1, max_levels)):
        for v in rng.sample(range(vocab), rng.randint(0 if base else 1, max_new)):
            if v not in base:
                base.append(v)
        out.append(list(base))
    return out


def levels_jaccard(variant: str) -> ProbeGrid:
    """Nested id sets (the generator of the random levels test).  Tight families: a right copy lacks one id of the level
    step 1 compares (and of level 0, which no step of a deeper item visits), or holds one more, taken from level 2 -- the
    nesting holds and every later level is identical.  Subset pairs: every level of the right item is a prefix of the left
    item's level."""
    rng = random.Random(2500)
    vocab = 40
    left = [_nested_item(rng, vocab, 6, 3) for _ in range(83)]
    right = [_nested_item(rng, vocab, 6, 3) for _ in range(N_RIGHT)]
    for k in range(1, N_RIGHT, 9):
        src = [list(lv) for lv in left[rng.randrange(len(left))]]
        right[k] = src[:-1] if k % 2 and len(src) > 1 else src
    free = [k for k in range(N_RIGHT) if k % 9 != 1]
    rng.shuffle(free)
    tight: Dict[str, List[Pair]] = {}
    # (depth, ids at level 0, at level 1, at level 2): level 1 grows by at least 12 ids over level 0, level 2 over level 1
    shapes = ((1, 13, 0, 0), (3, 1, 13, 14), (4, 2, 15, 13), (6, 3, 14, 12))
    for k, (depth, n0, n1, n2) in enumerate(shapes):
        ids = rng.sample(range(vocab), min(vocab, n0 + n1 + n2 + 2))
        cuts = [n0, n0 + n1, n0 + n1 + n2, n0 + n1 + n2 + 1, n0 + n1 + n2 + 1, n0 + n1 + n2 + 2]
        item = [ids[:c] for c in cuts[:depth]]
        i = 4 + 17 * k
        left[i] = item
        lv = step1_level(item)
        lo = n0 if depth > 1 else 0
        drop = []
        for x in item[lv][lo: lo + FAMILY_SIZE] if depth > 1 else item[0][:FAMILY_SIZE]:
            j = free.pop()
            right[j] = [[v for v in lvl if v != x] if q <= lv else list(lvl) for q, lvl in enumerate(item)]
            drop.append((i, j))
        tight[f"drop1@left{i}"] = drop
        if depth >= 3:
            add = []
            for y in item[2][len(item[1]): len(item[1]) + FAMILY_SIZE]:
                j = free.pop()
                right[j] = [list(lvl) + ([y] if q == 1 else []) for q, lvl in enumerate(item)]
                add.append((i, j))
            tight[f"add1@left{i}"] = add
    subset = []
    for _ in range(10):
        i = rng.randrange(len(left))
        j = free.pop()
        right[j] = [lvl[: (len(lvl) + 1) // 2] for lvl in left[i]]
        subset.append((i, j))
    widest = max(len(it[-1]) for it in left + right)
    g = ProbeGrid("levels_jaccard", "jaccard", False, left, right, size=16 if widest <= 16 else 32 if widest <= 32 else 64,
                  tight=tight, subset=subset)
    return _categories(rng, g, variant)


# ------------------------------------------------------------------------------------------------------- catalogue
RAW_INDEL = ["raw_indel_64", "raw_indel_128", "raw_indel_256", "raw_indel_512"]
RAW_JACCARD = ["raw_jaccard_16", "raw_jaccard_32", "raw_jaccard_64"]
ONE_WORD = [f"levels_indel_one_word-{v}" if v != "plain" else "levels_indel_one_word" for v in VARIANTS]
MULTI_WORD = [f"levels_indel_multi_word_{s}" + ("" if v == "plain" else f"-{v}") for s in (128, 256, 512) for v in VARIANTS]
LEVELS_JACCARD = [f"levels_jaccard-{v}" if v != "plain" else "levels_jaccard" for v in VARIANTS]
LEVELS = ONE_WORD + MULTI_WORD + LEVELS_JACCARD
EVERY = RAW_INDEL + RAW_JACCARD + LEVELS

_BUILT: Dict[str, ProbeGrid] = {}


def grid(name: str) -> ProbeGrid:
    if name not in _BUILT:
        base, _, variant = name.partition("-")
        variant = variant or "plain"
        if base.startswith("raw_indel_"):
            g = raw_indel(int(base.rsplit("_", 1)[1]))
        elif base.startswith("raw_jaccard_"):
            g = raw_jaccard(int(base.rsplit("_", 1)[1]))
        elif base == "levels_indel_one_word":
            g = levels_indel_one_word(variant)
        elif base.startswith("levels_indel_multi_word_"):
            g = levels_indel_multi_word(int(base.rsplit("_", 1)[1]), variant)
        elif base == "levels_jaccard":
            g = levels_jaccard(variant)
        else:
            raise KeyError(name)
        assert g.name == name, (g.name, name)
        _BUILT[name] = g
    return _BUILT[name]


def probes_of(g: ProbeGrid, cap: int = 40) -> List[float]:
    return probes(all_scores(g), cap, g.family_pairs())
