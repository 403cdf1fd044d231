"""Seeded operand grids for the two general kernels of csrc/any_grids.hip (``nsm_indel_any_grid``,
``nsm_jaccard_any_grid``), shared by tests/test_gpu_any_grids.py (kernel against oracle) and
tests/test_cpu_any_operands.py (the same grids through the oracle alone: are they worth running?).

A grid holds plain ints: code units of level strings (fuzzy) or token ids of level sets (Jaccard), item -> level -> ints.
The oracle takes them as they are (sets without repeats), the kernel side gets ``chr(BASE + v)`` strings / the int tokens.
Every generator is deterministic: its own ``random.Random(seed)``, nothing drawn from global state.
"""
import math
import random
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

BASE = 0x4E00  # code unit v is chr(BASE + v) on the kernel side: letters, no surrogates up to BASE + 1023
CAT_NONE, CAT_INTERSECT, CAT_INTERSECT_OR_BOTH_EMPTY = 0, 1, 2
DEPTHS = (1, 2, 3, 8, 63, 64, 65, 100, 300)
PATTERN_EDGES = (127, 128, 129, 255, 256, 257)  # chunk seams of the left string (128 code units per chunk)
TEXT_EDGES = (31, 32, 33, 63, 64, 65)           # carry words of the right string (32 positions per word)
LONG_EDGES = (4095, 4096)                       # the cap
ABOVE_ONE = 1.25


@dataclass
class Grid:
    name: str
    kind: str  # "indel" | "jaccard"
    left: List[List[List[int]]]
    right: List[List[List[int]]]
    mids: Tuple[float, ...] = (0.5,)  # middle thresholds: some pairs hit, some do not
    raw: bool = False
    cat_l: Optional[np.ndarray] = None
    cat_r: Optional[np.ndarray] = None
    mode: int = CAT_NONE
    probe: bool = False            # thresholds at exact oracle scores (and one ulp above) are added
    layout: Optional[str] = None   # Jaccard: the layout wide.jaccard_any_grid must choose
    mixed_depths: bool = False     # a hit pair of unequal depths and one with a side deeper than 64 are required
    long_strings: bool = False     # a hit pair with a left string > 128 units and one with a right string > 32 are required

    @property
    def pairs(self) -> int:
        return len(self.left) * len(self.right)


# ----------------------------------------------------------------------------------------------- two faces of a grid
def kernel_operands(g: Grid):
    """What wide.indel_any_grid / wide.jaccard_any_grid take: level strings, or the token lists as they are."""
    if g.kind == "jaccard":
        return g.left, g.right
    text = lambda items: [["".join(chr(BASE + v) for v in lv) for lv in it] for it in items]
    return text(g.left), text(g.right)


def _oracle_items(g: Grid, items):
    if g.kind == "jaccard":
        return [[sorted(set(lv)) for lv in it] for it in items]
    return items


_ALL: Dict[str, list] = {}


def oracle_all(g: Grid) -> list:
    """The oracle's hit list at threshold 0.0: every pair the category masks allow, in the canonical order.  A ratio is
    never negative, so this is every score of the grid; ``oracle_at`` cuts it at a threshold exactly as the oracle's own
    ``score >= thr`` does (tests/test_cpu_any_operands.py checks that against a second oracle call)."""
    if g.name not in _ALL:
        _ALL[g.name] = oracle_call(g, 0.0)
    return _ALL[g.name]


def oracle_call(g: Grid, thr: float) -> list:
    from oracle import native

    left, right = _oracle_items(g, g.left), _oracle_items(g, g.right)
    if g.raw:
        assert g.mode == CAT_NONE and all(len(it) == 1 for it in left + right)
        fn = native.indel_raw if g.kind == "indel" else native.jaccard_raw
        return fn(native.csr([it[0] for it in left]), native.csr([it[0] for it in right]), thr, cap=g.pairs + 1)
    return native.levels(g.kind == "indel", left, right, thr, g.cat_l, g.cat_r, g.mode, cap=g.pairs + 1)


def oracle_at(all_hits: Sequence[tuple], thr: float) -> list:
    return [h for h in all_hits if h[0] >= thr]


def probe_scores(all_hits: Sequence[tuple]) -> List[float]:
    """Distinct oracle scores to put a threshold on: the lowest positive one, the quartiles, the highest below 1.0 and the
    highest of all."""
    distinct = sorted({h[0] for h in all_hits if h[0] > 0.0})
    if not distinct:
        return []
    below_one = [s for s in distinct if s < 1.0]
    picks = {distinct[0], distinct[len(distinct) // 4], distinct[len(distinct) // 2], distinct[(3 * len(distinct)) // 4], distinct[-1]}
    if below_one:
        picks.add(below_one[-1])
    return sorted(picks)


def near_neighbours(all_hits: Sequence[tuple], s: float, slack: float = 1e-9) -> int:
    """Pairs scoring strictly between ``s - slack`` and ``s``: the ones a pruning bound with a wrong slack would confuse."""
    return sum(1 for h in all_hits if s - slack < h[0] < s)


def thresholds(g: Grid, all_hits: Sequence[tuple]) -> List[float]:
    out = [0.0, *g.mids, ABOVE_ONE]
    if g.probe:
        for s in probe_scores(all_hits):
            out += [s, math.nextafter(s, 2.0)]
    return out


def rows_per_chunk(n_left: int, n_right: int) -> int:
    """The launcher's geometry (csrc/any_grids.hip): 64 right items per tile, about 4096 blocks in all."""
    n_tiles = (n_right + 63) // 64
    chunks = (4096 + n_tiles - 1) // n_tiles
    return max(1, (n_left + chunks - 1) // chunks)


# ----------------------------------------------------------------------------------------------------- string helpers
def _units(rng, n: int, alphabet: int) -> List[int]:
    return [rng.randrange(alphabet) for _ in range(n)]


def _changed(s: Sequence[int], pos: int, alphabet: int) -> List[int]:
    t = list(s)
    t[pos] = (t[pos] + 1) % alphabet if alphabet > 1 else t[pos]
    return t


def _short(rng, alphabet: int, hi: int = 90) -> List[int]:
    return [] if rng.random() < 0.1 else _units(rng, rng.randint(0, hi), alphabet)


def _masks(rng, n: int, bits=(0, 1, 5, 40, 62, 63), zero: float = 0.25) -> np.ndarray:
    out = np.zeros(n, dtype=np.uint64)
    for k in range(n):
        if rng.random() >= zero:
            for _ in range(rng.randint(1, 3)):
                out[k] |= np.uint64(1) << np.uint64(rng.choice(bits))
    return out


# ------------------------------------------------------------------------------------------- (a) fuzzy, length edges
def fuzzy_length_edges(raw: bool) -> Grid:
    """Level strings of exactly the lengths where the chunked bit-parallel LCS changes shape, on both sides, in one wave
    with short and empty strings; near-duplicates of a 4096-unit and a 257-unit left string with one unit changed at
    position 0, at both sides of the first chunk seam, at the end, and one unit deleted before the seam."""
    rng = random.Random(1101 if raw else 1100)
    alphabet = 12

    def item(main, depth=None):
        """``main`` at a level that is visited (level 0 of a deeper item never is), short strings around it."""
        if raw:
            return [main], 0
        depth = depth or rng.randint(1, 4)
        levels = [_short(rng, alphabet) for _ in range(depth)]
        at = rng.randrange(1, depth) if depth > 1 else 0
        levels[at] = main
        return levels, at

    def with_main(src, new_main):
        levels, at = src
        return [list(lv) if k != at else new_main for k, lv in enumerate(levels)], at

    edges = PATTERN_EDGES + TEXT_EDGES
    left = [item(_units(rng, n, alphabet)) for n in edges] + [item(_short(rng, alphabet)) for _ in range(10)]
    right = [item(_units(rng, n, alphabet)) for n in edges] + [item(_short(rng, alphabet)) for _ in range(36)]
    long_base = item(_units(rng, 4096, alphabet), 4)  # (four levels: a copy can score up to 1 - 2^-4)
    mid_base = item(_units(rng, 257, alphabet), 4)
    left += [long_base, mid_base, item(_units(rng, 4095, alphabet)), item([])]
    right += [item(_units(rng, 4095, alphabet)), item(_units(rng, 4096, alphabet)), item([])]
    for base in (long_base, mid_base):
        s = base[0][base[1]]
        for pos in (0, 127, 128, len(s) - 1):
            right.append(with_main(base, _changed(s, pos, alphabet)))
        right.append(with_main(base, s[:126] + s[127:]))  # every later chunk of the pattern is shifted by one
        right.append(with_main(base, list(s)))
    # both roles: near-duplicates of a right string on the left (pattern = the copy)
    s = right[len(PATTERN_EDGES) - 1][0][right[len(PATTERN_EDGES) - 1][1]]  # the 257-unit right string
    left.append(with_main(right[len(PATTERN_EDGES) - 1], _changed(s, 128, alphabet)))
    left.append(with_main(right[len(PATTERN_EDGES) - 1], s[:127] + s[128:]))
    rng.shuffle(left)
    rng.shuffle(right)
    return Grid("fuzzy_length_edges_raw" if raw else "fuzzy_length_edges", "indel", [it for it, _ in left], [it for it, _ in right],
                mids=(0.3, 0.6, 0.9), raw=raw, probe=True, long_strings=True)


# ------------------------------------------------------------------------------------------------ (b) fuzzy, alphabets
def fuzzy_alphabet(alphabet: int) -> Grid:
    """Exactly ``alphabet`` distinct code units in the grid (a left string that is a permutation of all of them)."""
    rng = random.Random(1200 + alphabet)
    hi = 300 if alphabet == 1 else 160
    level = lambda: _units(rng, rng.choice((0, 1, 31, 32, 33, 128, 129, rng.randint(1, hi), rng.randint(1, hi))), alphabet)
    item = lambda: [level() for _ in range(rng.randint(1, 3))]
    left = [item() for _ in range(18)]
    right = [item() for _ in range(70)]
    everything = list(range(alphabet))
    rng.shuffle(everything)
    left[0] = [_short(rng, alphabet, 20), everything]
    left[1] = [_units(rng, 2 * alphabet + 130, alphabet)]
    for k in range(0, len(right), 4):  # near-duplicates: a few units changed or dropped
        src = [list(lv) for lv in left[rng.randrange(len(left))]]
        for lv in src:
            for _ in range(rng.randint(0, 3)):
                if lv:
                    pos = rng.randrange(len(lv))
                    lv[pos:pos + 1] = [] if rng.random() < 0.5 else [rng.randrange(alphabet)]
        right[k] = src
    left[2] = [_units(rng, rng.randint(1, hi), alphabet) for _ in range(4)]  # four levels and an exact copy: 1 - 2^-4
    right[1] = [list(lv) for lv in left[2]]
    return Grid(f"fuzzy_alphabet_{alphabet}", "indel", left, right, mids=(0.3, 0.6, 0.9), probe=alphabet == 1, long_strings=True)


# --------------------------------------------------------------------------------------------------------- (d) depths
def _deep_strings(rng, depth: int, alphabet: int) -> List[List[int]]:
    """Level strings that change a little from level to level (as the reference's suffix levels do)."""
    s = _units(rng, rng.randint(3, 12), alphabet)
    out = []
    for _ in range(depth):
        roll = rng.random()
        if roll < 0.3 and len(s) < 20:
            s = s + [rng.randrange(alphabet)]
        elif roll < 0.5 and s:
            s = _changed(s, rng.randrange(len(s)), alphabet)
        out.append(list(s))
    return out


def _recut(rng, item: List[List[int]], depths=DEPTHS) -> List[List[int]]:
    """The same levels at another depth: cut, or the last level repeated."""
    depth = rng.choice([d for d in depths if d != len(item)])
    return [list(lv) for lv in (item[:depth] if depth <= len(item) else item + [item[-1]] * (depth - len(item)))]


def fuzzy_depths() -> Grid:
    rng = random.Random(1400)
    alphabet = 6
    left = [_deep_strings(rng, d, alphabet) for d in DEPTHS for _ in range(2)]
    right = [_deep_strings(rng, DEPTHS[k % len(DEPTHS)], alphabet) for k in range(54)]
    for k in range(0, 54, 3):
        right[k] = _recut(rng, left[rng.randrange(len(left))])
    for src in (left[-1], left[-3], left[10]):  # depth 300, 100, 64: copies that differ only far down (scores within 1e-9)
        for at in (31, 40, 50):
            twin = [list(lv) for lv in src]
            for lv in range(min(at, len(twin) - 1), len(twin)):
                twin[lv] = twin[lv] + [0]
            right.append(twin)
        right.append([list(lv) for lv in src])
    right.append([list(left[-1][0])])  # depth 1 against depth 300
    left.append([list(right[0][-1])])
    rng.shuffle(right)
    return Grid("fuzzy_depths", "indel", left, right[:64] + right[64:], mids=(0.3, 0.5, 0.8), probe=True, mixed_depths=True)


def _nested_item(rng, depth: int, vocab: int, max_new: int = 2, start: int = 3) -> List[List[int]]:
    base = rng.sample(range(vocab), start)
    out = []
    for _ in range(depth):
        out.append(list(base))
        for v in rng.sample(range(vocab), rng.randint(0, max_new)):
            if v not in base:
                base.append(v)
    return out


def jaccard_depths(deep: bool) -> Grid:
    """Nested items of mixed depths.  ``deep``: depths up to 300, which forces the independent layout; else at most 64
    levels, where the nested layout (one merge per pair, histogram of first common steps) must be taken."""
    rng = random.Random(1410 if deep else 1411)
    depths = DEPTHS if deep else tuple(d for d in DEPTHS if d <= 64)
    vocab = 420 if deep else 120
    left = [_nested_item(rng, d, vocab) for d in depths for _ in range(2)]
    right = [_nested_item(rng, depths[k % len(depths)], vocab) for k in range(60)]
    for k in range(0, 60, 3):
        right[k] = _recut(rng, left[rng.randrange(len(left))], depths)
    deepest = left[-1]
    right.append([list(lv) for lv in deepest])
    right.append([list(lv) for lv in deepest[:40]] + [lv + [vocab + 1] for lv in deepest[40:]])  # differs from level 40 on
    right.append([list(deepest[0])])  # depth 1 against the deepest
    left.append([list(right[1][-1])])
    rng.shuffle(right)
    return Grid("jaccard_depths_deep" if deep else "jaccard_depths_64", "jaccard", left, right, mids=(0.2, 0.5, 0.8), probe=True,
                layout="independent" if deep else "nested", mixed_depths=deep)


# ------------------------------------------------------------------------------------------ (e) Jaccard, nested layout
ENTRY_LEVELS = (0, 1, 2, 63)


def _entering(rng, enter: int, depth: int, shared: Sequence[int], private_from: int, n_private: int) -> List[List[int]]:
    """A nested item of ``depth`` levels in which the ``shared`` ids come in at level ``enter`` and ``n_private`` ids of its
    own at levels all over."""
    at = {v: enter for v in shared}
    for k in range(n_private):
        at[private_from + k] = rng.randrange(depth)
    return [[v for v, lv in at.items() if lv <= level] for level in range(depth)]


def jaccard_nested() -> Grid:
    rng = random.Random(1500)
    shared = list(range(10))
    left, right = [], []
    nxt = 1000
    for side in (left, right):
        for enter in ENTRY_LEVELS:
            for depth in sorted({max(enter + 1, 2) if enter else 1, 64}):  # (enter 0: once as the only level, once under 63 more)
                n_private = rng.randint(1, 6) if enter or depth > 1 else 2
                it = _entering(rng, enter, depth, shared, nxt, n_private)
                if not it[0]:
                    it = [lv + [nxt + 50] for lv in it]  # (no empty level: the oracle refuses 0 / 0)
                side.append(it)
                nxt += 100
    n_combo = len(left)
    # wide items (65 .. 3000 ids) against small ones (1 .. 40), nested over 1 .. 4 levels
    vocab = 6000

    def grown(total: int, depth: int) -> List[List[int]]:
        ids = rng.sample(range(2000, 2000 + vocab), total)
        cuts = sorted(rng.randint(1, total) for _ in range(depth - 1)) + [total]
        return [ids[:c] for c in cuts]

    for total in (65, 66, 200, 1000, 3000, 2999):
        left.append(grown(total, rng.randint(1, 4)))
    for _ in range(8):
        left.append(grown(rng.randint(1, 40), rng.randint(1, 4)))
    for _ in range(48):
        right.append(grown(rng.randint(1, 40), rng.randint(1, 4)))
    big = left[n_combo + 4]  # 3000 ids
    right.append([lv[:-3] for lv in big])                       # a wide near-duplicate (subset at every level: the size bound is exact)
    right.append([list(lv) for lv in big])
    right.append([lv[: max(1, len(lv) // 2)] for lv in left[n_combo + 3]])
    right.append([lv[:30] for lv in left[n_combo + 2]][:1])     # small subset of a wide item, one level
    left.append([lv + lv[:3] + lv[:1] for lv in right[n_combo + 2]])  # repeated tokens inside a level count once
    right.append([lv + lv[-2:] for lv in left[n_combo + 1]])
    order = list(range(len(right)))
    rng.shuffle(order)
    return Grid("jaccard_nested", "jaccard", left, [right[k] for k in order], mids=(0.1, 0.4, 0.8), probe=True, layout="nested")


def entry_level_pairs(g: Grid):
    """(p, q) for every pair of ``jaccard_nested`` in which some id comes in at level p on the left and q on the right."""
    def first_levels(it):
        seen = {}
        for lv, level in enumerate(it):
            for v in level:
                seen.setdefault(v, lv)
        return seen

    found = set()
    for a in g.left:
        fa = first_levels(a)
        if len(fa) > 64:
            continue
        for b in g.right:
            fb = first_levels(b)
            if len(fb) > 64:
                continue
            found |= {(fa[v], fb[v]) for v in fa.keys() & fb.keys()}
    return found


def jaccard_cap_pair():
    """One item of exactly 65535 ids over three nested levels, against itself and against a copy with one id fewer, and
    the scores ``compare_terms`` x ``intersection_vs_union`` gives them, from the sizes, in the reference's operation
    order.  (The C oracle's intersection is quadratic: it is not run on this pair.)"""
    ids = list(range(7, 7 + 65535))
    cuts = (30000, 50000, 65535)
    item = [ids[:c] for c in cuts]
    fewer = [lv[1:] for lv in item]  # id 7 is gone from every level
    want = []
    for j, other in enumerate((item, fewer)):
        score, factor = 0.0, 1.0
        for s in range(1, 4):
            a, b = set(item[min(s, 2)]), set(other[min(s, 2)])
            factor /= 2
            score += (len(a & b) / len(a | b)) * factor
        want.append((score, 0, j))
    want.sort(key=lambda h: (-h[0], h[1], h[2]))
    return [item], [item, fewer], want


# ------------------------------------------------------------------------------------- (f) Jaccard, independent layout
def jaccard_independent() -> Grid:
    """Levels that are not suffix-nested (a level drops a token of the one before), empty levels on the right only, more
    than 64 levels, wide levels (65+ ids) at some steps and tiny ones at others."""
    rng = random.Random(1600)
    vocab = 260

    def item(depth: int, allow_empty: bool) -> List[List[int]]:
        out = []
        prev: List[int] = []
        for _ in range(depth):
            roll = rng.random()
            if allow_empty and roll < 0.12:
                cur: List[int] = []
            elif roll < 0.3:
                cur = rng.sample(range(vocab), rng.randint(65, 150))
            elif roll < 0.6 and len(prev) > 1:
                cur = prev[1:] + [rng.randrange(vocab)]  # drops a token of the level before
            else:
                cur = rng.sample(range(vocab), rng.randint(1, 4))
            out.append(cur)
            prev = cur
        return out

    depths = (1, 2, 3, 4, 6, 70)
    left = [item(depths[k % len(depths)], False) for k in range(20)]
    right = [item(depths[(k * 5) % len(depths)], True) for k in range(66)]
    for k in range(0, 66, 4):
        src = left[rng.randrange(len(left))]
        right[k] = [list(lv) if rng.random() < 0.7 else lv[: max(1, len(lv) - 2)] for lv in src]
    right[1] = [lv[: max(1, len(lv) // 2)] for lv in left[5]]  # a subset at every level: the size bound is exact
    return Grid("jaccard_independent", "jaccard", left, right, mids=(0.1, 0.4, 0.8), probe=True, layout="independent")


def jaccard_raw_wide() -> Grid:
    """RAW quotient of single sets: 65 .. 400 ids against 1 .. 40."""
    rng = random.Random(1610)
    vocab = 900
    size = lambda wide: rng.randint(65, 400) if wide else rng.randint(1, 40)
    left = [[rng.sample(range(vocab), size(k % 3 == 0))] for k in range(24)]
    right = [[rng.sample(range(vocab), size(k % 9 == 0))] for k in range(70)]
    for k in range(0, 70, 5):
        src = left[rng.randrange(len(left))][0]
        right[k] = [src[: max(1, len(src) - rng.randint(0, 4))] + [vocab + k]]
    right[2] = [list(left[0][0]) + left[0][0][:2]]
    return Grid("jaccard_raw_wide", "jaccard", left, right, mids=(0.1, 0.4, 0.8), raw=True, probe=True, layout="nested")


# ------------------------------------------------------------------------------------------------------- (g) geometry
RIGHT_TAILS = (1, 63, 64, 65, 129)


def _small_fuzzy_item(rng, alphabet: int = 5) -> List[List[int]]:
    return [_units(rng, rng.randint(0, 10), alphabet) for _ in range(rng.randint(1, 3))]


def _small_set_item(rng, vocab: int = 30) -> List[List[int]]:
    return _nested_item(rng, rng.randint(1, 3), vocab, max_new=2, start=rng.randint(1, 3))


def tails(kind: str, n_right: int) -> Grid:
    rng = random.Random(1700 + (0 if kind == "indel" else 1))  # (the same pool for every n_right: a prefix of it)
    make = _small_fuzzy_item if kind == "indel" else _small_set_item
    left = [make(rng) for _ in range(12)]
    right = [make(rng) for _ in range(max(RIGHT_TAILS))]
    for k in (0, 62, 63, 64, 128):  # the last lane of every tail holds a copy of a left item
        right[k] = [list(lv) for lv in left[(k * 7) % 12]]
    return Grid(f"tails_{kind}_{n_right}", kind, left, right[:n_right], mids=(0.5,), layout="nested" if kind == "jaccard" else None)


ROWS_LEFT, ROWS_RIGHT = 9001, 70


def many_rows(kind: str) -> Grid:
    """So many left items that a block of the general kernels walks several rows, the last block fewer."""
    rng = random.Random(1710 + (0 if kind == "indel" else 1))
    make = _small_fuzzy_item if kind == "indel" else _small_set_item
    left = [make(rng) for _ in range(ROWS_LEFT)]
    right = [make(rng) for _ in range(ROWS_RIGHT)]
    for k in range(0, ROWS_RIGHT, 6):
        right[k] = [list(lv) for lv in left[rng.randrange(ROWS_LEFT)]]
    while len(left[-1]) < 2 or not all(left[-1]):  # (a copy of it scores at least 0.75)
        left[-1] = make(rng)
    right[5] = [list(lv) for lv in left[-1]]  # the single row of the last block
    return Grid(f"many_rows_{kind}", kind, left, right, mids=(0.5, 0.8), layout="nested" if kind == "jaccard" else None)


# -------------------------------------------------------------------------------- (h) categories and zero-level items
def with_categories(kind: str, mode: int) -> Grid:
    rng = random.Random(1800 + 10 * mode + (0 if kind == "indel" else 1 if kind == "jaccard" else 2))
    if kind == "indel":
        make = lambda: _deep_strings(rng, rng.choice((1, 2, 3, 8)), 5)
        layout = None
    elif kind == "jaccard":
        make = lambda: _nested_item(rng, rng.choice((1, 2, 3, 8)), 40)
        layout = "nested"
    else:
        make = lambda: [rng.sample(range(40), rng.randint(1, 6)) for _ in range(rng.choice((1, 2, 3, 70)))]
        layout = "independent"
    left = [make() for _ in range(30)]
    right = [make() for _ in range(80)]
    cat_l, cat_r = _masks(rng, 30), _masks(rng, 80)
    top = np.uint64(1) << np.uint64(63)
    for k in range(0, 80, 3):
        src = rng.randrange(30)
        right[k] = [list(lv) for lv in left[src]]
        if k % 2 == 0:  # every other copy meets its source through bit 63 alone; the rest are left to chance
            cat_l[src] |= top
            cat_r[k] = top
    name = {"indel": "indel", "jaccard": "jaccard_nested", "independent": "jaccard_independent"}[kind]
    return Grid(f"categories_{name}_mode{mode}", "indel" if kind == "indel" else "jaccard", left, right, mids=(0.3, 0.6),
                cat_l=cat_l, cat_r=cat_r, mode=mode, layout=layout)


def zero_levels_only(kind: str, mode: int) -> Grid:
    """Every item without levels: each allowed pair scores 0.0 (a hit at threshold 0.0 and at no positive one)."""
    rng = random.Random(1900 + mode)
    cats = (None, None) if mode == CAT_NONE else (_masks(rng, 5), _masks(rng, 70))
    return Grid(f"zero_levels_only_{kind}_mode{mode}", kind, [[] for _ in range(5)], [[] for _ in range(70)], mids=(1e-300, 0.5),
                cat_l=cats[0], cat_r=cats[1], mode=mode, layout="nested" if kind == "jaccard" else None)


def zero_levels_apart(kind: str, mode: int) -> Grid:
    """Zero-level items and items with levels in one grid, kept apart by their masks (bit 5 is the zero-level items'
    alone): a visited mixed pair would be the reference's IndexError, which is the host's to raise."""
    rng = random.Random(1910 + mode + (0 if kind == "indel" else 5))
    make = _small_fuzzy_item if kind == "indel" else _small_set_item
    bits = (0, 1, 40, 63)

    def side(n):
        items, cat = [], np.zeros(n, dtype=np.uint64)
        for k in range(n):
            if rng.random() < 0.3:
                items.append([])
                cat[k] = np.uint64(1) << np.uint64(5)
            else:
                items.append(make(rng))
                cat[k] = _masks(rng, 1, bits, zero=0.0)[0]
        return items, cat

    left, cat_l = side(20)
    right, cat_r = side(75)
    return Grid(f"zero_levels_apart_{kind}_mode{mode}", kind, left, right, mids=(1e-300, 0.5), cat_l=cat_l, cat_r=cat_r, mode=mode,
                layout="nested" if kind == "jaccard" else None)


# ---------------------------------------------------------------------------------------------------------- the lists
def _catalogue():
    entries = [
        ("fuzzy_length_edges", fuzzy_length_edges, (False,)),
        ("fuzzy_length_edges_raw", fuzzy_length_edges, (True,)),
        *[(f"fuzzy_alphabet_{a}", fuzzy_alphabet, (a,)) for a in (1, 255, 256, 1023)],
        ("fuzzy_depths", fuzzy_depths, ()),
        ("jaccard_depths_deep", jaccard_depths, (True,)),
        ("jaccard_depths_64", jaccard_depths, (False,)),
        ("jaccard_nested", jaccard_nested, ()),
        ("jaccard_independent", jaccard_independent, ()),
        ("jaccard_raw_wide", jaccard_raw_wide, ()),
        *[(f"tails_{k}_{n}", tails, (k, n)) for k in ("indel", "jaccard") for n in RIGHT_TAILS],
        ("many_rows_indel", many_rows, ("indel",)),
        ("many_rows_jaccard", many_rows, ("jaccard",)),
        *[(f"categories_{n}_mode{m}", with_categories, (k, m))
          for k, n in (("indel", "indel"), ("jaccard", "jaccard_nested"), ("independent", "jaccard_independent")) for m in (1, 2)],
        *[(f"zero_levels_apart_{k}_mode{m}", zero_levels_apart, (k, m)) for k in ("indel", "jaccard") for m in (1, 2)],
    ]
    return {name: (make, args) for name, make, args in entries}


CATALOGUE = _catalogue()
# grids whose every allowed pair scores 0.0: no middle threshold can split them, they are checked on their own
ZERO_ONLY = {f"zero_levels_only_{k}_mode{m}": (zero_levels_only, (k, m)) for k in ("indel", "jaccard") for m in (0, 1, 2)}
_BUILT: Dict[str, Grid] = {}


def grid(name: str) -> Grid:
    if name not in _BUILT:
        make, args = {**CATALOGUE, **ZERO_ONLY}[name]
        _BUILT[name] = make(*args)
        assert _BUILT[name].name == name, (_BUILT[name].name, name)
    return _BUILT[name]
