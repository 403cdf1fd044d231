"""Seam corpora of the bit-parallel LCS loops behind ``fuzzy_match``, built by construction, and a host model of the
loops' dispatch.  Shared by tests/test_cpu_lcs_seams.py (the corpora through the oracle alone: do they hold what they claim,
do they reach every instantiation?) and tests/test_gpu_lcs_seams.py (every Indel entry and route on every case).

A CASE is one (stride S = 64 K, pattern length P): ALL left strings of a case have exactly P code units.  Every loop picks
its specialisation from the wave's pattern length(s) -- ``words`` of wide_lcs, ``limbs`` of tile_lcs1_any / tile_lcs2_any,
``la_max`` of the dense passes, ``max(laA, laB)`` of the two-pattern passes --, so with one length on the whole left side the
instantiation depends on the case alone, whichever rows a kernel batches or pairs up.  The host model below restates those
rules; ``reached(stride)`` lists what the cases of a stride reach.

Left strings (7): a run, a 2- and a 4-letter pseudo-random string, a string whose matches all sit in its top 64-bit word, one
for the top 32-bit limb, one with unique markers at bits 31 / 32 of every limb (hence 63 / 64 of every word), and the pattern
of the last-lane late-match row, over letters no other row holds.  Right strings (<= 101: a full tile of 64 and a partial one) are
derived from them, and every family records the LCS it has by construction in ``grid.closed``.

Every grid is a ``threshold_probes.ProbeGrid``: ``all_scores``, ``expectation``, ``thresholds_around`` and the
``probe_tables`` helpers apply unchanged.
"""
import random
from typing import Dict, List, Tuple

from support import threshold_probes as tp

STRIDES = (64, 128, 256, 512)
LAYOUTS = ("step1", "step2_dense", "step2_sparse", "deep")
MAX_LEFT, MAX_RIGHT = 8, 64 + 37
CADENCES = (4, 8, 16)  # text units between two stop tests: raw_lcs_units, wide_lcs_words<EARLY>, tile_lcs2<EARLY>

A, B, C, D = (ord(c) for c in "abcd")
X, Y, Z = (ord(c) for c in "xyz")           # below / in the top word or limb; the foreign filler of padded rows
M_FILL, N_FILL = ord("m"), ord("n")         # the marker string's filler, and its partner's
LATE = [ord(c) for c in "pqrs"]             # the last-lane pattern's letters
JUNK = ord("#")
MARKER0 = 1000                              # markers: one code point per position
KEYS = [ord(c) for c in "ABCDEFG"]          # level-1 keys of the sparse layout, one per left string
WIDE0 = 5000                                # code points of the 255-symbol cases
CUT_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)  # prefixes and suffixes (and P - 1)
MOD16_LENGTHS = (10, 11, 12, 13)  # further prefixes: with the rest, texts of every residue mod 16 at every stride


def indel_score(la: int, lb: int, lcs: int) -> float:
    """``fuzzy_match`` from the LCS, in the doubles of csrc/indel_score.hpp (an empty string scores 0)."""
    if la == 0 or lb == 0:
        return 0.0
    n = la + lb
    return ((1.0 - float(n - 2 * lcs) / float(n)) * 100.0) / 100.0


# --------------------------------------------------------------------------------------------- host model of the dispatch
def wide_words(K: int, la: int) -> int:
    """csrc/indel_wide.hpp ``wide_lcs<K, EARLY>``: the W of the ``wide_lcs_words<K, W>`` it calls for a pattern of ``la``."""
    words = (la + 63) >> 6
    if words <= 1:
        return 1
    if K >= 2 and words == 2:
        return 2
    if K >= 4 and words == 3:
        return 3
    if K >= 4 and words == 4:
        return 4
    if K >= 8 and words <= 6:
        return 6
    return K


def wide2_words(K: int, la_max: int) -> int:
    """csrc/indel_wide.hpp ``wide_lcs2<K>`` (park kernel, two patterns per pass)."""
    return 1 if la_max <= 64 else min(K, 2)


def tile1_limbs(K: int, la_max: int) -> int:
    """csrc/indel_tile_lcs.hpp ``tile_lcs1_any<K>``: the L of the ``tile_lcs1<K, L>`` it calls."""
    limbs = (la_max + 31) >> 5
    if limbs <= 2:
        return 2
    if limbs in (3, 4):
        return limbs
    if K >= 4 and limbs in (5, 6):
        return limbs
    if K >= 4 and limbs <= 8:
        return 8
    if K >= 8 and limbs <= 12:
        return 12
    return 2 * K


def tile_two_patterns(la_a: int, la_b: int) -> bool:
    """csrc/indel_levels_tile.hpp, step 1 and the wave-wide later steps: two rows share a pass (``tile_lcs2_any``) while the
    longer pattern has at most 2 x 64 code units; beyond, one ``tile_lcs1_any`` pass per row."""
    return max(la_a, la_b) <= 128


def tile2_limbs(la_max: int) -> int:
    """csrc/indel_tile_lcs.hpp ``tile_lcs2_any<K, EARLY>`` (la_max <= 128)."""
    assert la_max <= 128
    return min(max((la_max + 31) >> 5, 2), 4)


def finish_sweep(la: int, lb: int) -> Tuple[str, str]:
    """csrc/indel_levels_finish.hpp ``lane_lcs``: the shorter string is the pattern (the left one on a tie), a 32-bit sweep
    when the pattern has at most 32 units.  (Wave-wide it is the LONGEST pattern of the wave that decides; with one length
    on the left side, ``min(P, lb)`` of a pair is what its own lane asks for.)"""
    return ("narrow" if min(la, lb) <= 32 else "wide", "left_is_pattern" if la <= lb else "right_is_pattern")


def raw_top_k_words(stride: int) -> int:
    """csrc/top_k_raw.hip: ``indel_top_k_kernel<W, ...>`` with W = stride / 64 (every word live whatever the pattern)."""
    return stride // 64


# --------------------------------------------------------------------------------------------------------------- cases
def pattern_lengths(stride: int) -> List[int]:
    limb_seams = {32 * m + d for m in range(1, 17) for d in (-1, 0, 1)}
    word_seams = {64 * w + d for w in range(1, 9) for d in (-1, 0, 1)}  # (a subset of the limb seams: do not prune)
    return sorted(p for p in {1, 2, 3, 4, 5} | limb_seams | word_seams if p <= stride)


def cases(stride: int) -> List[Tuple[int, bool]]:
    """(P, 255 symbols?) of a stride: every seam length, and the alphabet case (P = stride - 1: odd limb tail, top word)."""
    return [(p, False) for p in pattern_lengths(stride)] + [(stride - 1, True)]


def case_id(stride: int, p: int, alpha: bool) -> str:
    return f"{stride}_{p}" + ("_a255" if alpha else "")


CASE_IDS = {s: [case_id(s, p, a) for p, a in cases(s)] for s in STRIDES}


def seam_positions(p: int) -> List[int]:
    """Bits 31 and 32 of every limb boundary below ``p`` (every second one is bit 63 / 64 of a word), and the string's
    first and last position."""
    pos = {0, p - 1} | {q for limb in range(16) for q in (32 * limb + 31, 32 * limb + 32) if q < p}
    return sorted(pos)


def _late_lengths(stride: int, p: int) -> List[Tuple[int, int]]:
    """(m, T) of the late-match rows ``junk^(T - m) . suffix_m``, m around the cadences: T - m is a multiple of 16, so LCS so
    far + units left == m at a check point of every cadence (4, 8, 16 units), and from T - m on at every later one."""
    return sorted({(m, m + 16 * max(1, (p - m) // 16)) for m in (min(p, 5), min(p, 9), min(p, 17))})


def _last_lane(stride: int, p: int) -> Tuple[int, int]:
    """(m, T) of the late-match row on which a whole wave's verdict rests: as long as the stride (patterns of 16 units and
    more), so that at its last check points every other row of its tile -- none shares a letter with its pattern -- has
    fewer units left than it needs, and this lane alone keeps the scan going, with LCS so far + units left == need."""
    m = min(p, 17)
    return (m, stride) if m >= 16 else (m, m + 16 * ((stride - m) // 16))


def _strings(stride: int, p: int, alpha: bool, extra_symbols: int):
    """left, right, closed {(i, j): LCS}, late [(i, j, m)], source (right row -> the left string it was made from)."""
    rng = random.Random(7000 + stride * 1000 + p)
    top_w, top_l = p - 64 * ((p - 1) // 64), p - 32 * ((p - 1) // 32)  # units in the top word / limb
    marks = seam_positions(p)
    marker = [M_FILL] * p
    for k, q in enumerate(marks):
        marker[q] = MARKER0 + k
    two = [rng.choice((A, B)) for _ in range(p)]
    if alpha:  # distinct code points, as many as fit beside the rest (the fill rows below bring the total to 255)
        two = [WIDE0 + k % 180 for k in range(p)]
    left = [[A] * p, two, [rng.choice((A, B, C, D)) for _ in range(p)], [X] * (p - top_w) + [Y] * top_w,
            [X] * (p - top_l) + [Y] * top_l, marker, [rng.choice(LATE) for _ in range(p)]]
    RUN, TWO, FOUR, TOPW, TOPL, MARK, LATEP = range(7)
    right: List[List[int]] = []
    closed: Dict[Tuple[int, int], int] = {}
    late: List[Tuple[int, int, int]] = []
    source: List[int] = []

    def add(row, src, lcs=None, also=()):
        j = len(right)
        right.append(list(row))
        source.append(src)
        if lcs is not None:
            closed[(src, j)] = lcs
        for i, v in also:
            closed[(i, j)] = v
        return j

    for i, s in enumerate(left[:LATEP]):  # each left string itself (but the last-lane pattern: see _last_lane)
        add(s, i, p)
    cuts = [n for n in CUT_LENGTHS + MOD16_LENGTHS + (p - 1,) if 0 <= n <= p]
    for k, n in enumerate(sorted(set(cuts))):  # prefixes and suffixes, dealt over the run and the random strings
        src = (RUN, TWO, FOUR)[k % 3]
        add(left[src][:n], src, n)
        if n and n not in MOD16_LENGTHS:
            add(left[(src + 1) % 3][p - n:], (src + 1) % 3, n)
    for k, t in enumerate(sorted({t for t in (p + 1, p + 2, p + 3, stride - 1, stride) if p < t <= stride})):
        src = (FOUR, TWO)[k % 2]  # the left string inside a foreign filler: texts of every residue mod 4, longer than P
        cut = (k * 7) % (p + 1)
        add(left[src][:cut] + [Z] * (t - p) + left[src][cut:], src, p)
    for t in sorted({t for t in (1, p - 1, p, p + 1, stride) if 1 <= t <= stride}):
        add([A] * t, RUN, min(p, t))  # against a^P the addition carries through every word at every step
    for k, t in enumerate(sorted({t for t in (1, top_l, top_l + 1, top_w, top_w + 1, stride) if 1 <= t <= stride})):
        # every match in the last word / limb (the rows belong to the two strings in turn: the sparse layout's families)
        add([Y] * t, (TOPL, TOPW)[k % 2], also=[(TOPW, min(t, top_w)), (TOPL, min(t, top_l))])
    other = [N_FILL] * p
    for q in marks:
        other[q] = marker[q]
    add(other, MARK, len(marks))  # matches in place at the seam bits only
    if p < stride:
        add([N_FILL] * (stride - p) + other, MARK, len(marks))
    for m, t in _late_lengths(stride, p):
        late.append((FOUR, add([JUNK] * (t - m) + left[FOUR][p - m:], FOUR, m), m))
    m, t = _last_lane(stride, p)
    late.append((LATEP, add([JUNK] * (t - m) + left[LATEP][p - m:], LATEP, m), m))
    if alpha:  # fill rows of fresh symbols: 255 in all, the pad code right behind the last one
        used = {u for s in left + right for u in s}
        fresh = 255 - len(used) - extra_symbols
        assert fresh > 0
        nxt = WIDE0 + 1000
        while fresh > 0:
            n = min(fresh, stride)
            add(list(range(nxt, nxt + n)), TWO)
            nxt += n
            fresh -= n
    assert len(left) <= MAX_LEFT and len(right) <= MAX_RIGHT, (stride, p, len(right))
    return left, right, closed, late, source


def _finish(g: tp.ProbeGrid, stride, p, alpha, closed, late, source) -> tp.ProbeGrid:
    g.stride, g.pattern, g.alpha = stride, p, alpha
    g.closed, g.late, g.source = closed, late, source
    return g


_BUILT: Dict[str, tp.ProbeGrid] = {}


def raw_case(stride: int, p: int, alpha: bool = False) -> tp.ProbeGrid:
    name = "seam_raw_" + case_id(stride, p, alpha)
    if name not in _BUILT:
        left, right, closed, late, source = _strings(stride, p, alpha, 0)
        _BUILT[name] = _finish(tp.ProbeGrid(name, "indel", True, left, right, size=stride), stride, p, alpha, closed, late, source)
    return _BUILT[name]


def levels_case(stride: int, p: int, alpha: bool, layout: str) -> tp.ProbeGrid:
    """The strings of the RAW case as level strings of items.

    * ``step1``: depth 1 -- the seam string is what step 1 scores (scan loops, EARLY two-pattern loop of the tile kernel).
    * ``step2_dense``: depth 3, ``[x, key, seam]`` with ONE key: every pair outlives step 1, the later steps run wave-wide.
    * ``step2_sparse``: the same with a key per left string; a right item carries the key of the left string it was made
      from, so a row keeps a handful of survivors: they are parked and scored by the lane-per-pair dense pass.
    * ``deep``: depth 5, ``[x, key, key, key, seam]``: deeper than the tile kernel's resident images, the seam step reads its
      text from global memory (the generic full-limb pass, text stride 1).
    """
    name = f"seam_{layout}_" + case_id(stride, p, alpha)
    if name in _BUILT:
        return _BUILT[name]
    n_keys = {"step1": 0, "step2_dense": 1, "step2_sparse": len(KEYS), "deep": 1}[layout]
    left, right, closed, late, source = _strings(stride, p, alpha, n_keys + (1 if n_keys else 0))
    key = lambda k: [KEYS[k % n_keys]] * 6
    head = [ord("X")]
    if layout == "step1":
        wrap = lambda s, k: [s]
    elif layout == "deep":
        wrap = lambda s, k: [head, key(0), key(0), key(0), s]
    else:
        wrap = lambda s, k: [head, key(k), s]
    g = tp.ProbeGrid(name, "indel", False, [wrap(s, i) for i, s in enumerate(left)], [wrap(s, source[j]) for j, s in enumerate(right)],
                     size=stride)
    g.layout = layout
    _BUILT[name] = _finish(g, stride, p, alpha, closed, late, source)
    return _BUILT[name]


def level_score(g: tp.ProbeGrid, i: int, j: int, lcs: int) -> float:
    """The score of pair (i, j) of a levels layout whose seam strings have the LCS ``lcs``: step s = 1 .. depth compares
    level min(s, depth - 1) and weighs 2^-s, so the last level counts twice in an item of more than one level; the key steps
    compare equal or disjoint keys (ratio 1 or 0)."""
    ratio = indel_score(g.pattern, len(g.right[j][-1]), lcs)
    same = g.layout != "step2_sparse" or g.source[j] == i
    steps = {"step1": [ratio], "step2_dense": [1.0, ratio, ratio], "step2_sparse": [1.0 if same else 0.0, ratio, ratio],
             "deep": [1.0, 1.0, 1.0, ratio, ratio]}[g.layout]
    score, factor = 0.0, 1.0
    for r in steps:
        factor /= 2
        score += r * factor
    return score


PROBE_CAP = 5  # (the whole GPU file runs with every later pull request: every probe costs three thresholds on every route)


def probe_scores(g: tp.ProbeGrid, cap: int = PROBE_CAP) -> List[float]:
    """At most ``cap`` positive oracle scores to cut at, in this order: the late-match pairs' (at most 4: never dropped), the
    self pairs', the run pairs'."""
    at = {(i, j): s for s, i, j in tp.all_scores(g)}
    first = [at[(i, j)] for i, j, _ in g.late]
    first += [at[(i, i)] for i in range(len(g.left) - 1)]  # right row i is left string i
    first += [at[p] for p in sorted(g.closed) if p[0] == 0 and g.source[p[1]] == 0]
    out: List[float] = []
    for s in first:
        if s > 0.0 and s not in out and len(out) < cap:
            out.append(s)
    return out


_THRESHOLDS: Dict[str, List[float]] = {}


def thresholds(g: tp.ProbeGrid) -> List[float]:
    """0.0, 1.0, and every probe score with one ulp to either side (cached per grid)."""
    if g.name not in _THRESHOLDS:
        _THRESHOLDS[g.name] = sorted({0.0, 1.0} | set(tp.thresholds_around(probe_scores(g))))
    return _THRESHOLDS[g.name]


# ---------------------------------------------------------------------------------------------- what the cases reach
def reached(stride: int) -> Dict[str, set]:
    """Per loop the instantiations that the cases of ``stride`` reach, with the pattern length that reaches each:
    ``wide_lcs`` {(K, W, P)}, ``wide_lcs2`` {(K, W, P)}, ``tile_lcs1`` {(K, L, P)}, ``tile_lcs2`` {(L, P)},
    ``finish`` {(sweep, roles)} (stride 64 only: the split path is the one-word kernels'), ``raw_top_k`` {(W, lb % 16)}."""
    K = stride // 64
    out = {k: set() for k in ("wide_lcs", "wide_lcs2", "tile_lcs1", "tile_lcs2", "finish", "raw_top_k")}
    for p, alpha in cases(stride):
        g = raw_case(stride, p, alpha)
        out["wide_lcs"].add((K, wide_words(K, p), p))
        out["tile_lcs1"].add((K, tile1_limbs(K, p), p))
        if tile_two_patterns(p, p):
            out["tile_lcs2"].add((tile2_limbs(p), p))
            out["wide_lcs2"].add((K, wide2_words(K, p), p))
        for row in g.right:
            if row:
                out["raw_top_k"].add((raw_top_k_words(stride), len(row) % 16))
                if stride == 64:
                    out["finish"].add(finish_sweep(p, len(row)))
    return out
