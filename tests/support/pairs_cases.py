"""Seam cases of the listed-pairs kernels (csrc/pairs.hip), built by construction, shared by tests/test_gpu_pairs.py (the
kernels against the oracle) and tests/test_cpu_pairs.py (the same grids through the oracle alone: do they hold what they
claim?).  Every grid is a ``threshold_probes.ProbeGrid``, so the oracle helpers of that module apply (``all_scores`` caches
by name); all N x M pairs of a grid are scored.

One wavefront scores one pair: the shorter string is the pattern, 64 code units per word, the carry of the bit-parallel
LCS travels from word to word; a set's ids sit one per lane.  Hence:

* string lengths 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512 on either side, each at the stride it forces;
* a string against itself (LCS = length); two strings that share only the units at bits 63 / 64 of every word; a run of
  one symbol against a longer run (every word all ones: the carry chain over all K words);
* sets of 0, 1 and W ids, disjoint, equal, nested, overlapping;
* levels items of depths 1, 2, 3 and 6 on both sides (Ll != Lr both ways), and -- widths 32 and 64 -- up to 64 levels on
  one side against 1 on the other.
"""
import random
from typing import List

from support import threshold_probes as tp

PAIR_COUNTS = (1, 63, 64, 65, 259)  # (259: not a multiple of the 4 pairs a block of 4 wavefronts takes per round)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)
STRIDES = (64, 128, 256, 512)
A, B, E = tp.LETTERS[0], tp.LETTERS[1], tp.LETTERS[4]


def straddle_positions(stride: int) -> List[int]:
    """Bits 63 and 64 of every word boundary a row of ``stride`` units has (and bit 63 of the last word)."""
    return [p for w in range(stride // 64) for p in (64 * w + 63, 64 * w + 64) if p < stride]


def indel_seams(stride: int) -> tp.ProbeGrid:
    """RAW strings: one random string of every seam length up to ``stride`` on both sides (the longest ones force the
    stride), the left strings again on the right (``self_pairs``), the straddle pair and the two runs."""
    rng = random.Random(3100 + stride)
    lengths = [n for n in LENGTHS if n <= stride]
    alphabet = tp.LETTERS[:4]
    left = [[rng.choice(alphabet) for _ in range(n)] for n in lengths]
    right = [[rng.choice(alphabet) for _ in range(n)] for n in lengths]
    g = tp.ProbeGrid(f"pairs_indel_seams_{stride}", "indel", True, left, right, size=stride)
    g.self_pairs = [(k, len(right) + k) for k in range(len(left))]
    right += [list(s) for s in left]
    pos = straddle_positions(stride)
    mine, other = [B] * stride, [E] * stride
    for k, p in enumerate(pos):
        mine[p] = other[p] = 1000 + k  # (one symbol per position: they can only match in place)
    g.straddle = (len(left), len(right), len(pos))  # (i, j, LCS)
    left.append(mine)
    right.append(other)
    g.runs = [(len(left), len(right), stride - 1), (len(left) + 1, len(right) + 1, stride - 1)]  # (i, j, LCS)
    left += [[A] * (stride - 1), [A] * stride]
    right += [[A] * stride, [A] * (stride - 1)]
    return g


def jaccard_seams(width: int) -> tp.ProbeGrid:
    """RAW sets of 0, 1 and ``width`` ids: equal, disjoint, nested, half overlapping.  No empty set on the left (empty
    against empty is the oracle's ZeroDivisionError; the GPU file scores that pair on its own)."""
    w = width
    left = [[0], list(range(w)), list(range(w, 2 * w)), list(range(w // 2)), [w - 1], list(range(w - 1, -1, -1))]
    right = [[], [0], list(range(w)), list(range(w, 2 * w)), list(range(w // 2)), list(range(w // 2, w // 2 + w)), [5 * w],
             list(range(1, w))]
    return tp.ProbeGrid(f"pairs_jaccard_seams_{width}", "jaccard", True, left, right, size=width)


def _nested(rng, depth: int, vocab: int, most: int) -> List[List[int]]:
    ids = rng.sample(range(vocab), rng.randint(1, 3))
    out = [list(ids)]
    for _ in range(depth - 1):
        for v in rng.sample(range(vocab), rng.randint(0, 2)):
            if v not in ids and len(ids) < most:
                ids.append(v)
        out.append(list(ids))
    return out


DEPTHS = (1, 2, 3, 6)


def levels_seams(kind: str) -> tp.ProbeGrid:
    """Items of depths 1, 2, 3 and 6, three of each, on both sides: every (Ll, Lr) combination, L = 1 included."""
    rng = random.Random(3300 + len(kind))
    if kind == "jaccard":
        side = lambda: [_nested(rng, d, 12, 16) for d in DEPTHS for _ in range(3)]
        return tp.ProbeGrid("pairs_levels_seams_jaccard", "jaccard", False, side(), side(), size=16)
    item = lambda d: [[rng.choice(tp.LETTERS[:3]) for _ in range(rng.choice((0, 1, 5, 63, 64)))] for _ in range(d)]
    side = lambda: [item(d) for d in DEPTHS for _ in range(3)]
    return tp.ProbeGrid("pairs_levels_seams_indel", "indel", False, side(), side(), size=64)


def levels_jaccard_wide(width: int) -> tp.ProbeGrid:
    """40 x 40 nested items of up to ``width`` ids and 1 .. 64 levels: 64 levels on one side meet 1 on the other."""
    rng = random.Random(3400 + width)
    depth = lambda: rng.choice((1, 1, 2, 3, 6, 17, 64))
    left = [_nested(rng, depth(), 2 * width, width) for _ in range(40)]
    right = [_nested(rng, depth(), 2 * width, width) for _ in range(40)]
    left[0], right[0] = _nested(rng, 64, 2 * width, width), _nested(rng, 1, 2 * width, width)
    left[1], right[1] = _nested(rng, 1, 2 * width, width), _nested(rng, 64, 2 * width, width)
    # (an item that fills the row: the width the encoder must choose)
    left[2] = [list(range(k + 1)) for k in range(0, width, max(1, width // 16))] + [list(range(width))]
    return tp.ProbeGrid(f"pairs_levels_jaccard_{width}", "jaccard", False, left, right, size=width)


_BUILT = {}


def grid(name: str) -> tp.ProbeGrid:
    if name not in _BUILT:
        kind, _, arg = name.rpartition("_")
        make = {"pairs_indel_seams": lambda: indel_seams(int(arg)), "pairs_jaccard_seams": lambda: jaccard_seams(int(arg)),
                "pairs_levels_seams": lambda: levels_seams(arg), "pairs_levels_jaccard": lambda: levels_jaccard_wide(int(arg))}
        _BUILT[name] = make[kind]()
        assert _BUILT[name].name == name
    return _BUILT[name]


INDEL_SEAMS = [f"pairs_indel_seams_{s}" for s in STRIDES]
JACCARD_SEAMS = [f"pairs_jaccard_seams_{w}" for w in (16, 32, 64)]
LEVELS_SEAMS = ["pairs_levels_seams_indel", "pairs_levels_seams_jaccard"]
LEVELS_JACCARD_WIDE = ["pairs_levels_jaccard_32", "pairs_levels_jaccard_64"]
EVERY = INDEL_SEAMS + JACCARD_SEAMS + LEVELS_SEAMS + LEVELS_JACCARD_WIDE


# -------------------------------------------------------------------------------------- plain-Python scores of one pair
def lcs(a, b) -> int:
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0
        for y in range(1, len(b) + 1):
            up = row[y]
            row[y] = diag + 1 if x == b[y - 1] else max(up, row[y - 1])
            diag = up
    return row[len(b)]


def indel_ratio(a, b) -> float:
    if not a or not b:
        return 0.0
    n = len(a) + len(b)
    return ((1.0 - (n - 2 * lcs(a, b)) / n) * 100.0) / 100.0


def jaccard(a, b) -> float:
    return len(set(a) & set(b)) / len(set(a) | set(b))


def pair_score(g: tp.ProbeGrid, i: int, j: int) -> float:
    """The score of pair (i, j) of a plain grid (no categories), recomputed in plain Python."""
    part = indel_ratio if g.kind == "indel" else jaccard
    a, b = g.left[i], g.right[j]
    if g.raw:
        return part(a, b)
    score, factor = 0.0, 1.0
    for s in range(1, max(len(a), len(b)) + 1):
        factor /= 2
        score += part(a[min(s, len(a) - 1)], b[min(s, len(b) - 1)]) * factor
    return score
