"""The yardstick of the token-set measures beside Jaccard (tests/test_cpu_set_measures.py, tests/test_gpu_set_measures.py):
the three definitions in plain Python, their zero-division predicates, and the inputs the GPU tests use -- built here so
that the CPU tests can check them (every threshold has a pair exactly on it and one below it)."""
import math
from contextlib import contextmanager

VOCAB = [f"t{k}" for k in range(24)]
NAMES = {"mean": "intersection_vs_mean", "smaller": "intersection_vs_smaller", "left": "intersection_vs_left"}
MEASURES = tuple(NAMES)


def _sets(left, right):
    split = lambda v: frozenset(v if isinstance(v, list) else v.split())
    return split(left), split(right)


# ------------------------------------------------------------------------------------------------------- definitions
def intersection_vs_mean(left, right) -> float:
    """Sorensen-Dice: 2 |A n B| / (|A| + |B|)."""
    a, b = _sets(left, right)
    return 2 * len(a & b) / (len(a) + len(b))


def intersection_vs_smaller(left, right) -> float:
    """Overlap (Szymkiewicz-Simpson) coefficient: |A n B| / min(|A|, |B|)."""
    a, b = _sets(left, right)
    return len(a & b) / min(len(a), len(b))


def intersection_vs_left(left, right) -> float:
    """Containment of left in right: |A n B| / |A|."""
    a, b = _sets(left, right)
    return len(a & b) / len(a)


def intersection_vs_union(left, right) -> float:
    a, b = _sets(left, right)
    return len(a & b) / len(a | b)


DEFINITIONS = {"mean": intersection_vs_mean, "smaller": intersection_vs_smaller, "left": intersection_vs_left,
               "union": intersection_vs_union}
# does the definition raise ZeroDivisionError for sets of a and b tokens?
DIVIDES_BY_ZERO = {"mean": lambda a, b: a + b == 0, "smaller": lambda a, b: min(a, b) == 0, "left": lambda a, b: a == 0,
                   "union": lambda a, b: a + b == 0}


@contextmanager
def registered(monkeypatch):
    """The definitions under their plug-in names in the oracle's registry (``oracle.score_functions.get`` reads it)."""
    from oracle import score_functions as osf

    for measure, name in NAMES.items():
        monkeypatch.setitem(osf.SCORE_FUNCTIONS, name, DEFINITIONS[measure])
    yield


# ------------------------------------------------------------------------------------------------------------ RAW grids
RAW_THRESHOLDS = (0.5, 2 / 3, 1.0)


def thresholds_with_next(base):
    return tuple(t for b in base for t in (b, math.nextafter(b, 2.0)))


def window(start: int, size: int):
    return [VOCAB[(start + q) % len(VOCAB)] for q in range(size)]


def raw_grid(measure: str, width: int = 16):
    """(left rows, right rows) of token lists for tables of ``width``.  Width 16: every size 1..16 on both sides as prefixes
    and as sliding windows (so every intersection size occurs), 37 left rows (not a multiple of the 8 rows a wavefront
    owns), 70 right rows of size 4 (more than one 64-lane batch in a class), and an empty right row where the measure
    divides by nothing it brings (mean, left).  Widths 32 / 64: a smaller grid with the sizes only that width holds."""
    if width == 16:
        left = [window(0, n) for n in range(1, 17)] + [window(3 + n, n) for n in range(1, 17)] + \
               [window(20, 2), window(9, 1), window(6, 3), window(1, 2), window(13, 4)]
        right = [window(0, n) for n in range(1, 17)] + [window(2 * n, n) for n in range(1, 17)]
        fours = []
        for q in range(200):
            row = sorted({VOCAB[q % 24], VOCAB[(q + 1) % 24], VOCAB[(5 * q + 3) % 24], VOCAB[(7 * q + 11) % 24]})
            if len(row) == 4 and len(fours) < 70:
                fours.append(row)
        assert len(fours) == 70
        right += fours
    else:
        lo = width // 2 + 1
        vocab = [f"t{k}" for k in range(width + 8)]
        win = lambda s, n: [vocab[(s + q) % len(vocab)] for q in range(n)]
        left = [win(0, n) for n in range(lo, width + 1, 3)] + [win(5, n) for n in (1, 2, 7, lo, width)] + [win(0, 4), win(0, 3)]
        right = [win(0, n) for n in range(lo, width + 1, 2)] + [win(3, n) for n in (1, 2, 4, 8, lo + 1, width)] + \
                [win(width // 2, n) for n in (lo, width - 1)] + [win(1, lo)]  # (win(0, 3) has 2 of its 3 tokens in win(1, lo))
    if measure in ("mean", "left"):
        right = right + [[]]
    return left, right


def raw_hits(measure: str, left, right, threshold: float):
    """The definition's records ``(score, i, j)`` with score >= threshold, canonical order."""
    f = DEFINITIONS[measure]
    hits = [(f(a, b), i, j) for i, a in enumerate(left) for j, b in enumerate(right)]
    return sorted((h for h in hits if h[0] >= threshold), key=lambda h: (-h[0], h[1], h[2]))


# ---------------------------------------------------------------------------------------------------------- levels grids
LEVELS_THRESHOLDS = (0.5, 0.75)


def nested(*sizes, start: int = 0):
    """A suffix-nested item: level l is the window of sizes[l] tokens from ``start`` (sizes non-decreasing)."""
    return [window(start, n) for n in sizes]


def levels_grid(measure: str):
    """(left items, right items): 1..4 suffix-nested levels, different level counts on the two sides, one-level items, and
    (mean, left: on the right side only) an item whose first two levels are empty."""
    left = [nested(2), nested(4), nested(1, 2), nested(2, 4), nested(1, 3, 6), nested(2, 2, 4, 8), nested(1, 2, 4, 8),
            nested(3, start=1), nested(2, 4, start=2), nested(1, 2, 3, start=4), nested(4, 8, 12, 16), nested(2, 6, start=10),
            nested(1, 1, 2, 4, start=1)]
    right = [nested(2), nested(4), nested(2, 4), nested(1, 2, 4), nested(2, 4, 8), nested(1, 2, 4, 8), nested(4, 4, 8, 8),
             nested(3, start=1), nested(2, 4, start=2), nested(2, 3, start=4), nested(8, 16), nested(6, start=10),
             nested(1, 4, start=1), nested(2, 2, start=0), nested(1, 2, 2, 4), nested(3, 6, 12, start=1), nested(4, 8, start=0)]
    if measure in ("mean", "left"):
        right = right + [nested(0, 0, 2)]
    return left, right


def levels_categories(n_left: int, n_right: int):
    """uint64 category masks with empty ones on both sides (the "both empty" rule of the second category mode)."""
    import numpy as np

    cl = np.array([0 if k % 5 == 0 else (1 << (k % 3)) | (1 << ((k // 2) % 4)) for k in range(n_left)], dtype=np.uint64)
    cr = np.array([0 if k % 4 == 0 else (1 << (k % 4)) for k in range(n_right)], dtype=np.uint64)
    return cl, cr


def category_match(cl: int, cr: int, mode: int) -> bool:
    return bool(cl & cr) or (mode == 2 and cl == 0 and cr == 0)


def levels_hits(measure: str, left, right, threshold: float, keep=lambda i, j: True, f=None):
    """``oracle.compare.compare_terms`` with the definition as score_func over the pairs ``keep`` admits: the records
    ``(score, i, j)`` with score >= threshold, canonical order."""
    from oracle.compare import compare_terms

    f = f or DEFINITIONS[measure]
    hits = [(compare_terms(a, b, f), i, j) for i, a in enumerate(left) for j, b in enumerate(right) if keep(i, j)]
    return sorted((h for h in hits if h[0] >= threshold), key=lambda h: (-h[0], h[1], h[2]))
