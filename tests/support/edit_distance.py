"""The yardstick of the Levenshtein score functions (tests/test_cpu_edit_distance.py, tests/test_gpu_edit_distance.py): a
two-row dynamic programme for the distance d and the occurrence distance w, the two definitions in plain Python over the
oracle's ``join_sorted`` / ``default_process``, host restatements of what the kernels compute beside the score (the
word-wise column update, the greatest distance that still reaches a threshold, the histogram bound), and the inputs the
GPU tests use -- built here so that the CPU tests can check them (every threshold has a pair exactly on it and one below)."""
import math
import random
from contextlib import contextmanager

import numpy as np

from oracle.score_functions import default_process, join_sorted

NAMES = {"edit": "levenshtein_match", "edit_within": "levenshtein_within"}
METRICS = tuple(NAMES)
CODES = {"indel": 0, "edit": 1, "edit_within": 2}
SEAMS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)  # pattern lengths around the 64-bit word boundaries
STRIDES = (64, 128, 256, 512)


# ---------------------------------------------------------------------------------------------------------------- the DP
def _dp(a: str, b: str, within: bool):
    """Two rows of the edit-distance table, rows along ``b``: row t holds d(a[:p], b[..t]) for p = 0..la.  ``within``: an
    occurrence may start anywhere in ``b`` (row value 0 at p = 0) and end anywhere (the minimum over the rows' last cells)."""
    la = len(a)
    prev = list(range(la + 1))
    best = prev[la]
    for cb in b:
        cur = [0 if within else prev[0] + 1]
        for p in range(1, la + 1):
            cur.append(min(prev[p] + 1, cur[p - 1] + 1, prev[p - 1] + (a[p - 1] != cb)))
        prev = cur
        best = min(best, prev[la])
    return prev[la], best


def distance(a: str, b: str) -> int:
    """Unit-cost Levenshtein distance d(a, b)."""
    return _dp(a, b, False)[0]


def within(a: str, b: str) -> int:
    """w(a, b): the least d(a, s) over the substrings s of b, the empty one included (Sellers); 0 <= w <= len(a)."""
    return _dp(a, b, True)[1]


def _dp_fast(a: str, b: str, is_within: bool) -> int:
    """The same two-row programme with numpy rows (the GPU tests' long strings): the row's own dependency
    cur[p] = min(cur[p], cur[p - 1] + 1) is a running minimum of cur[p] - p.  Checked against ``_dp`` on the CPU."""
    la = len(a)
    av = np.frombuffer(a.encode("utf-32-le"), dtype=np.uint32)
    ramp = np.arange(la + 1, dtype=np.int64)
    prev = ramp.copy()
    best = int(prev[la])
    for cb in b:
        cur = np.empty(la + 1, dtype=np.int64)
        cur[0] = 0 if is_within else prev[0] + 1
        np.minimum(prev[1:] + 1, prev[:-1] + (av != ord(cb)), out=cur[1:])
        cur = np.minimum.accumulate(cur - ramp) + ramp
        prev = cur
        best = min(best, int(prev[la]))
    return best if is_within else int(prev[la])


def _units(s) -> np.ndarray:
    return np.frombuffer(s.encode("utf-32-le"), dtype=np.uint32).astype(np.int64) if isinstance(s, str) \
        else np.asarray(s, dtype=np.int64).reshape(-1)


def both_all(lefts, rights, chunk: int = 8):
    """(d, w): int64 [len(lefts)][len(rights)] arrays of d(a, b) and w(a, b), each pair's two distances from ONE pass of
    the two-row programme.  The rows of the distance and of the occurrence distance are stacked, a step along the texts
    serves every b and ``chunk`` patterns at once (numpy), a b shorter than the longest simply stops taking part, and a
    pattern shorter than its chunk's longest is padded with a unit that matches nothing (cell p of a row depends on the
    cells up to p alone, so the pattern's own last cell is unharmed).  Strings: str or sequences of ints.  Checked
    against ``_dp`` on the CPU."""
    m = len(rights)
    lens = np.array([len(b) for b in rights], dtype=np.int64)
    order = np.argsort(-lens, kind="stable")  # longest first: the texts still taking part at step t are a prefix
    longest = int(lens.max(initial=0))
    text = np.full((m, longest), -1, dtype=np.int64)
    for r, k in enumerate(order.tolist()):
        text[r, : len(rights[k])] = _units(rights[k])
    sorted_lens = lens[order]
    taking_part = [int(np.searchsorted(-sorted_lens, -t, side="left")) for t in range(longest)]  # texts with len > t
    steps = np.arange(longest + 1)[:, None, None]
    d_all, w_all = np.empty((len(lefts), m), dtype=np.int64), np.empty((len(lefts), m), dtype=np.int64)
    by_length = np.argsort([len(a) for a in lefts], kind="stable")
    for c0 in range(0, len(lefts), chunk):
        ids = by_length[c0: c0 + chunk]
        las = np.array([len(lefts[k]) for k in ids], dtype=np.int64)
        c, width = len(ids), int(las.max())
        pattern = np.full((c, width), -2, dtype=np.int64)
        for r, k in enumerate(ids.tolist()):
            pattern[r, : las[r]] = _units(lefts[k])
        rows = np.arange(c)
        # rows shifted by their position, q[p] = row[p] - p (so q starts as zeros): the row's own dependency is then a plain
        # running minimum, and q[p] = min(q_prev[p] + 1, q_prev[p - 1] + (a[p - 1] != b[t]) - 1)
        q = np.zeros((2, c, m, width + 1), dtype=np.int16)
        last = np.zeros((longest + 1, c, 2, m), dtype=np.int16)  # the pattern's last cell of either table after every step
        for t in range(longest):
            n = taking_part[t]
            prev = q[:, :, :n]
            cur = np.empty_like(prev)
            cur[0, :, :, 0], cur[1, :, :, 0] = t + 1, 0
            step = (pattern[:, None, :] != text[None, :n, t, None]).astype(np.int16) - 1
            np.add(prev[..., 1:], 1, out=cur[..., 1:])
            np.minimum(cur[..., 1:], prev[..., :-1] + step[None], out=cur[..., 1:])
            np.minimum.accumulate(cur, axis=3, out=prev)
            last[t + 1] = q[:, rows, :, las]
        cells = last.astype(np.int64) + las[None, :, None, None]  # row[la] = q[la] + la; a finished text keeps its value
        d_sorted = cells[sorted_lens[None, :], rows[:, None], 0, np.arange(m)[None, :]]
        w_sorted = np.where(steps <= sorted_lens[None, None, :], cells[:, :, 1, :], las[None, :, None]).min(axis=0)
        for r, k in enumerate(ids.tolist()):  # (step 0 of w: the empty occurrence)
            d_all[k, order], w_all[k, order] = d_sorted[r], w_sorted[r]
    return d_all, w_all


def both_many(a, rights):
    """(d(a, b), w(a, b)) of one pattern and every b of ``rights``, as lists: ``both_all`` of one pattern."""
    d, w = both_all([a], rights)
    return d[0].tolist(), w[0].tolist()


def distance_table(lefts, texts, known=None) -> dict:
    """``{(a, b): (d, w)}`` for every a of ``lefts`` and b of ``texts`` (hashable strings: str or tuples of code units),
    added to ``known``: one ``both_all`` call.  The one place the yardsticks of the GPU files build their cache from."""
    known = {} if known is None else known
    lefts, texts = list(lefts), list(texts)
    if lefts and texts:
        d, w = both_all(lefts, texts)
        for r, a in enumerate(lefts):
            known.update({(a, b): dw for b, dw in zip(texts, zip(d[r].tolist(), w[r].tolist()))})
    return known


def plain_score(metric: str, la: int, lb: int, d: int, w: int) -> float:
    """The definition on strings as they are (the C entries take prepared strings): ``score`` of the metric's own distance."""
    return score(metric, la, lb, d if metric == "edit" else w)


def prepared(value) -> str:
    """What both score functions feed to the distance for one operand: ``fuzzy_match``'s preparation."""
    return default_process(join_sorted(value) if isinstance(value, list) else value)


def score(metric: str, la: int, lb: int, x: int) -> float:
    """The score of prepared strings of la and lb code units at distance / occurrence distance x."""
    if la == 0 or lb == 0:
        return 0.0
    return 1.0 - x / (max(la, lb) if metric == "edit" else la)


def _definition(metric: str, left, right, dp) -> float:
    a, b = prepared(left), prepared(right)
    if not a or not b:
        return 0.0
    return score(metric, len(a), len(b), dp(a, b, metric == "edit_within"))


def levenshtein_match(left, right) -> float:
    """``1 - d(a, b) / max(la, lb)``; 0.0 when either prepared string is empty."""
    return _definition("edit", left, right, lambda a, b, w: distance(a, b))


def levenshtein_within(left, right) -> float:
    """``1 - w(a, b) / la``; 0.0 when either prepared string is empty."""
    return _definition("edit_within", left, right, lambda a, b, w: within(a, b))


DEFINITIONS = {"edit": levenshtein_match, "edit_within": levenshtein_within}
# the same definitions over the numpy rows, for grids of long strings
FAST = {"edit": lambda l, r: _definition("edit", l, r, _dp_fast), "edit_within": lambda l, r: _definition("edit_within", l, r, _dp_fast)}


@contextmanager
def registered(monkeypatch, fast: bool = False):
    """The definitions under their plug-in names in the oracle's registry (``oracle.score_functions.get`` reads it)."""
    from oracle import score_functions as osf

    for metric, name in NAMES.items():
        monkeypatch.setitem(osf.SCORE_FUNCTIONS, name, (FAST if fast else DEFINITIONS)[metric])
    yield


# ------------------------------------------------------------------------------------------- what the kernels restate
M64 = (1 << 64) - 1


def column(a: str, b: str, top: int) -> int:
    """The bit-vector column update of csrc/edit_distance.hpp, word by word with explicit carries: d(a, b) for top = 1,
    w(a, b) for top = 0.  ``a`` is the pattern."""
    la = len(a)
    words = max(1, (la + 63) // 64)
    pm = {}
    for p, ch in enumerate(a):
        pm.setdefault(ch, [0] * words)[p // 64] |= 1 << (p % 64)
    vp, vn = [M64] * words, [0] * words
    value = best = la
    last_word, last_bit = (la - 1) // 64, (la - 1) % 64
    for ch in b:
        m = pm.get(ch, [0] * words)
        carry, hp_in, hn_in = 0, top, 0
        for w in range(words):
            total = vp[w] + (m[w] & vp[w]) + carry
            carry, total = total >> 64, total & M64
            d0 = (total ^ vp[w]) | m[w] | vn[w]
            hp = (vn[w] | ~(d0 | vp[w])) & M64
            hn = d0 & vp[w]
            if la and w == last_word:
                value += ((hp >> last_bit) & 1) - ((hn >> last_bit) & 1)
            hps, hns = ((hp << 1) | hp_in) & M64, ((hn << 1) | hn_in) & M64
            hp_in, hn_in = hp >> 63, hn >> 63
            vp[w] = (hns | ~(d0 | hps)) & M64
            vn[w] = hps & d0
        best = min(best, value)
    return value if top else best


def most_start(metric: str, la: int, lb: int, eff: float) -> int:
    """Where ``edit_most`` (csrc/edit_distance.hpp) starts its walk down: one above floor((1 - eff) den), clamped."""
    den = max(la, lb) if metric == "edit" else la
    if eff <= 0.0:
        return den
    return int(max(-1.0, min(math.floor((1.0 - eff) * den) + 1.0, float(den))))


def most(metric: str, la: int, lb: int, eff: float, start_offset: int = 0) -> int:
    """``edit_most``: the greatest x with score(x) >= eff (la, lb >= 1), -1 when none.  ``start_offset``: a mutation."""
    x = most_start(metric, la, lb, eff) + (start_offset if eff > 0.0 else 0)
    while x >= 0 and score(metric, la, lb, x) < eff:
        x -= 1
    return x


def hist32(s: str, code_of) -> list:
    """The table's 32-bucket histogram column: bucket code & 31, counts saturating at 255."""
    h = [0] * 32
    for ch in s:
        h[code_of[ch] & 31] = min(255, h[code_of[ch] & 31] + 1)
    return h


def sad(h1, h2) -> int:
    return sum(abs(x - y) for x, y in zip(h1, h2))


# ---------------------------------------------------------------------------------------------------------- RAW corpora
ALPHABET = "abcdefghijklmnopqrstuvwxyz0123456789"  # 36 symbols: four buckets of the histogram hold two each
RAW_THRESHOLDS = {"edit": (1 - 3 / 7, 0.875), "edit_within": (1 - 2 / 6, 0.875)}


def thresholds_around(base):
    """Every base threshold with its neighbours on either side, and 0.0."""
    return tuple(t for b in base for t in (math.nextafter(b, -1.0), b, math.nextafter(b, 2.0))) + (0.0,)


def text(n: int, seed: int) -> str:
    """n code units over ALPHABET (a skewed draw: common symbols repeat), no blank, so a fixed point of the preparation."""
    rng = random.Random(1000 * seed + n)
    return "".join(ALPHABET[min(int(rng.expovariate(0.12)), len(ALPHABET) - 1)] for _ in range(n))


def flip(ch: str) -> str:
    return "z" if ch != "z" else "y"


def raw_corpus(stride: int):
    """(left strings, right strings) whose longest string selects ``stride``.  Lengths at the word seams the stride holds;
    pairs that differ only in their last and only in their first code unit; for the occurrence distance the left string at
    the start, in the middle and at the very end of a right string, and right strings shorter than the left; an empty
    string on each side; 70 right strings of one length (more than one 64-lane batch in a class); 8 k + 3 left rows."""
    seams = sorted({n for n in SEAMS if stride // 2 < n <= stride} | {n for n in (1, 63, 64, 65) if n <= stride})
    long_seams = [n for n in seams if n > 8]
    left = ["kitten", "gewischt", "gewicht", "lewenstein", ""]
    right = ["sitting", "das gewicht bei aufnahme", "gewicht des patienten bei aufnahme", "levenshtein", "", "gewicht"]
    for n in seams:
        base = text(n, 1)
        left += [base, base[:-1] + flip(base[-1])]
        right += [base, base[:-1] + flip(base[-1]), flip(base[0]) + base[1:]]
    for n in long_seams:
        base = text(n, 1)
        right += [base[: n // 2], base[1:], base[:-1]]  # shorter than the left string
        room = stride - n
        if room >= 2:  # the left string inside a longer right one
            pad = text(room, 2)
            right += [base + pad, pad[: room // 2] + base + pad[room // 2:], pad + base]
    base6 = "gewich"
    right += [base6[:k % 6] + ALPHABET[(k * 7) % 36] + base6[k % 6 + 1:] for k in range(70)]  # 70 rows of 6 code units
    left += [text(6, 3), text(7, 3), text(9, 4)]
    while len(left) % 8 != 3:
        left.append(text(5 + len(left) % 4, 5))
    assert stride // 2 < max(len(s) for s in left + right) <= stride
    return left, right


def raw_hits(metric: str, left, right, threshold: float = float("-inf")):
    """The definition's records ``(score, i, j)`` with score >= threshold, canonical order (numpy rows)."""
    f = FAST[metric]
    hits = [(f(a, b), i, j) for i, a in enumerate(left) for j, b in enumerate(right)]
    return sorted((h for h in hits if h[0] >= threshold), key=lambda h: (-h[0], h[1], h[2]))


SHARP = ((15, 3), (6, 2), (19, 5), (10, 1), (12, 4))  # (length n, distance x): floor((1 - score(x)) n) lands on x - 1


def sharp_corpus():
    """(left strings, right strings) for the histogram filter without slack: right string k is left string k with x
    interior code units replaced by symbols the left side never uses, so d = x and the histogram L1 is exactly 2 x (26
    distinct symbols: every one has a bucket of its own) -- the filter d >= ceil(L1 / 2) is tight -- at lengths where the
    start guess of the greatest distance, floor((1 - eff) den) + 1, has no slack at the threshold score(x)."""
    own, foreign = "abcdefghijklmnopqrs", "tuvwxyz"
    left, right = [], []
    for n, x in SHARP:
        a = list(own[:n])
        for q in range(x):
            a[1 + (q * (n - 2)) // x] = foreign[q]
        left.append(own[:n])
        right.append("".join(a))
    return left + ["abc", "stu"], right + ["xyz", "abd"]


def saturated_corpus():
    """(left strings, right strings) at stride 512 whose rows hold more than 255 copies of one symbol: that bucket of the
    uint8 histogram column saturates, which is where the Indel sweep switches its histogram filter off and the
    NSM_METRIC_EDIT filter stays on (a saturated count only weakens d >= ceil(L1 / 2))."""
    tail = "cdefghij"
    left = ["a" * 300 + "b" * 100 + tail, "a" * 256, "a" * 255 + "b", "a" * 300, "b" * 260 + "a" * 200, "a" * 504 + tail]
    right = ["a" * 280 + "k" * 20 + "b" * 100 + tail, "a" * 260 + "b" * 140 + tail, "a" * 512, "b" * 300 + "a" * 100 + tail,
             "a" * 300 + "b" * 100 + tail, "a" * 257, "k" * 256, "a" * 250 + "b" * 6, "b" * 256 + "a" * 256]
    return left, right


# ------------------------------------------------------------------------------------------------------- explicit floors
FLOOR_CORPORA = ("raw_64", "raw_256", "levels", "levels_wide")
FLOOR_SHIFTS = {"below": -1, "on": 0, "above": 1}  # the floor against the score it is taken from, in doubles
ABOVE_ALL = 2  # this left item's floor lies one double above its best score in every case: it admits nothing


def caller_id(k):
    """Caller ids with gaps: item k reports 3 k + 2 (the floor arrays are indexed by them)."""
    return 3 * k + 2


def by_caller_id(floors):
    """A floor per item as the array the entries index by caller id; an id that names no item holds a NaN."""
    out = np.full(caller_id(len(floors) - 1) + 1, np.nan)
    out[[caller_id(k) for k in range(len(floors))]] = floors
    return out


def ranked_floors(records, n_left: int, n_right: int, rank: int, shift: int):
    """(left floors, right floors) by item: the item's ``rank``-th distinct score from the top (0: its best, 1: its second
    best; an item with fewer distinct scores: its lowest), moved ``shift`` doubles (``FLOOR_SHIFTS``).  Left item
    ``ABOVE_ALL`` gets one double above its best instead."""
    def side(pos, n):
        per = {}
        for r in records:
            per.setdefault(r[pos], set()).add(r[0])
        picked = [sorted(per[k], reverse=True)[min(rank, len(per[k]) - 1)] for k in range(n)]
        return [f if shift == 0 else math.nextafter(f, 2.0 if shift > 0 else -1.0) for f in picked], per

    (left, per_left), (right, _) = side(1, n_left), side(2, n_right)
    left[ABOVE_ALL] = math.nextafter(max(per_left[ABOVE_ALL]), 2.0)
    return left, right


def floor_cases(records, n_left: int, n_right: int, shift: int):
    """(label, left floors by item or None, right floors by item or None): the floors on the items' best and second-best
    scores, on the left side only, on the right side only, and on both."""
    out = []
    for rank in (0, 1):
        left, right = ranked_floors(records, n_left, n_right, rank, shift)
        out += [(f"rank {rank} left", left, None), (f"rank {rank} right", None, right), (f"rank {rank} both", left, right)]
    return out


def floors_plain(records, left, right):
    """The definition of a floor grid on records by item: ``score >= floor`` of both its items (None: no floor)."""
    return [r for r in records if (left is None or r[0] >= left[r[1]]) and (right is None or r[0] >= right[r[2]])]


_CORPUS = {}


def floor_corpus(kind: str):
    """(left, right) of a ``FLOOR_CORPORA`` name: ``raw_corpus`` at strides 64 and 256, the two ``levels_corpus``."""
    if kind not in _CORPUS:
        _CORPUS[kind] = raw_corpus(int(kind[4:])) if kind.startswith("raw_") else levels_corpus(kind == "levels_wide")
    return _CORPUS[kind]


def floor_corpus_records(kind: str, metric: str):
    """Every pair's record of a floor corpus, canonical order, from ``distance_table`` (one pass gives d and w); the CPU
    tests compare it with ``raw_hits`` / ``levels_hits``, which the GPU tests use."""
    if (kind, metric) not in _CORPUS:
        left, right = floor_corpus(kind)
        known = _CORPUS.setdefault((kind, "d and w"), {})
        if not known:
            flat = lambda side: sorted({s for it in side for s in ([it] if isinstance(it, str) else it)})
            distance_table(flat(left), flat(right), known)
        f =lambda a, b: plain_score(metric, len(a), len(b), *known[a, b])
        if kind.startswith("raw_"):
            hits = [(f(a, b), i, j) for i, a in enumerate(left) for j, b in enumerate(right)]
            _CORPUS[kind, metric] = sorted(hits, key=lambda h: (-h[0], h[1], h[2]))
        else:
            _CORPUS[kind, metric] = levels_hits(metric, left, right, f=f)
    return _CORPUS[kind, metric]


# --------------------------------------------------------------------------------------------------------- levels corpora
def levels_thresholds(records):
    """Two thresholds that sit exactly on scores of the yardstick's ``records``: the distinct scores a third and two
    thirds of the way up, so each has a record on it, records below it and records above it."""
    distinct = sorted({r[0] for r in records})
    assert len(distinct) >= 6
    return distinct[len(distinct) // 3], distinct[2 * len(distinct) // 3]


def levels_corpus(wide: bool):
    """(left items, right items): 1..4 levels per item, different level counts on the two sides.  Not ``wide``: level
    strings of at most 64 code units (one word); ``wide``: up to 129 (stride 256, three words).  The first right items
    share one 64-lane batch and hold level strings of lengths 1, 5, 63, 64 and 65 (``wide``) against the same left level:
    a lane that read its distance past its own length would count the wave's padding as edits."""
    top = 129 if wide else 64
    base = text(top, 7)
    lens = [1, 5, 63, 64] + ([65, 127, 128, 129] if wide else [33, 17])
    left = [[base[:n]] for n in (5, 63, 64)] + [[base[:9], base[:30]], [base[:20], base[:40], base[:top]], ["gewicht"],
            ["gewicht", "gewicht kg"], [text(12, 8), text(25, 8), text(40, 8), text(top, 8)], [base[:top]], [text(3, 9), base[:64]]]
    right = [[base[:n]] for n in lens] + [[base[:5], base[:n]] for n in lens] + \
            [[base[:9], base[:31]], [base[:21], base[:40], base[1:top]], ["das gewicht bei aufnahme"],
             ["gewicht", "gewicht in kg bei aufnahme"], [text(12, 8), text(26, 8)], [text(top, 8)],
             [text(12, 8), text(25, 8), text(41, 8), text(top, 8)], [base[2:60], base[:64], base[:top]], [text(3, 9)]]
    return left, right


def levels_categories(n_left: int, n_right: int):
    """uint64 category masks with empty ones on both sides (the "both empty" rule of the second category mode)."""
    cl = np.array([0 if k % 5 == 0 else (1 << (k % 3)) | (1 << ((k // 2) % 4)) for k in range(n_left)], dtype=np.uint64)
    cr = np.array([0 if k % 4 == 0 else (1 << (k % 4)) for k in range(n_right)], dtype=np.uint64)
    return cl, cr


def category_match(cl: int, cr: int, mode: int) -> bool:
    return bool(cl & cr) or (mode == 2 and cl == 0 and cr == 0)


def levels_hits(metric: str, left, right, threshold: float = float("-inf"), keep=lambda i, j: True, f=None):
    """``oracle.compare.compare_terms`` with the definition as score_func over the pairs ``keep`` admits: the records
    ``(score, i, j)`` with score >= threshold, canonical order."""
    from oracle.compare import compare_terms

    f = f or FAST[metric]
    hits = [(compare_terms(a, b, f), i, j) for i, a in enumerate(left) for j, b in enumerate(right) if keep(i, j)]
    return sorted((h for h in hits if h[0] >= threshold), key=lambda h: (-h[0], h[1], h[2]))
