"""The per-pair LCS of the RAW fuzzy kernels (csrc/indel_raw.hip: raw_lcs_pair) restated in plain Python, with its stop
rule, and the string families that aim at the rule (tests/test_cpu_indel_raw_lcs_abandon.py checks the model against a
plain DP, tests/test_gpu_indel_raw_lcs_abandon.py the kernels against the oracle on the same strings).

The kernel: the LONGER string of a pair is the pattern (one code unit per lane), the SHORTER one the text, fed to the
bit-parallel recurrence V' = (V + (V & M)) | (V & ~M) in words of four units.  After a word that is not the text's last,
every STOP_EVERY words, it stops where LCS so far + text units left < need: a text unit adds at most one to the LCS, so
such a pair cannot reach need any more.  A stopped call returns the count so far, which is below need.

Every family keeps to at most 32 distinct symbols, so that a bucket of the 32-bucket histogram holds one symbol whatever
codes the alphabet hands out, and the histogram bound of a pair is the sum of the per-symbol minima.
"""
import itertools
import random

STOP_EVERY = 1  # words of four text units between two stop tests: what csrc/indel_raw.hip ships (NSM_LCS_STOP_EVERY)
MASK64 = (1 << 64) - 1

HEADS = "abcdefghijklmnop"  # 16 symbols for the parts in which two strings differ in order
TAILS = "qrstuvwxyzABCDEF"  # 16 symbols for the parts they share


def need_of(thr, s):
    """The smallest LCS with which strings of la + lb = s reach ``thr`` (csrc/indel_score.hpp, the same doubles), or None."""
    for lcs in range(s // 2 + 1):
        if (1.0 - float(s - 2 * lcs) / float(s)) * 100.0 / 100.0 >= thr:
            return lcs
    return None


def pair_need(thr, x, y):
    """need of a pair as the kernels have it: 0 or None (never) for an empty string."""
    if not x or not y:
        return 0 if 0.0 >= thr else None
    return need_of(thr, len(x) + len(y))


def lcs_dp(x, y):
    """Plain dynamic programming."""
    prev = [0] * (len(y) + 1)
    for cx in x:
        cur = [0]
        for k, cy in enumerate(y):
            cur.append(prev[k] + 1 if cx == cy else max(prev[k + 1], cur[k]))
        prev = cur
    return prev[-1]


def lcs_bits(x, y):
    """Bit-parallel LCS over Python integers (the tests' quick exact LCS; test_cpu checks it against the DP)."""
    masks = {}
    for k, c in enumerate(x):
        masks[c] = masks.get(c, 0) | (1 << k)
    full = (1 << len(x)) - 1
    v = full
    for c in y:
        u = v & masks.get(c, 0)
        v = ((v + u) | (v & ~u)) & full
    return len(x) - bin(v).count("1")


def model(x, y, need, every=STOP_EVERY, shorter_as_text=True):
    """raw_lcs_pair(x, y, need): (returned count, stopped, text units processed).  ``every`` = 0: no stop test;
    ``shorter_as_text`` = False: the right string is the text whatever its length (the roles before the stop rule)."""
    pat, text = (y, x) if shorter_as_text and len(x) < len(y) else (x, y)  # the longer string sits in the lanes
    lt = len(text)
    assert len(pat) <= 64
    v = MASK64
    lim = lt - need + 64  # popcount(V) + units done > lim  <=>  (64 - popcount(V)) + (lt - units done) < need
    units, w, stopped = 0, 0, False
    go = lt > 0
    while go:
        for b in range(4):
            c = text[4 * w + b] if 4 * w + b < lt else None  # (past the text: a value no lane holds)
            m = sum(1 << k for k, p in enumerate(pat) if p == c)
            u = v & m
            v = ((v + u) | (v & ~m)) & MASK64
        units += min(4, lt - 4 * w)
        w += 1
        go = 4 * w < lt
        if go and every and w % every == 0 and bin(v).count("1") + 4 * w > lim:
            go, stopped = False, True
    return 64 - bin(v).count("1"), stopped, units


def sum_of_minima(x, y):
    """The 32-bucket histogram bound where no two symbols share a bucket."""
    return sum(min(x.count(c), y.count(c)) for c in set(x))


def reaches_lcs(thr, x, y):
    """Does the pair pass the exact filters in front of the LCS (the length filter and the 32-bucket test)?"""
    need = pair_need(thr, x, y)
    return need is not None and min(len(x), len(y)) >= need and sum_of_minima(x, y) >= need


def boundary_pairs(thr, left, right):
    """{lcs - need} over the pairs that reach the LCS, restricted to 0 and -1, with one example each."""
    seen = {}
    for (i, x), (j, y) in itertools.product(enumerate(left), enumerate(right)):
        if x and y and reaches_lcs(thr, x, y):
            d = lcs_bits(x, y) - pair_need(thr, x, y)
            if d in (0, -1):
                seen.setdefault(d, (i, j))
    return seen


# --- the families ------------------------------------------------------------------------------------------------------------


def _tail(n, rng):
    return "".join(rng.choice(TAILS) for _ in range(n))


def late_matches(thr=0.8, lengths=(17, 31, 32, 33, 40, 63, 64), seed=1):
    """Left J.T and right J'.T (``late``) or T.J and T.J' (``early``): J distinct symbols, J' their reversal (LCS(J, J') = 1)
    or J with only its last part reversed, T a common part over other symbols, so LCS = LCS(J, J') + |T| with identical
    multisets.  Per length one such pair at LCS == need and one at need - 1.  Returns (left, right, [(i, j, lcs - need)])."""
    rng = random.Random(seed)
    left, right, planned = [], [], []
    for n, late, keep in itertools.product(lengths, (True, False), (0, 2)):
        need = need_of(thr, 2 * n)
        for d in (0, -1):
            t = need + d - 1 - keep  # LCS = keep + 1 + t
            j = n - t
            if not 2 <= j - keep or j > len(HEADS):
                continue
            head = "".join(rng.sample(HEADS, j))
            other = head[:keep] + head[keep:][::-1]
            tail = _tail(t, rng)
            x, y = (head + tail, other + tail) if late else (tail + head, tail + other)
            planned.append((len(left), len(right), d))
            left.append(x)
            right.append(y)
    return left, right, planned


ROLE_LENGTHS = (16, 17, 18, 31, 32, 33, 62, 63, 64)  # text lengths 0, 1, 2, 3 mod 4; patterns of <= 32 and of more units


def roles_and_word_edges(thr=0.4, seed=2):
    """Every (la, lb) of ROLE_LENGTHS x ROLE_LENGTHS (la < lb, la > lb, la == lb), each with one pair at LCS == need and
    one at need - 1 that both pass the histogram test: a common part C, a part J that the other string holds reversed
    (LCS 1, but |J| for the histograms), and fillers over symbols the other string lacks; the common parts sit at the
    strings' ends or at their starts in turn.  At ``thr`` = 0.4 every pair of lengths passes the length filter."""
    rng = random.Random(seed)
    c_syms, j_syms, x_syms, y_syms = TAILS, HEADS[:6], HEADS[6:11], HEADS[11:]
    left, right, planned = [], [], []
    for k, (la, lb) in enumerate(itertools.product(ROLE_LENGTHS, ROLE_LENGTHS)):
        need = need_of(thr, la + lb)
        assert need is not None and need <= min(la, lb)
        for d in (0, -1):
            j = 3
            c = need + d - 1  # LCS = c + 1
            if c + j > min(la, lb):  # no room for the reversed part: the common part alone (then the bound is tight)
                j = 2 if d == -1 else 0
                c = need + d - (1 if j else 0)
            assert c >= 0 and c + j <= min(la, lb)
            common = "".join(rng.choice(c_syms) for _ in range(c))
            turn = "".join(rng.sample(j_syms, j))
            fx = "".join(rng.choice(x_syms) for _ in range(la - c - j))
            fy = "".join(rng.choice(y_syms) for _ in range(lb - c - j))
            if k % 2:
                x, y = common + turn + fx, common + turn[::-1] + fy
            else:
                x, y = fx + turn + common, fy + turn[::-1] + common
            assert len(x) == la and len(y) == lb
            planned.append((len(left), len(right), d))
            left.append(x)
            right.append(y)
    return left, right, planned


def threshold_one(seed=3):
    """Identical strings, strings that differ only in the first or only in the last unit (the histograms stop those), and
    strings with their first two or last two units exchanged (same multiset, LCS = n - 1 = need - 1 at threshold 1.0)."""
    rng = random.Random(seed)
    left, right, planned = [], [], []
    for n in (16, 17, 18, 19, 32, 33, 63, 64):
        s = "".join(rng.choice(TAILS) for _ in range(n - 4))
        s = "ab" + s + "cd"
        variants = [(s, 0), ("e" + s[1:], None), (s[:-1] + "e", None), ("ba" + s[2:], -1), (s[:-2] + "dc", -1)]
        for y, d in variants:
            if d is not None:
                planned.append((len(left), len(right), d))
            right.append(y)
        left.append(s)
    return left, right, planned


def threshold_zero(seed=4):
    """Random strings and empty rows: at threshold 0 every pair is a hit and need is 0."""
    rng = random.Random(seed)
    word = lambda: "".join(rng.choice(HEADS + TAILS) for _ in range(rng.randint(1, 64)))
    left = [word() for _ in range(37)] + ["", "", "q" * 64]
    right = ["", "q" * 64] + [word() for _ in range(38)]
    return left, right


def crowded_drain(seed=5, n_left=96, n_right=161):
    """A 4-letter alphabet: most pairs pass the coarse test and many the 32-bucket test, stack entries carry several
    pairs and one drain pass runs several LCS calls back to back, stopped ones among them; ``n_left`` rows of ONE length
    (three blocks) x ``n_right`` rows fill the stack beyond its drain level inside the class."""
    rng = random.Random(seed)
    word = lambda n: "".join(rng.choice("abcd") for _ in range(n))
    left = [word(40) for _ in range(n_left)]
    right = [word(rng.randint(28, 56)) for _ in range(n_right)]
    # near copies, so that hits stand beside the stopped pairs: units replaced one by one (the LCS falls by at most one a
    # time) until the copy is ``short`` below the left row's length; 8 and 9 short are need and need - 1 at 40 + 40 units
    for k in range(0, n_right, 7):
        x = left[(3 * k) % n_left]
        y, short = list(x), (k // 7) % 4 + 6
        while len(x) - lcs_bits(x, "".join(y)) < short:
            y[rng.randrange(len(y))] = rng.choice("abcd")
        right[k] = "".join(y)
    return left, right
