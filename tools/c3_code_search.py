#!/usr/bin/env python3
"""Search and check tool for the FP4 value tables of the packed C3 scan (csrc/indel_raw_coarse.hpp, NSM_C3C_CODES2).  CPU only.

Per bucket, with a the left count, r the right count and k the right string's scale exponent, the packed scan computes

    D_b = [a >= 1][r >= 1] + [a >= 2][r >= 2] + 2^k (x3(a) y3(rho) + x4(a) y4(rho)),    rho = rho_k(r)

with x3, x4, y3, y4 tables of E2M1 values over the counts 0 .. 15:

    left    a count above 15 reads entry 15 (the left side has no scale: it saturates);
    right   k = 0 (no count above 15): rho = r.  k > 0: rho = r below 3, else 2 + ceil((r - 2) / 2^k), which the choice of k
            (c3c_fp4_scale: the smallest with max r - 3 <= 12 x 2^k) keeps at 15 or below.

The tables satisfy  x3(a) y3(r) + x4(a) y4(r) >= max(min(a, r) - 2, 0)  for a, r in 0 .. 15.  For every a, r in 0 .. 64 and
every k a string can carry this gives D_b >= min(a, r): with A = min(a, 15) and m = max(min(A, rho) - 2, 0),
2^k m >= min(a - 2, r - 2) because either A - 2 is the smaller (then a - 2 <= 2^k (A - 2) where a <= 15, and rho <= 15 = A
otherwise) or 2^k ceil((r - 2) / 2^k) >= r - 2 is.  `check_bound` does not rely on that argument: it walks every a, r, k.

The search minimises the number of pairs of a seeded sample (synthetic.strings(4000, 1234) x synthetic.strings(4000, 5678),
threshold 0.8) whose bound reaches need = lcsmin[la + lb], over monotone tables.  Two families:

    integer   every product x(a) y(r) of a slot is an integer: the 9-bit fields, the bias and the fold mask of the OR fold
              stay as they are;
    quarter   any E2M1 values (products are multiples of 1/4): the fields would have to be widened.

The integer tables are taken if they pass at most 1.25 x the pairs the quarter tables pass.

    python tools/c3_code_search.py [--seconds S] [--seed N]      search both families, print the tables and their counts
    python tools/c3_code_search.py --check                       check and count the tables the kernel ships (SHIPPED)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "napkon-string-matching_amd"))

FP4 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # E2M1 codes 0 .. 7
NEVER = 255
TOP = 15          # the tables' last count
MAX_FIELD_D = 254  # OR fold: D < 256 + need for need >= 0, and D + 1 < 256 for need = kNever, whichever width the fields have

# The tables the kernel ships, as E2M1 codes by count 0 .. 15: this tool's output (--seconds 240 --seed 1; the search runs
# against the clock, so another machine may print other tables: --check is what vouches for these), pasted.
SHIPPED = {
    "x3": (0, 0, 0, 4, 4, 4, 4, 4, 4, 4, 4, 5, 6, 6, 6, 7),
    "x4": (0, 0, 0, 0, 2, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4),
    "y3": (0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3),
    "y4": (0, 0, 0, 0, 2, 4, 4, 4, 5, 5, 5, 5, 5, 5, 5, 5),
}
NAMES = ("x3", "x4", "y3", "y4")


# --- the rules the kernel follows ----------------------------------------------------------------------------------------------


def scale_of(top):
    """k of a right string whose largest count is `top` (c3c_fp4_scale)."""
    return 0 if top <= 15 else 1 if top <= 27 else 2 if top <= 51 else 3


def rho(r, k):
    """The right table's index of a count r under the scale exponent k."""
    if k == 0 or r < 3:
        return r
    return 2 + ((r - 2 + (1 << k) - 1) >> k)


def values(codes):
    return np.array([FP4[c] for c in codes])


def bucket_table(tables, k):
    """T[a][r] = D_b for a in 0 .. 64 and the r in 0 .. 64 that a string with exponent k can hold (-1 elsewhere)."""
    x3, x4, y3, y4 = (values(tables[n]) for n in NAMES)
    top_r = (15, 27, 51, 64)[k]
    out = -np.ones((65, 65))
    for a in range(65):
        ai = min(a, TOP)
        for r in range(top_r + 1):
            ri = rho(r, k)
            assert ri <= TOP, (r, k)
            out[a, r] = min(a, r, 2) + (1 << k) * (x3[ai] * y3[ri] + x4[ai] * y4[ri])
    return out


def check_bound(tables):
    """D_b >= min(a, r) for every a, r in 0 .. 64 and every k that a string holding r can carry.  A string's k comes from its
    LARGEST count, so a count r meets every k from scale_of(r) up."""
    for k in range(4):
        t = bucket_table(tables, k)
        for a in range(65):
            for r in range(65):
                if scale_of(r) <= k:
                    assert t[a, r] >= min(a, r), (a, r, k, t[a, r])
                    # slots 3 and 4 alone: the statement of the tables' own condition
                    assert t[a, r] - min(a, r, 2) >= max(min(a, r) - 2, 0), (a, r, k)
    return True


def is_monotone(tables):
    return all(all(p <= q for p, q in zip(tables[n], tables[n][1:])) for n in NAMES)


def products_are_integers(tables):
    for xs, ys in (("x3", "y3"), ("x4", "y4")):
        for x in set(tables[xs]):
            for y in set(tables[ys]):
                if (FP4[x] * FP4[y]) % 1.0 != 0.0:
                    return False
    return True


def _maxplus(f, g):
    """h[A][R] = max over a <= A, r <= R of f[A - a][R - r] + g[a][r] (arrays 65 x 65, -inf where impossible)."""
    h = np.full((65, 65), -np.inf)
    for a in range(65):
        for r in range(65):
            if g[a, r] == -np.inf:
                continue
            h[a:, r:] = np.maximum(h[a:, r:], f[: 65 - a, : 65 - r] + g[a, r])
    return h


def max_bound(tables):
    """The largest D over all pairs of 32-bucket histograms with sum a <= 64 and sum r <= 64, by exponent k: a max-plus
    knapsack over the buckets.  For k > 0 one bucket holds a count that calls for k (above 15, 27, 51), the other 31 any count
    that k allows."""
    out = []
    for k in range(4):
        t = bucket_table(tables, k)
        any_r = np.where(t >= 0, t, -np.inf)
        pw = {1: any_r}
        for n in (2, 4, 8, 16):
            pw[n] = _maxplus(pw[n // 2], pw[n // 2])
        f31 = _maxplus(_maxplus(_maxplus(_maxplus(pw[16], pw[8]), pw[4]), pw[2]), pw[1])
        forced = any_r.copy()
        if k > 0:
            forced[:, : (16, 28, 52)[k - 1]] = -np.inf
        out.append(float(_maxplus(f31, forced).max()))
    return out


# --- the sample ----------------------------------------------------------------------------------------------------------------


def lcsmin_of(threshold):
    out = [NEVER] * 132
    for s in range(2, 129):
        for lcs in range(0, s // 2 + 1):
            if (1.0 - (s - 2 * lcs) / s) * 100.0 / 100.0 >= threshold:
                out[s] = lcs
                break
    return out


def histograms(n, seed):
    from napkon_string_matching_amd import synthetic

    codes, length = synthetic.strings(n, seed)
    hist = np.zeros((n, 32), dtype=np.int64)
    for i in range(n):
        hist[i] = np.bincount(codes[i, : length[i]] & 31, minlength=32)
    return hist, length.astype(np.int64)


class Sample:
    """4000 x 4000 seeded strings at threshold 0.8.  Every count is 15 or below (k = 0), which `__init__` asserts."""

    def __init__(self, n=4000, threshold=0.8):
        self.lh, self.ll = histograms(n, 1234)
        self.rh, self.rl = histograms(n, 5678)
        assert self.lh.max() <= 15 and self.rh.max() <= 15
        lcsmin = np.array(lcsmin_of(threshold))
        self.need = lcsmin[self.ll[:, None] + self.rl[None, :]]
        self.fits = np.minimum(self.ll[:, None], self.rl[None, :]) >= self.need
        self.pairs = int(self.fits.sum())
        # slots 1 and 2: sum of min(a, r, 2)
        f = np.float32
        self.d12 = sum((self.lh >= s).astype(f) @ (self.rh >= s).astype(f).T for s in (1, 2))
        self.sum_min = sum((self.lh >= s).astype(f) @ (self.rh >= s).astype(f).T for s in range(1, 16))

    def passes_of_bound(self, d):
        return int(((d >= self.need) & self.fits).sum())

    def d_of(self, tables):
        x3, x4, y3, y4 = (values(tables[n]).astype(np.float32) for n in NAMES)
        return self.d12 + x3[self.lh] @ y3[self.rh].T + x4[self.lh] @ y4[self.rh].T

    def passes(self, tables):
        d = self.d_of(tables)
        assert not ((self.sum_min >= self.need) & self.fits & (d < self.need)).any(), "a pair with sum of min >= need is dropped"
        return self.passes_of_bound(d)

    def passes_present(self, fp4_grid=True):
        """The code of before: slots [>= 1], [>= 2], [>= 3] and [a >= 4] E(r - 3), E on the grid 0 1 2 3 4 6 8 12 or exact."""
        grid = (0, 1, 2, 3, 4, 6, 8, 12)
        e = np.array([0.0 if r <= 3 else (min(g for g in grid if g >= r - 3) if fp4_grid else r - 3) for r in range(16)], dtype=np.float32)
        f = np.float32
        d = self.d12 + (self.lh >= 3).astype(f) @ (self.rh >= 3).astype(f).T + (self.lh >= 4).astype(f) @ e[self.rh].T
        return self.passes_of_bound(d)

    def candidates(self, margin=3):
        """The pairs the search looks at: those the present code passes and those whose sum of min is within `margin` of their
        need.  (A table that passes other pairs is still counted in full by `passes`: this set only steers.)"""
        f = np.float32
        present = self.d12 + (self.lh >= 3).astype(f) @ (self.rh >= 3).astype(f).T + (self.lh >= 4).astype(f) @ np.maximum(self.rh - 3, 0).astype(f).T
        li, ri = np.nonzero(((present >= self.need) | (self.sum_min + margin >= self.need)) & self.fits)
        combos = np.zeros((len(li), 256), dtype=np.float32)
        a, r = self.lh[li], self.rh[ri]
        live = (a >= 3) & (r >= 3)
        rows = np.repeat(np.arange(len(li))[:, None], 32, axis=1)
        np.add.at(combos, (rows[live], (a * 16 + r)[live]), 1.0)
        slack = (self.need - self.d12)[li, ri].astype(np.float32)  # what the slots 3 and 4 must reach for a pass
        return combos, slack


# --- the search ----------------------------------------------------------------------------------------------------------------

CLASSES = {"even": (0, 4, 6, 7), "int": (0, 2, 4, 5, 6, 7), "any": (0, 1, 2, 3, 4, 5, 6, 7)}  # E2M1 codes: 2 4 6 | integers | all
INTEGER_FAMILIES = (("even", "any"), ("int", "int"), ("any", "even"))  # (left, right) value sets whose products are integers


def t34_of(tab):
    x3, x4, y3, y4 = (values(tab[n]) for n in NAMES)
    return np.outer(x3, y3) + np.outer(x4, y4)


def feasible(tab):
    t = t34_of(tab)
    idx = np.arange(16)
    return bool((t >= np.maximum(np.minimum(idx[:, None], idx[None, :]) - 2, 0)).all())


def anneal(combos, slack, allowed, seconds, rng):
    """Simulated annealing over monotone tables whose entries come from `allowed[name]`.  A move sets one entry to a
    neighbouring allowed value and drags the entries beside it along so that the table stays monotone."""
    weight = combos.sum(axis=0) / len(slack)

    def cost(tab):
        t = t34_of(tab).reshape(256).astype(np.float32)
        return float(((combos @ t) >= slack).sum()) + 50.0 * float(weight @ t) + 1e-3 * float(t.sum())

    # the start: slot 3 the indicator pair of before (a product of 1 from a count of 3 on), slot 4 the loosest from 4 on
    one = next({"x3": x, "y3": y} for x, y in ((4, 1), (2, 2), (1, 4)) if x in allowed["x3"] and y in allowed["y3"])
    tab = {n: [0, 0, 0] + ([one[n]] * 13 if n in one else [0] + [allowed[n][-1]] * 12) for n in NAMES}
    assert feasible(tab)
    cur = cost(tab)
    best, best_cost = {n: tuple(v) for n, v in tab.items()}, cur
    t0, step = time.time(), 0
    while time.time() - t0 < seconds:
        step += 1
        temp = 3.0 * max(1.0 - (time.time() - t0) / seconds, 0.0) ** 2 + 1e-3
        n = NAMES[rng.integers(4)]
        i = int(rng.integers(3, 16))
        vals = allowed[n]
        at = vals.index(tab[n][i])
        to = at + (1 if rng.random() < 0.35 else -1)
        if to < 0 or to >= len(vals):
            continue
        new = list(tab[n])
        new[i] = vals[to]
        for j in range(3, i):
            new[j] = min(new[j], new[i])
        for j in range(i + 1, 16):
            new[j] = max(new[j], new[i])
        trial = dict(tab)
        trial[n] = new
        if not feasible(trial):
            continue
        c = cost(trial)
        if c <= cur or rng.random() < np.exp((cur - c) / temp):
            tab, cur = trial, c
            if c < best_cost:
                best, best_cost = {m: tuple(v) for m, v in tab.items()}, c
    return best, best_cost


def search(sample, seconds, seed):
    combos, slack = sample.candidates()
    print(f"# search set: {len(slack)} pairs of {sample.pairs}")
    rng = np.random.default_rng(seed)
    results = {}
    runs = [("integer", s3, s4) for s3 in INTEGER_FAMILIES for s4 in INTEGER_FAMILIES] + [("quarter", ("any", "any"), ("any", "any"))] * 3
    for family, s3, s4 in runs:
        allowed = {"x3": CLASSES[s3[0]], "y3": CLASSES[s3[1]], "x4": CLASSES[s4[0]], "y4": CLASSES[s4[1]]}
        tab, _ = anneal(combos, slack, allowed, seconds / len(runs), rng)
        n = sample.passes(tab)
        print(f"#   {family:8s} slot 3 {s3}, slot 4 {s4}: {n} pairs pass")
        if family not in results or n < results[family][0]:
            results[family] = (n, tab)
    return results


# --- output --------------------------------------------------------------------------------------------------------------------


def byte_tables(tables):
    """The kernel's constants: the byte of a count is slot 3's code in its low nibble and slot 4's in its high nibble; counts
    0 .. 3 and 4 .. 7 are the two words of the table v_perm_b32 reads for a count below 8, 8 .. 11 and 12 .. 15 the other's."""
    out = {}
    for side, lo, hi in (("left", "x3", "x4"), ("right", "y3", "y4")):
        b = [tables[lo][c] | (tables[hi][c] << 4) for c in range(16)]
        out[side] = [sum(b[4 * w + j] << (8 * j) for j in range(4)) for w in range(4)]
    return out


def report(sample, name, tables):
    assert is_monotone(tables), name
    check_bound(tables)
    n = sample.passes(tables)
    tops = max_bound(tables)
    print(f"{name}: {n} of {sample.pairs} pairs pass ({n / sample.pairs:.3g}); products integers: {products_are_integers(tables)}; "
          f"largest D by k: {tops}")
    for t in NAMES:
        print(f"    {t} codes  {tuple(tables[t])}   values {[FP4[c] for c in tables[t]]}")
    bt = byte_tables(tables)
    for side in ("left", "right"):
        print(f"    {side:5s} byte tables, counts 0-3, 4-7, 8-11, 12-15: " + ", ".join(f"0x{w:08x}" for w in bt[side]))
    return n, tops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    sample = Sample()
    now = sample.passes_present()
    print(f"pairs that pass the length filter: {sample.pairs} of {len(sample.ll) * len(sample.rl)}")
    print(f"present code: {now} pairs pass ({now / sample.pairs:.3g}); without the FP4 rounding of E: {sample.passes_present(False)}; "
          f"sum of min: {sample.passes_of_bound(sample.sum_min)}")
    if args.check:
        n, tops = report(sample, "shipped", SHIPPED)
        assert max(tops) <= MAX_FIELD_D  # (quarter products: the fields are 4 D + 1024 - 4 need in 11 bits)
        assert n <= 0.45 * now
        print(f"shipped / present = {n / now:.3f}")
        return
    results = search(sample, args.seconds, args.seed)
    counts = {}
    for family, (_, tab) in results.items():
        counts[family], tops = report(sample, family, tab)
        assert max(tops) <= MAX_FIELD_D, "the fields of the OR fold would carry"
    take = "integer" if counts["integer"] <= 1.25 * counts["quarter"] else "quarter"
    print(f"integer / quarter = {counts['integer'] / counts['quarter']:.3f}: take the {take} tables; against the present code "
          f"{counts[take] / now:.3f}")


if __name__ == "__main__":
    main()
