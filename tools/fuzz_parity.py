#!/usr/bin/env python3
"""Randomised differential test of every grid kernel against the C oracle (oracle/c/nsm_oracle.c), for a
time budget:  python tools/fuzz_parity.py [--seconds 300] [--seed 0]

Each round draws a kernel family, table shapes, vocabulary / alphabet sizes, category layout, partition
on/off and a threshold, and requires the hit list (score, i, j) to be IDENTICAL to the oracle's.  Exits
non-zero with the failing round's seed.  Test infrastructure: not part of the product path.
"""
import argparse
import os
import json
import math
import random
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "napkon-string-matching_amd"), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--family", default=None, help="only this kernel family (jaccard_raw, indel_raw, jaccard_levels, indel_levels, indel_split, wide; "
                    "indel_top_k, jaccard_top_k, indel_raw_top_k_grouped, jaccard_raw_top_k_grouped, indel_levels_top_k, jaccard_levels_top_k, wide_levels_indel and wide_levels_jaccard are "
                    "drawn only when named here)")
    ap.add_argument("--on-score", action="store_true", help="in about one round in four, whatever the family, take the threshold "
                    "from the oracle's own score list of that round: a score s, or nextafter(s, 2.0)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from napkon_string_matching_amd import _lib, grid, tables
    from oracle import native

    dev = torch.device("cuda:0")
    thresholds = [0.0, 1e-9, 0.05, 0.1, 0.25, 1 / 3, 0.4, 0.5, 0.6, 2 / 3, 0.7, 0.75, 0.8, 0.9, 0.95, 1.0, 1.2]
    counts = {}
    t_end = time.time() + args.seconds
    rnd = args.seed
    total_hits = 0

    def check(got, want, what):
        nonlocal total_hits
        got_t = got.as_tuples()
        total_hits += len(want)
        if got_t != want:
            extra = sorted(set(got_t) - set(want))[:5]
            missing = sorted(set(want) - set(got_t))[:5]
            print(json.dumps({"FAIL": what, "round_seed": rnd, "got": len(got_t), "want": len(want),
                              "extra": extra, "missing": missing}))
            sys.exit(1)

    def rand_sets(rng, n, kmax, vocab, allow_empty):
        rows = []
        for _ in range(n):
            k = rng.randint(0 if allow_empty else 1, kmax)
            rows.append(rng.sample(range(vocab), min(k, vocab)))
        return rows

    def dup_some(rng, left, right, frac, mutate):
        for k in range(len(right)):
            if rng.random() < frac and left:
                right[k] = mutate(list(left[rng.randrange(len(left))]))

    def nested_item(rng, vocab, max_levels, max_new):
        base, out = [], []
        for _ in range(rng.randint(1, max_levels)):
            for v in rng.sample(range(vocab), min(vocab, rng.randint(0 if base else 1, max_new))):
                if v not in base:
                    base.append(v)
            out.append(list(base))
        return out

    def rand_string(rng, alphabet, lo, hi):
        return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))).strip()

    def on_score(thr, oracle):
        """The round's threshold: in an on-score round a positive score ``s`` of the round's own oracle list (``oracle(t)`` = the
        list at threshold t), or one ulp above it; else ``thr`` as drawn.  Every family passes its oracle call through here."""
        if not score_round:
            return thr
        positive = [h[0] for h in oracle(0.0) if h[0] > 0.0]
        if not positive:
            return thr
        s = score_rng.choice(positive)
        return s if score_rng.random() < 0.5 else math.nextafter(s, 2.0)

    next_report = time.time() + 60.0
    while time.time() < t_end:
        rnd += 1
        if time.time() >= next_report:  # a long silent GPU job is taken to be hung
            print(json.dumps({"progress": counts, "round_seed": rnd}), flush=True)
            next_report += 60.0
        rng = random.Random(rnd)
        # posting entries of the global inverted index (include/nsm_hip.h: post_format): every format gets its share
        fmt_rng = random.Random(rnd * 7919 + 1)
        tables.COMPACT_POSTINGS = fmt_rng.random() < 0.8
        tables.RAW_POST_FORMAT = fmt_rng.choice([1, 2, 2])
        family = rng.choice(["jaccard_raw", "indel_raw", "jaccard_levels", "indel_levels", "indel_levels", "indel_split", "wide"])
        if args.family:
            family = args.family
        counts[family] = counts.get(family, 0) + 1
        thr = rng.choice(thresholds)
        # (--on-score) a generator of its own decides, so that the rounds' other draws stay what they are without the option
        score_rng = random.Random(rnd * 104729 + 3)
        score_round = args.on_score and score_rng.random() < 0.25
        if score_round:
            counts["on_score"] = counts.get("on_score", 0) + 1
        n, m = rng.randint(1, 400), rng.randint(1, 600)
        if family in ("wide_levels_indel", "wide_levels_jaccard"):
            # the general kernels (csrc/any_grids.hip) called directly, levels mode: depths up to 300 in one wave, string
            # lengths at the chunk seams / carry words / the cap, alphabets at 255 / 256 / 1023, nested or independent level
            # sets, 64-bit category masks, thresholds from the list or exactly on an oracle score.  Only through --family.
            from napkon_string_matching_amd import wide
            from support import any_operands as ao

            n, m = rng.randint(1, 40), rng.randint(1, 140)
            deep = rng.random() < 0.5
            depth = lambda: rng.choice([1, 2, 3, 4, 8, 63, 64, 65, 100, 300] if deep else [1, 1, 2, 3, 4, 8])
            mode = rng.choice([_lib.CAT_NONE, _lib.CAT_INTERSECT, _lib.CAT_INTERSECT_OR_BOTH_EMPTY])
            lcat, rcat = (None, None) if mode == _lib.CAT_NONE else (ao._masks(rng, n), ao._masks(rng, m))
            if family == "wide_levels_indel":
                alphabet = rng.choice([1, 4, 12, 255, 256, 1023])
                edges = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]
                budget = [3]  # strings at the cap per grid (the oracle's LCS is quadratic)

                def length(d):
                    if d > 8:
                        return rng.randint(0, 20)
                    if budget[0] and rng.random() < 0.02:
                        budget[0] -= 1
                        return rng.choice([4095, 4096])
                    return rng.choice(edges) if rng.random() < 0.4 else rng.randint(0, 90)

                def item():
                    d = depth()
                    return [ao._units(rng, length(d), alphabet) for _ in range(d)]

                def mutate(it):
                    it = [list(lv) for lv in it]
                    for _ in range(rng.randint(0, 2)):
                        lv = it[rng.randrange(len(it))]
                        if lv:
                            at = rng.choice([0, len(lv) - 1, min(len(lv) - 1, 127), min(len(lv) - 1, 128), rng.randrange(len(lv))])
                            lv[at:at + 1] = [] if rng.random() < 0.5 else [rng.randrange(alphabet)]
                    return it if rng.random() < 0.7 else ao._recut(rng, it)

                what = f"|alphabet|={alphabet}"
            else:
                nested = rng.random() < 0.5
                vocab = rng.choice([30, 300, 5000])
                width = lambda: rng.randint(65, min(300, vocab)) if vocab > 65 and rng.random() < 0.1 else rng.randint(1, min(vocab, 6))

                def item(may_be_empty=False):
                    d = depth()
                    if nested:
                        return ao._nested_item(rng, d, vocab, max_new=rng.choice([1, 2, min(40, vocab)]), start=rng.randint(1, 3))
                    return [[] if may_be_empty and rng.random() < 0.1 else rng.sample(range(vocab), width()) for _ in range(d)]

                def mutate(it):
                    it = [list(lv) for lv in it]
                    if rng.random() < 0.5:  # one more token from some level on (a nested item stays nested)
                        at = rng.randrange(len(it))
                        it = [lv + [vocab + 1] if k >= at else lv for k, lv in enumerate(it)]
                    return it if rng.random() < 0.7 else ao._recut(rng, it)

                what = f"nested={nested} vocab={vocab}"
            left = [item() for _ in range(n)]
            right = [item(True) if family == "wide_levels_jaccard" else item() for _ in range(m)]
            dup_some(rng, left, right, rng.choice([0.0, 0.15, 0.5]), mutate)
            g = ao.Grid(f"round{rnd}", "indel" if family == "wide_levels_indel" else "jaccard", left, right, cat_l=lcat, cat_r=rcat,
                        mode=mode)
            full = ao.oracle_call(g, 0.0)
            if full and rng.random() < 0.5:  # exactly on a pair's score, or one ulp above it
                thr = rng.choice(full)[0]
                if rng.random() < 0.3:
                    thr = math.nextafter(thr, 2.0)
            thr = on_score(thr, lambda t: ao.oracle_call(g, t))  # (besides this family's own, older draw on a score)
            want = ao.oracle_call(g, thr)
            kl, kr = ao.kernel_operands(g)
            fn = wide.indel_any_grid if g.kind == "indel" else wide.jaccard_any_grid
            got = fn(kl, kr, thr, lcat, rcat, mode, capacity=rng.choice([None, 16]))
            check(got, want, f"{family} {what} deep={deep} thr={thr!r} mode={mode} {n}x{m}")
            continue
        if family in ("indel_levels_top_k", "jaccard_levels_top_k"):
            # per-item top-k of the levels grids (nsm_*_levels_top_k) against the definition: the oracle's levels grid
            # without the banned pairs, cut per left item after rank k (score descending, j ascending).  Draws categories,
            # banned pairs, depths, strides, k and thresholds.  Only through --family: the default draw is unchanged.
            thr = rng.choice(thresholds + [-1.0, 0.0, -0.5])
            n, m = rng.randint(1, 100), rng.randint(1, 200)
            k = rng.choice([1, 1, 2, 3, 5, 10, rng.randint(1, m + 8), m, m + 3])
            prune = rng.random() < 0.75
            ncat = rng.choice([0, 0, 3, 6, 64])
            mode = _lib.CAT_NONE if ncat == 0 else rng.choice([_lib.CAT_INTERSECT, _lib.CAT_INTERSECT_OR_BOTH_EMPTY])
            lcat = rcat = None
            if ncat:
                def cats(cnt):
                    out = np.zeros(cnt, dtype=np.uint64)
                    for q in range(cnt):
                        for _ in range(rng.choice([0, 1, 1, 2, 3])):
                            out[q] |= np.uint64(1) << np.uint64(rng.randrange(ncat))
                    return out

                lcat, rcat = cats(n), cats(m)
            if family == "jaccard_levels_top_k":
                vocab = rng.choice([12, 60, 400, 20_000])
                max_levels, max_new = rng.choice([1, 2, 4, 9, 20, 64]), rng.choice([1, 2, 3, 8])
                left = [nested_item(rng, vocab, max_levels, max_new) for _ in range(n)]
                right = [nested_item(rng, vocab, max_levels, max_new) for _ in range(m)]
                dup_some(rng, left, right, rng.choice([0.0, 0.1, 0.5]), lambda it: [list(lv) for lv in it])  # exact copies: ties
                biggest = max(len(it[-1]) for it in left + right)
                if biggest > 64:
                    continue
                width = rng.choice([w for w in (16, 32, 64) if w >= biggest])
                vocabulary = tables.Vocabulary()
                lt = tables.SetTable.from_levels(left, "left", dev, vocabulary, width=width, categories=lcat, category_mode=mode,
                                                 partition=False, index=False)
                rt = tables.SetTable.from_levels(right, "right", dev, vocabulary, width=width, categories=rcat, category_mode=mode,
                                                 partition=False, index=False)
                thr = on_score(thr, lambda t: native.levels(False, left, right, t, lcat, rcat, mode, cap=n * m + 1))
                full = native.levels(False, left, right, thr, lcat, rcat, mode, cap=n * m + 1)
                what = f"W={width} vocab={vocab} levels<={max_levels} new<={max_new}"
            else:
                hi = rng.choice([4, 10, 40, 64, 64, 120, 250, 500])
                alphabet = rng.choice(["ab", "abc ", "abcdefghij klm", "abcdefghijklmnopqrstuvwxyz0123456789 ",
                                       "".join(chr(0x100 + c) for c in range(250))])
                max_levels = rng.choice([1, 2, 4, 4, 7, 64])
                item = lambda: [rand_string(rng, alphabet, 0, hi) for _ in range(rng.randint(1, max_levels))]
                left, right = [item() for _ in range(n)], [item() for _ in range(m)]
                dup_some(rng, left, right, rng.choice([0.0, 0.1, 0.5]), lambda it: list(it))  # exact copies: ties
                li, ls, ri, rs = tables.encode_level_strings(left, right, dev, lcat, rcat, mode, partition=False)
                cps = lambda items: [[[ord(c) for c in s_] for s_ in it] for it in items]
                thr = on_score(thr, lambda t: native.levels(True, cps(left), cps(right), t, lcat, rcat, mode, cap=n * m + 1))
                full = native.levels(True, cps(left), cps(right), thr, lcat, rcat, mode, cap=n * m + 1)
                what = f"hi={hi} stride={ls.stride} |alphabet|={len(alphabet)} levels<={max_levels}"
            # banned: random pairs and, per row, often its best pair (what the list would otherwise keep first)
            banned = {(rng.randrange(n), rng.randrange(m)) for _ in range(rng.choice([0, 0, 3, n]))}
            best = {}
            for h in full:
                if h[1] not in best or (-h[0], h[2]) < (-best[h[1]][0], best[h[1]][2]):
                    best[h[1]] = h
            banned |= {(i_, h[2]) for i_, h in best.items() if rng.random() < 0.3}
            ban_arr = None
            if banned:
                arr = np.array(sorted(banned), dtype=np.int64)
                ban_arr = (arr[:, 0], arr[:, 1])
            what = (f"{family} {what} thr={thr} k={k} prune={prune} mode={mode} ncat={ncat} banned={len(banned)} {n}x{m}")
            if family == "jaccard_levels_top_k":
                got = grid.jaccard_levels_top_k(lt, rt, k, thr, category_mode=mode, prune=prune, banned=ban_arr)
            else:
                got = grid.indel_levels_top_k(li, ls, ri, rs, k, thr, category_mode=mode, prune=prune, banned=ban_arr)
            rows = {}
            for h in full:
                if (h[1], h[2]) not in banned:
                    rows.setdefault(h[1], []).append(h)
            want = sorted((h for lst in rows.values() for h in sorted(lst, key=lambda t: (-t[0], t[2]))[:k]),
                          key=lambda t: (-t[0], t[1], t[2]))
            check(got, want, what)
            continue
        if family in ("indel_raw_top_k_grouped", "jaccard_raw_top_k_grouped"):
            # grouped top-k (nsm_*_raw_top_k_grouped) against the definition (tests/support/grouped.py): the oracle's full
            # grid at the threshold, per left item the best row of every group, of those the first k.  Shapes, alphabets,
            # empty rows, k, threshold, prune and the group pattern are drawn.  Only through --family.
            from support.grouped import GROUP_PATTERNS, draw_groups, group_cut

            thr = rng.choice(thresholds + [-1.0, 0.0, -0.5])
            n, m = rng.randint(1, 160), rng.randint(1, 300)
            k = rng.choice([1, 1, 2, 3, 5, 10, rng.randint(1, m + 8), m, m + 3])
            prune = rng.random() < 0.75
            pattern = rng.choice(GROUP_PATTERNS)
            groups = draw_groups(rng, m, pattern)
            if family == "indel_raw_top_k_grouped":
                hi = rng.choice([4, 8, 30, 64, 64, 100, 128, 200, 256, 400, 512])
                alphabet = rng.choice(["ab", "abc", "abcdefgh ", "abcdefghijklmnopqrstuvwxyz0123456789 ", "".join(chr(0x100 + c) for c in range(150))])
                left = [rand_string(rng, alphabet, 0 if rng.random() < 0.2 else 1, hi) for _ in range(n)]
                right = [rand_string(rng, alphabet, 0 if rng.random() < 0.2 else 1, hi) for _ in range(m)]
                dup_some(rng, left, right, rng.choice([0.0, 0.1, 0.5]), lambda s_: "".join(s_))  # exact copies: ties
                lt, rt = tables.encode_strings(left, right, dev)
                cp = lambda ss: native.csr([[ord(c) for c in s_] for s_ in ss])
                thr = on_score(thr, lambda t: native.indel_raw(cp(left), cp(right), t, cap=n * m + 1))
                full = native.indel_raw(cp(left), cp(right), thr, cap=n * m + 1)
                what = f"{family} hi={hi} |alphabet|={len(alphabet)} thr={thr} k={k} prune={prune} groups={pattern} {n}x{m}"
                got = grid.indel_raw_top_k(lt, rt, k, thr, prune=prune, groups=groups)
            else:
                width = rng.choice([16, 16, 32, 64])
                kmax = rng.randint(1, width)
                vocab = rng.choice([kmax + 1, 3 * kmax, 50 * kmax])
                left_empty = rng.random() < 0.2
                left = rand_sets(rng, n, kmax, vocab, allow_empty=left_empty)
                right = rand_sets(rng, m, kmax, vocab, allow_empty=rng.random() < 0.2 and not left_empty)
                mutate = (lambda r: list(r)) if not any(not r for r in left) else (lambda r: list(r) or [0])
                dup_some(rng, left, right, rng.choice([0.0, 0.1, 0.5]), mutate)
                pad = lambda rr: np.array([r + [-1] * (width - len(r)) for r in rr], dtype=np.int32).reshape(len(rr), width)
                lt = tables.SetTable.from_padded(pad(left), "left", dev, width=width)
                rt = tables.SetTable.from_padded(pad(right), "right", dev, width=width)
                thr = on_score(thr, lambda t: native.jaccard_raw(native.csr(left), native.csr(right), t, cap=n * m + 1))
                full = native.jaccard_raw(native.csr(left), native.csr(right), thr, cap=n * m + 1)
                what = f"{family} W={width} kmax={kmax} vocab={vocab} thr={thr} k={k} prune={prune} groups={pattern} {n}x{m}"
                got = grid.jaccard_raw_top_k(lt, rt, k, thr, prune=prune, groups=groups)
            check(got, group_cut(full, groups.tolist(), k), what)
            continue
        if family in ("indel_top_k", "jaccard_top_k"):
            # per-item top-k (nsm_*_raw_top_k) against the definition: the oracle's threshold grid, cut per left item after
            # rank k in the order (score descending, j ascending).  Only through --family: the default draw is unchanged.
            thr = rng.choice(thresholds + [-1.0, 0.0, -0.5])
            n, m = rng.randint(1, 160), rng.randint(1, 300)
            k = rng.choice([1, 1, 2, 3, 5, 10, rng.randint(1, m + 8), m, m + 3])
            prune = rng.random() < 0.75
            if family == "indel_top_k":
                hi = rng.choice([4, 8, 30, 64, 64, 100, 128, 200, 256, 400, 512])
                alphabet = rng.choice(["ab", "abc", "abcdefgh ", "abcdefghijklmnopqrstuvwxyz0123456789 ", "".join(chr(0x100 + c) for c in range(150))])
                left = [rand_string(rng, alphabet, 0 if rng.random() < 0.2 else 1, hi) for _ in range(n)]
                right = [rand_string(rng, alphabet, 0 if rng.random() < 0.2 else 1, hi) for _ in range(m)]
                dup_some(rng, left, right, rng.choice([0.0, 0.1, 0.5]), lambda s_: "".join(s_))  # exact copies: ties
                lt, rt = tables.encode_strings(left, right, dev)
                cp = lambda ss: native.csr([[ord(c) for c in s_] for s_ in ss])
                thr = on_score(thr, lambda t: native.indel_raw(cp(left), cp(right), t, cap=n * m + 1))
                full = native.indel_raw(cp(left), cp(right), thr, cap=n * m + 1)
                what = f"indel_top_k hi={hi} |alphabet|={len(alphabet)} thr={thr} k={k} prune={prune} {n}x{m}"
                got = grid.indel_raw_top_k(lt, rt, k, thr, prune=prune)
            else:
                width = rng.choice([16, 16, 32, 64])
                kmax = rng.randint(1, width)
                vocab = rng.choice([kmax + 1, 3 * kmax, 50 * kmax])
                left_empty, right_empty = rng.random() < 0.2, rng.random() < 0.2
                left = rand_sets(rng, n, kmax, vocab, allow_empty=left_empty)
                right = rand_sets(rng, m, kmax, vocab, allow_empty=right_empty and not left_empty)
                dup_some(rng, left, right, rng.choice([0.0, 0.1, 0.5]), lambda r: list(r))
                pad = lambda rr: np.array([r + [-1] * (width - len(r)) for r in rr], dtype=np.int32).reshape(len(rr), width)
                lt = tables.SetTable.from_padded(pad(left), "left", dev, width=width)
                rt = tables.SetTable.from_padded(pad(right), "right", dev, width=width)
                what = f"jaccard_top_k W={width} kmax={kmax} vocab={vocab} thr={thr} k={k} prune={prune} {n}x{m}"
                if any(not r for r in left) and any(not r for r in right):  # (a copied empty row): the reference raises
                    try:
                        grid.jaccard_raw_top_k(lt, rt, k, thr, prune=prune)
                    except ZeroDivisionError:
                        continue
                    print(json.dumps({"FAIL": what + " (no ZeroDivisionError for empty x empty)", "round_seed": rnd}))
                    sys.exit(1)
                thr = on_score(thr, lambda t: native.jaccard_raw(native.csr(left), native.csr(right), t, cap=n * m + 1))
                full = native.jaccard_raw(native.csr(left), native.csr(right), thr, cap=n * m + 1)
                what = f"jaccard_top_k W={width} kmax={kmax} vocab={vocab} thr={thr} k={k} prune={prune} {n}x{m}"
                got = grid.jaccard_raw_top_k(lt, rt, k, thr, prune=prune)
            rows = {}
            for h in full:
                rows.setdefault(h[1], []).append(h)
            want = sorted((h for lst in rows.values() for h in sorted(lst, key=lambda t: (-t[0], t[2]))[:k]),
                          key=lambda t: (-t[0], t[1], t[2]))
            check(got, want, what)
            continue
        if family == "wide":
            # operands beyond the fast kernels through the plugin faces (only the wide items leave the fast path)
            from napkon_string_matching_amd.compare import score_functions as sf

            n, m = rng.randint(1, 60), rng.randint(1, 90)
            if rng.random() < 0.5:
                vocab = rng.choice([150, 3000])
                size = lambda: rng.randint(65, 140) if rng.random() < 0.15 else rng.randint(1, 40)
                left = [rng.sample(range(vocab), min(vocab, size())) for _ in range(n)]
                right = [rng.sample(range(vocab), min(vocab, size())) for _ in range(m)]
                dup_some(rng, left, right, 0.1, lambda r: list(dict.fromkeys(r[: max(1, len(r) - rng.randint(0, 3))] + [rng.randrange(vocab)])))
                thr = on_score(thr, lambda t: native.jaccard_raw(native.csr([sorted(set(r)) for r in left]), native.csr([sorted(set(r)) for r in right]), t, cap=1 << 16))
                want = native.jaccard_raw(native.csr([sorted(set(r)) for r in left]), native.csr([sorted(set(r)) for r in right]), thr, cap=1 << 16)
                names = lambda rows: [[f"t{v}" for v in r] for r in rows]
                check(sf.intersection_vs_union.raw_grid(names(left), names(right), thr), want, f"wide jaccard_raw vocab={vocab} thr={thr} {n}x{m}")
            else:
                alphabet = rng.choice(["abcdefgh ", "".join(chr(0x4E00 + k) for k in range(rng.choice([40, 300, 600])))])
                length = lambda: rng.randint(513, 1400) if rng.random() < 0.1 else rng.randint(0, 80)
                left = [rand_string(rng, alphabet, 0, length()) for _ in range(n)]
                right = [rand_string(rng, alphabet, 0, length()) for _ in range(m)]
                dup_some(rng, left, right, 0.1, lambda s_: ("".join(s_)[:-1] + rng.choice(alphabet)).strip())
                cp = lambda ss: native.csr([[ord(c) for c in sf.fuzzy_operand(s_)] for s_ in ss])
                thr = on_score(thr, lambda t: native.indel_raw(cp(left), cp(right), t, cap=1 << 16))
                want = native.indel_raw(cp(left), cp(right), thr, cap=1 << 16)
                check(sf.fuzzy_match.raw_grid(left, right, thr), want, f"wide indel_raw |alphabet|={len(alphabet)} thr={thr} {n}x{m}")
            continue
        if family == "jaccard_raw":
            width = rng.choice([16, 16, 32, 64])
            # the inverted-index kernel (low thresholds) on request too, and with several chunks of left rows per block
            # the right table's global inverted index (prefix filter) forced / chosen by the library, the per-tile LDS index
            # (W <= 32), or no index at all
            index = rng.choice([None, None, True, True, False] + (["tile"] if width < 64 else [])) if thr > 0 else None
            if index and rng.random() < 0.4:
                n = rng.randint(1500, 7000)
            kmax = rng.randint(1, width)
            vocab = rng.choice([kmax + 1, 3 * kmax, 50 * kmax, 100_000])
            left = rand_sets(rng, n, kmax, vocab, allow_empty=False)
            right = rand_sets(rng, m, kmax, vocab, allow_empty=rng.random() < 0.3)

            def mutate(r):
                if len(r) > 1 and rng.random() < 0.5:
                    r[rng.randrange(len(r))] = rng.randrange(vocab)
                return list(dict.fromkeys(r))

            dup_some(rng, left, right, 0.1, mutate)
            pad = lambda rr: np.array([r + [-1] * (width - len(r)) for r in rr], dtype=np.int32).reshape(len(rr), width)
            lt = tables.SetTable.from_padded(pad(left), "left", dev, width=width)
            rt = tables.SetTable.from_padded(pad(right), "right", dev, width=width)
            thr = on_score(thr, lambda t: native.jaccard_raw(native.csr(left), native.csr(right), t, cap=1 << 19))
            want = native.jaccard_raw(native.csr(left), native.csr(right), thr, cap=1 << 19)
            prune = rng.random() < 0.7
            check(grid.jaccard_raw_grid(lt, rt, thr, prune=prune, capacity=rng.choice([64, 4096, 1 << 16]), index=index), want,
                  f"jaccard_raw W={width} kmax={kmax} vocab={vocab} thr={thr} prune={prune} index={index} {n}x{m}")
        elif family == "indel_raw":
            hi = rng.choice([8, 30, 64, 64, 100, 128, 200, 256, 400, 512])
            alphabet = rng.choice(["ab", "abcdefgh ", "abcdefghijklmnopqrstuvwxyz0123456789 ", "".join(chr(0x100 + k) for k in range(150))])
            n, m = min(n, 200), min(m, 300)
            left = [rand_string(rng, alphabet, 0 if rng.random() < 0.2 else 1, hi) for _ in range(n)]
            right = [rand_string(rng, alphabet, 0 if rng.random() < 0.2 else 1, hi) for _ in range(m)]

            def mutate(s):
                s = "".join(s)
                if s and rng.random() < 0.7:
                    k = rng.randrange(len(s))
                    s = s[:k] + rng.choice(alphabet) + s[k + rng.randint(0, 1):]
                return s.strip()[:hi]

            dup_some(rng, left, right, 0.1, mutate)
            lt, rt = tables.encode_strings(left, right, dev)
            cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
            thr = on_score(thr, lambda t: native.indel_raw(cp(left), cp(right), t, cap=1 << 18))
            want = native.indel_raw(cp(left), cp(right), thr, cap=1 << 18)
            prune = rng.random() < 0.7
            two_stage = rng.random() < 0.7  # (64-unit tables: the 16-bucket first stage of the histogram filter, or not)
            check(grid.indel_raw_grid(lt, rt, thr, prune=prune, two_stage=two_stage), want,
                  f"indel_raw hi={hi} |alphabet|={len(alphabet)} thr={thr} prune={prune} two_stage={two_stage} {n}x{m}")
        else:
            ncat = rng.choice([0, 3, 6, 40, 64])
            mode = _lib.CAT_NONE if ncat == 0 else rng.choice([_lib.CAT_INTERSECT, _lib.CAT_INTERSECT_OR_BOTH_EMPTY])
            partition = rng.random() < 0.7

            def cats(k):
                out = np.zeros(k, dtype=np.uint64)
                for q in range(k):
                    for _ in range(rng.choice([0, 1, 1, 2, 3])):
                        out[q] |= np.uint64(1) << np.uint64(rng.randrange(max(1, ncat)))
                return out

            lcat, rcat = cats(n), cats(m)
            partition = partition and tables.partition_allowed(mode, lcat, rcat)
            if family == "jaccard_levels":
                vocab = rng.choice([12, 60, 400, 20_000])
                max_levels, max_new = rng.choice([1, 2, 4, 9, 20]), rng.choice([1, 2, 3, 8])
                left = [nested_item(rng, vocab, max_levels, max_new) for _ in range(n)]
                right = [nested_item(rng, vocab, max_levels, max_new) for _ in range(m)]
                dup_some(rng, left, right, 0.1, lambda it: [list(lv) for lv in (it[:-1] if len(it) > 1 and rng.random() < 0.5 else it)])
                biggest = max(len(it[-1]) for it in left + right)
                if biggest > 64:
                    continue
                width = tables.pick_width(biggest)
                vocabulary = tables.Vocabulary()
                lt = tables.SetTable.from_levels(left, "left", dev, vocabulary, width=width, categories=lcat, category_mode=mode,
                                                 partition=partition)
                rt = tables.SetTable.from_levels(right, "right", dev, vocabulary, width=width, categories=rcat, category_mode=mode,
                                                 partition=partition)
                thr = on_score(thr, lambda t: native.levels(False, left, right, t, lcat, rcat, mode, cap=1 << 19))
                want = native.levels(False, left, right, thr, lcat, rcat, mode, cap=1 << 19)
                # the inverted-index kernel forced / forbidden / chosen by the library (W <= 32, positive thresholds)
                index = rng.choice([None, True, True, False] + (["tile"] if width <= 32 else [])) if thr > 0 else None
                check(grid.jaccard_levels_grid(lt, rt, thr, category_mode=mode, index=index), want,
                      f"jaccard_levels vocab={vocab} levels<={max_levels} new<={max_new} W={width} thr={thr} mode={mode} "
                      f"partition={partition} ncat={ncat} index={index} {n}x{m}")
            else:
                n, m = min(n, 120), min(m, 200)
                lcat, rcat = lcat[:n], rcat[:m]
                hi = rng.choice([10, 40, 64, 64, 120, 250, 500])
                queue_cap = None
                if family == "indel_split":
                    # one-word strings at thresholds where the split path runs (scan -> survivor queue -> finish kernel),
                    # sometimes with a queue so small that it overflows (gated fused fallback)
                    hi = rng.choice([12, 30, 40, 64])
                    thr = rng.choice([0.7, 0.7, 0.75, 0.8, 0.9, 1.0])
                    queue_cap = rng.choice([None, None, 1024, 512 + 16 * 64, 512 + 16 * 2000])  # workspace bytes
                alphabet = rng.choice(["abc ", "abcdefghij klm", "abcdefghijklmnopqrstuvwxyz0123456789 "])
                max_levels = rng.choice([1, 2, 4, 4, 7])
                item = lambda: [rand_string(rng, alphabet, 0, hi) for _ in range(rng.randint(1, max_levels))]
                left, right = [item() for _ in range(n)], [item() for _ in range(m)]

                def mutate(it):
                    it = list(it)
                    k = rng.randrange(len(it))
                    it[k] = (it[k][:-1] + rng.choice(alphabet)).strip()
                    return it

                dup_some(rng, left, right, 0.1, mutate)
                li, ls, ri, rs = tables.encode_level_strings(left, right, dev, lcat, rcat, mode, partition=partition)
                cps = lambda items: [[[ord(c) for c in s] for s in it] for it in items]
                thr = on_score(thr, lambda t: native.levels(True, cps(left), cps(right), t, lcat, rcat, mode, cap=1 << 18))
                want = native.levels(True, cps(left), cps(right), thr, lcat, rcat, mode, cap=1 << 18)
                # multi-word strings: the shared-tile kernel (default) or the round-2 park kernel
                # (one-word strings: the split path at thresholds >= 0.7, else -- and with park -- the fused park kernel)
                park = rng.random() < 0.25 and family != "indel_split"
                prune = rng.random() < 0.8 or family == "indel_split"
                check(grid.indel_levels_grid(li, ls, ri, rs, thr, category_mode=mode, park=park, prune=prune, workspace=queue_cap), want,
                      f"{family} hi={hi} |alphabet|={len(alphabet)} levels<={max_levels} thr={thr} mode={mode} "
                      f"partition={partition} ncat={ncat} park={park} prune={prune} stride={ls.stride} queue_cap={queue_cap} {n}x{m}")
    print(json.dumps({"ok": True, "rounds": counts, "oracle_hits_compared": total_hits, "seconds": args.seconds,
                      "first_seed": args.seed + 1, "last_seed": rnd}))


if __name__ == "__main__":
    main()
