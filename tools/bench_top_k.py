"""Per-item top-k (nsm_*_raw_top_k) against the threshold grid plus a per-row selection.  Prints ONE JSON line.

    python tools/bench_top_k.py [--reps 20] [--c3 200000] [--term 20000] [--c2 50000]
    python tools/bench_top_k.py --levels [--reps 5] [--term 20000] [--c5w 100000]
    python tools/bench_top_k.py --grouped [--reps 20] [--c3 200000] [--term 20000] [--syn 200000]

Cases: synthetic.c3_corpus() fuzzy at k in {1, 10, 100} x thresholds {0, 0.5, 0.8}; Term-shaped fuzzy operands
(synthetic.term_cohort, the reference's default configuration) at 0.5; c2_corpus() Jaccard at {0, 0.1, 0.5}, k = 10.
Per case: ms per call (HIP events, after a warm-up), records, stats[0..3] / (N M), and -- where the threshold grid's hits
fit in 2^28 records, counted from its warm-up call -- the grid's own time (device grid, sort, copy of the hits to the host)
and, separately, the host-side per-row selection of those hits; else "n/a" and the bytes the hits would need.

--levels: the levels-mode queries (nsm_*_levels_top_k) instead: Term-shaped items (compare_terms x fuzzy_match, the
reference's default configuration) at 0.5 and 0 with k in {1, 10}; a c5w-shaped grid (configs[4] on word-like text, list
categories) at 0.5 and 0, k = 10, for both score functions; and ComparableData.compare(..., top_k=10) end to end against
compare() on Term-shaped cohorts (one call each, wall clock).

--grouped: the grouped queries (nsm_indel_raw_top_k_grouped).  (a) c3_corpus() at k = 10, thresholds 0.8 / 0.5 / 0 with
identity groups and with groups j // 8, the ungrouped nsm_indel_raw_top_k beside them in the same process, the three calls
alternating; per call the median and the min .. max of its per-call times (the ungrouped spread is the yardstick of the
ratios).  (b) a terminology-shaped case: --term Term-shaped items against --syn synonym-like rows whose Ids have a skewed
multiplicity (most 1-10 rows, a few several hundred), limit = 10 at threshold 0.1 through the grouped query, next to what
get_matches_batch(limit=10) needed before it: limit x (most rows of one Id) rows per item, or -- beyond 4096 -- the
threshold grid, whose records are counted on a sample of the left items.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "napkon-string-matching_amd")]

import torch  # noqa: E402

from napkon_string_matching_amd import grid, synthetic, tables  # noqa: E402
from napkon_string_matching_amd.compare import score_functions as sf  # noqa: E402

GRID_MAX_RECORDS = 1 << 28


def timed(fn, reps, warm=True):
    if warm:
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps, out


def case(name, lt, rt, n, m, top_k, raw_grid, k, thr, reps):
    st = []
    ms, hits = timed(lambda: top_k(lt, rt, k, thr, stats=st), reps)
    row = {"case": name, "k": k, "threshold": thr, "n": n, "m": m, "top_k_ms": round(ms, 3), "records": len(hits),
           "stats_per_pair": [v / (n * m) for v in st]}
    if thr <= 0:  # every pair is a hit
        row["grid_ms"] = "n/a"
        row["grid_bytes"] = n * m * grid.HIT_BYTES
        return row
    # the grid is timed only where its hits fit; their number comes from the warm-up call
    grid_hits = raw_grid(lt, rt, thr)
    row["grid_hits"] = len(grid_hits)
    if len(grid_hits) > GRID_MAX_RECORDS:
        row["grid_ms"] = "n/a"
        row["grid_bytes"] = len(grid_hits) * grid.HIT_BYTES
        return row
    gms, grid_hits = timed(lambda: raw_grid(lt, rt, thr), max(3, reps // 4), warm=False)
    t0 = time.perf_counter()
    selected = grid.select_top_k(grid_hits, k)
    sms = (time.perf_counter() - t0) * 1e3
    row["grid_ms"] = round(gms, 3)  # device grid, canonical sort and the copy of its hits to the host
    row["host_select_ms"] = round(sms, 3)  # the per-row cut of those hits (numpy, on the host)
    row["same_records"] = selected.as_tuples() == hits.as_tuples()
    return row


def levels_case(name, run_top_k, run_grid, n, m, k, thr, reps):
    """``case`` for the levels queries: ``run_top_k(k, thr, stats)`` / ``run_grid(thr)`` close over their tables."""
    return case(name, None, None, n, m, lambda _l, _r, kk, t, stats: run_top_k(kk, t, stats),
                lambda _l, _r, t: run_grid(t), k, thr, reps)


def term_frame(items, prefix):
    import pandas as pd

    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    rows = [{"Identifier": f"{prefix}{q}", "Variable": f"v{q}", "Sheet": "s", "Category": ["c"], "Term": it,
             "Tokens": [], "Parameter": ""} for q, it in enumerate(items)]
    return Questionnaire(pd.DataFrame(rows))


def main_levels(args) -> None:
    dev = torch.device("cuda:0")
    rows = []
    a = synthetic.term_cohort(args.term, 1234)
    b = synthetic.term_cohort(args.term, 5678, plant_from=a)
    la = [[sf.fuzzy_operand(lv) for lv in it] for it in synthetic.term_levels(a)]
    lb = [[sf.fuzzy_operand(lv) for lv in it] for it in synthetic.term_levels(b)]
    tabs = tables.encode_level_strings(la, lb, dev, partition=False)
    for thr in (0.5, 0.0):
        for k in (1, 10):
            rows.append(levels_case("term_levels_fuzzy", lambda kk, t, st: grid.indel_levels_top_k(*tabs, kk, t, stats=st),
                                    lambda t: grid.indel_levels_grid(*tabs, t), args.term, args.term, k, thr, args.reps))

    lex = synthetic.word_vocabulary()
    hap = synthetic.c5_cohort(args.c5w, 3, lex=lex)
    pop = synthetic.c5_cohort(args.c5w, 4, plant_from=hap, lex=lex)
    mode = 2  # list x list categories: "intersect, or both empty"
    cps = tables.encode_level_codes(synthetic.c5_level_codes(hap), synthetic.c5_level_codes(pop), len(synthetic.WORD_ALPHABET),
                                    dev, hap["cat"], pop["cat"], mode, partition=False)
    ptabs = tables.encode_level_codes(synthetic.c5_level_codes(hap), synthetic.c5_level_codes(pop), len(synthetic.WORD_ALPHABET),
                                      dev, hap["cat"], pop["cat"], mode)  # (the grid's own, partitioned layout)
    st_l = tables.SetTable.from_nested_arrays(hap["ids"], hap["plen"], hap["nlev"], "left", dev, categories=hap["cat"],
                                              category_mode=mode, partition=False, index=False)
    st_r = tables.SetTable.from_nested_arrays(pop["ids"], pop["plen"], pop["nlev"], "right", dev, categories=pop["cat"],
                                              category_mode=mode, partition=False, index=False)
    sp_l = tables.SetTable.from_nested_arrays(hap["ids"], hap["plen"], hap["nlev"], "left", dev, categories=hap["cat"],
                                              category_mode=mode)
    sp_r = tables.SetTable.from_nested_arrays(pop["ids"], pop["plen"], pop["nlev"], "right", dev, categories=pop["cat"],
                                              category_mode=mode)
    for thr in (0.5, 0.0):
        rows.append(levels_case("c5w_levels_fuzzy", lambda kk, t, st: grid.indel_levels_top_k(*cps, kk, t, category_mode=mode,
                                                                                             stats=st),
                                lambda t: grid.indel_levels_grid(*ptabs, t, category_mode=mode), args.c5w, args.c5w, 10, thr,
                                args.reps))
        rows.append(levels_case("c5w_levels_jaccard", lambda kk, t, st: grid.jaccard_levels_top_k(st_l, st_r, kk, t,
                                                                                                 category_mode=mode, stats=st),
                                lambda t: grid.jaccard_levels_grid(sp_l, sp_r, t, category_mode=mode), args.c5w, args.c5w, 10,
                                thr, args.reps))

    # end to end: the public API on Term-shaped cohorts, the reference's default configuration at 0.5
    left, right = term_frame(a, "hap"), term_frame(b, "pop")
    kw = dict(score_func="fuzzy_match", compare_column="Term", left_name="hap", right_name="pop", score_threshold=0.5,
              cached=False)
    e2e = {"case": "term_compare", "n": args.term, "m": args.term, "score_threshold": 0.5}
    left.compare(right, None, None, top_k=10, **kw)  # (warm-up: library, encoders)
    for label, extra in (("compare_top_k10", {"top_k": 10}), ("compare", {})):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = left.compare(right, None, None, **kw, **extra)
        e2e[label + "_s"] = round(time.perf_counter() - t0, 3)
        e2e[label + "_rows"] = len(got)
    rows.append(e2e)
    print(json.dumps({"bench": "top_k_levels", "device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": rows}))


def per_call_ms(fns, reps):
    """The calls of ``fns`` alternating, ``reps`` rounds after one warm-up round: per call the list of its times (ms)."""
    for fn in fns:
        fn()
    times = [[] for _ in fns]
    for _ in range(reps):
        for q, fn in enumerate(fns):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[q].append(start.elapsed_time(stop))
    return times


def spread(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def skewed_ids(rng, m):
    """Ids of m synonym rows: most Ids have 1-10 rows, about one in 500 has 200-600 (rows of an Id are scattered)."""
    import numpy as np

    ids, q = [], 0
    while len(ids) < m:
        rows = int(rng.integers(200, 601)) if rng.random() < 0.002 else int(rng.integers(1, 11))
        ids += [q] * rows
        q += 1
    ids = np.array(ids[:m], dtype=np.int32)
    rng.shuffle(ids)
    return ids


def main_grouped(args) -> None:
    import numpy as np

    dev = torch.device("cuda:0")
    rows = []
    (lc, ll), (rc, rl) = synthetic.c3_corpus(args.c3, args.c3)
    alpha = len(synthetic.STRING_ALPHABET)
    lt, rt = tables.StrTable.from_codes(lc, ll, alpha, dev), tables.StrTable.from_codes(rc, rl, alpha, dev)
    identity = torch.arange(args.c3, dtype=torch.int32, device=dev)
    eights = (torch.arange(args.c3, dtype=torch.int32, device=dev) // 8).contiguous()
    k = 10
    for thr in (0.8, 0.5, 0.0):
        stats = [[], [], []]
        outs = [None, None, None]

        def call(q, groups):
            def fn():
                outs[q] = grid.indel_raw_top_k(lt, rt, k, thr, stats=stats[q], groups=groups)
            return fn

        times = per_call_ms([call(0, None), call(1, identity), call(2, eights)], args.reps)
        base = spread(times[0])
        row = {"case": "c3_fuzzy", "k": k, "threshold": thr, "n": args.c3, "m": args.c3, "ungrouped": base}
        for q, label in ((1, "grouped_identity"), (2, "grouped_j_div_8")):
            row[label] = dict(spread(times[q]), ratio_to_ungrouped=round(spread(times[q])["median_ms"] / base["median_ms"], 4),
                              records=len(outs[q]), stats_per_pair=[v / (args.c3 * args.c3) for v in stats[q]])
        row["ungrouped"]["records"] = len(outs[0])
        row["ungrouped"]["stats_per_pair"] = [v / (args.c3 * args.c3) for v in stats[0]]
        row["identity_same_records"] = outs[0].as_tuples() == outs[1].as_tuples()
        rows.append(row)

    # (b) terminology-shaped: Term-shaped items against synonym-like rows with skewed Ids
    rng = np.random.default_rng(42)
    a = synthetic.term_cohort(args.term, 7)
    b = synthetic.term_cohort(args.syn, 8, plant_from=a)
    la = [sf.fuzzy_operand(t) for it in synthetic.term_levels(a) for t in it[:1]]
    lb = [sf.fuzzy_operand(t) for it in synthetic.term_levels(b) for t in it[:1]]
    ids = skewed_ids(rng, len(lb))
    most = int(np.bincount(ids).max())
    limit, thr = 10, 0.1
    lt, rt = tables.encode_strings(la, lb, dev)
    st = []
    out = [None]

    def grouped():
        out[0] = grid.indel_raw_top_k(lt, rt, limit, thr, stats=st, groups=ids)

    ts = per_call_ms([grouped], max(3, args.reps // 4))[0]
    n, m = len(la), len(lb)
    row = {"case": "terminology", "limit": limit, "threshold": thr, "n": n, "m": m, "distinct_ids": int(ids.max()) + 1,
           "most_rows_of_one_id": most,
           "grouped": dict(spread(ts), records=len(out[0]), bound_records=n * limit, stats_per_pair=[v / (n * m) for v in st])}
    need = limit * most  # rows per item the ungrouped route asks for
    if min(need, m) <= grid.TOP_K_MAX:
        st2 = []
        ts2 = per_call_ms([lambda: out.__setitem__(0, grid.indel_raw_top_k(lt, rt, need, thr, stats=st2))], 3)[0]
        row["before"] = dict(spread(ts2), route=f"top-k of {need} rows per item + host loop", records=len(out[0]))
    else:
        sample = np.sort(rng.choice(n, min(n, 200), replace=False))
        ls, rs = tables.encode_strings([la[q] for q in sample], lb, dev)
        hits = grid.indel_raw_grid(ls, rs, thr, capacity=len(sample) * m + 1)
        per_item = len(hits) / len(sample)
        row["before"] = {"route": f"{need} rows per item exceed {grid.TOP_K_MAX}: the threshold grid", "time": "n/a",
                         "sampled_left_items": int(len(sample)), "grid_records_per_item": round(per_item, 1),
                         "grid_records": int(per_item * n), "grid_bytes": int(per_item * n) * grid.HIT_BYTES}
    rows.append(row)
    print(json.dumps({"bench": "top_k_grouped", "device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": rows}))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--c3", type=int, default=200_000)
    ap.add_argument("--term", type=int, default=20_000)
    ap.add_argument("--c2", type=int, default=50_000)
    ap.add_argument("--levels", action="store_true", help="the levels-mode queries instead (see above)")
    ap.add_argument("--c5w", type=int, default=100_000)
    ap.add_argument("--grouped", action="store_true", help="the grouped queries instead (see above)")
    ap.add_argument("--syn", type=int, default=200_000, help="synonym rows of the terminology case (--grouped)")
    args = ap.parse_args()
    if args.levels:
        return main_levels(args)
    if args.grouped:
        return main_grouped(args)
    dev = torch.device("cuda:0")
    rows = []

    (lc, ll), (rc, rl) = synthetic.c3_corpus(args.c3, args.c3)
    alpha = len(synthetic.STRING_ALPHABET)
    lt, rt = tables.StrTable.from_codes(lc, ll, alpha, dev), tables.StrTable.from_codes(rc, rl, alpha, dev)
    for thr in (0.0, 0.5, 0.8):
        for k in (1, 10, 100):
            rows.append(case("c3_fuzzy", lt, rt, args.c3, args.c3, grid.indel_raw_top_k, grid.indel_raw_grid, k, thr, args.reps))

    a = synthetic.term_cohort(args.term, 7)
    b = synthetic.term_cohort(args.term, 8, plant_from=a)
    la = [sf.fuzzy_operand(t) for it in synthetic.term_levels(a) for t in it[:1]]
    lb = [sf.fuzzy_operand(t) for it in synthetic.term_levels(b) for t in it[:1]]
    lt, rt = tables.encode_strings(la, lb, dev)
    for k in (1, 10):
        rows.append(case("term_fuzzy", lt, rt, len(la), len(lb), grid.indel_raw_top_k, grid.indel_raw_grid, k, 0.5, args.reps))

    left, right = synthetic.c2_corpus(args.c2, args.c2)
    lt, rt = tables.SetTable.from_padded(left, "left", dev), tables.SetTable.from_padded(right, "right", dev)
    for thr in (0.0, 0.1, 0.5):
        rows.append(case("c2_jaccard", lt, rt, args.c2, args.c2, grid.jaccard_raw_top_k, grid.jaccard_raw_grid, 10, thr, args.reps))

    print(json.dumps({"bench": "top_k", "device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": rows}))


if __name__ == "__main__":
    main()
