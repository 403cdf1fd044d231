"""Per-item top-k (nsm_*_raw_top_k) against the threshold grid plus a per-row selection.  Prints ONE JSON line.

    python tools/bench_top_k.py [--reps 20] [--c3 200000] [--term 20000] [--c2 50000]

Cases: synthetic.c3_corpus() fuzzy at k in {1, 10, 100} x thresholds {0, 0.5, 0.8}; Term-shaped fuzzy operands
(synthetic.term_cohort, the reference's default configuration) at 0.5; c2_corpus() Jaccard at {0, 0.1, 0.5}, k = 10.
Per case: ms per call (HIP events, after a warm-up), records, stats[0..3] / (N M), and -- where the threshold grid's hits
fit in 2^28 records, counted from its warm-up call -- the grid's own time (device grid, sort, copy of the hits to the host)
and, separately, the host-side per-row selection of those hits; else "n/a" and the bytes the hits would need.
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--c3", type=int, default=200_000)
    ap.add_argument("--term", type=int, default=20_000)
    ap.add_argument("--c2", type=int, default=50_000)
    args = ap.parse_args()
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
