"""Threshold grids of the Levenshtein metrics (nsm_edit_*_floor_grid without floors, include/nsm_hip_edit.h) beside their two
yardsticks on the same tables in the same run: NSM_METRIC_INDEL through the same per-item sweep (what the distance costs
against the LCS in the same kernel family) and, for the RAW cases, the dedicated Indel grid nsm_indel_raw_grid (what the
sweep route costs against the headline kernel).  Writes profiles/edit_bench.json and prints it as ONE JSON line.

    python tools/bench_edit.py [--reps 3] [--window 0.3] [--c3 50000] [--term 10000] [--capacity 16777216]
                               [--out profiles/edit_bench.json]

Cases: synthetic.c3_corpus() (RAW, stride 64) at thresholds 0.8 and 0.9; the first-level strings of Term-shaped items
(synthetic.term_cohort, term_levels) as a RAW grid at 0.8; the same items in levels mode (3..5 level strings per item)
at 0.5, where the Indel yardstick is the sweep alone.  Per case and route ``ms``: the C ENTRY itself into a hit buffer
allocated once (its counter reset inside the window, as every caller must), between two HIP events after a warm-up, at
least ``--reps`` calls and at least ``--window`` seconds of them; ``records``: what the entry counts (beyond ``--capacity``
the counter keeps counting and the records are dropped: the timing stands); ``stats_per_pair``: the sweep's four counters
per pair of the grid -- pairs in visited classes, pairs past the length bound, pairs past the histogram bound, exact
distances (levels: pairs visited, past the step-1 length bound, past the histogram bound, scored exactly).  The occurrence
distance prunes towards shorter right strings only and has no histogram filter.
"""
import argparse
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "napkon-string-matching_amd")]

import torch  # noqa: E402

from napkon_string_matching_amd import _lib, grid, synthetic, tables  # noqa: E402
from napkon_string_matching_amd.compare import score_functions as sf  # noqa: E402

ROUTES = (("edit", _lib.METRIC_EDIT), ("edit_within", _lib.METRIC_EDIT_WITHIN), ("indel_through_sweep", _lib.METRIC_INDEL))


def timed(fn, reps, window):
    """ms per call of ``fn``: warm-up, then max(reps, window / one call) calls between two events."""
    fn()  # warm-up
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    calls = max(reps, math.ceil(window * 1e3 / max(start.elapsed_time(stop), 1e-3)))
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls, calls


def case(name, threshold, n, m, sweep, dedicated, dedicated_name, out, reps, window):
    """One row: ``sweep(code, stats_ptr)`` launches the per-item floor grid without floors under metric ``code``,
    ``dedicated()`` (or None) the Indel threshold grid; both fill ``out``."""
    dev = out.records.device
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    row = {"case": name, "n": n, "m": m, "threshold": threshold, "capacity": out.capacity, "routes": {}}

    def run(call):
        out.reset()
        call()

    for label, code in ROUTES:
        ms, calls = timed(lambda: run(lambda: sweep(code, 0)), reps, window)
        records = int(out.count.item())
        stats.zero_()
        run(lambda: sweep(code, stats.data_ptr()))
        row["routes"][label] = {"ms": round(ms, 3), "calls": calls, "records": records,
                                "stats_per_pair": [v / (n * m) for v in stats.tolist()]}
    indel = row["routes"]["indel_through_sweep"]["ms"]
    if dedicated is not None:
        ms, calls = timed(lambda: run(dedicated), reps, window)
        row["routes"][dedicated_name] = {"ms": round(ms, 3), "calls": calls, "records": int(out.count.item())}
        assert row["routes"][dedicated_name]["records"] == row["routes"]["indel_through_sweep"]["records"], "the two Indel routes disagree"
        row["sweep_over_dedicated"] = round(indel / ms, 3)
    row["metric_over_indel_sweep"] = {label: round(row["routes"][label]["ms"] / indel, 3) for label, _ in ROUTES[:2]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="least number of timed calls")
    ap.add_argument("--window", type=float, default=0.3, help="least length of a timed window, seconds")
    ap.add_argument("--c3", type=int, default=50_000)
    ap.add_argument("--term", type=int, default=10_000)
    ap.add_argument("--capacity", type=int, default=1 << 24, help="records of the hit buffer")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "edit_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = grid.HitBuffer(args.capacity, dev)
    tail = lambda st: (out.records.data_ptr(), out.capacity, out.count.data_ptr(), st, stream)
    rows = []

    def add(*a):
        rows.append(case(*a, out, args.reps, args.window))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    def raw_case(name, lt, rt, thr, n, m):
        ls, rs = lt.struct(), rt.struct()
        add(name, thr, n, m,
            lambda code, st: _lib.check(lib.nsm_edit_raw_floor_grid(ls, rs, code, thr, 0, 0, _lib.FLAG_PRUNE, *tail(st)), "sweep"),
            lambda: _lib.check(lib.nsm_indel_raw_grid(ls, rs, thr, _lib.FLAG_PRUNE, out.records.data_ptr(), out.capacity,
                                                      out.count.data_ptr(), stream), "grid"),
            "nsm_indel_raw_grid")

    (lc, ll), (rc, rl) = synthetic.c3_corpus(args.c3, args.c3)
    alpha = len(synthetic.STRING_ALPHABET)
    lt, rt = tables.StrTable.from_codes(lc, ll, alpha, dev), tables.StrTable.from_codes(rc, rl, alpha, dev)
    for thr in (0.8, 0.9):
        raw_case("c3_raw_s%d" % lt.stride, lt, rt, thr, args.c3, args.c3)

    a = synthetic.term_cohort(args.term, 7)
    b = synthetic.term_cohort(args.term, 8, plant_from=a)
    ops = lambda items: [[sf.fuzzy_operand(lv) for lv in it] for it in synthetic.term_levels(items)]
    la, lb = ops(a), ops(b)
    lt, rt = tables.encode_strings([it[0] for it in la], [it[0] for it in lb], dev)
    raw_case("term_raw_s%d" % lt.stride, lt, rt, 0.8, len(la), len(lb))

    # levels mode: the sweep's tables (an item is one row, no category partition); the Indel yardstick is the same sweep
    li, ls, ri, rs = tables.encode_level_strings(la, lb, dev, partition=False)
    lis, lss, ris, rss = li.struct(), ls.struct(), ri.struct(), rs.struct()
    thr = 0.5
    add("term_levels_s%d" % ls.stride, thr, len(la), len(lb),
        lambda code, st: _lib.check(lib.nsm_edit_levels_floor_grid(lis, lss, ris, rss, code, thr, 0, 0, _lib.CAT_NONE,
                                                                   _lib.FLAG_PRUNE, 0, 0, *tail(st)), "levels sweep"),
        None, None)

    result = {"bench": "Levenshtein metrics: threshold grids through the per-item sweep vs the Indel routes",
              "device": torch.cuda.get_device_name(dev), "least_calls": args.reps, "least_window_s": args.window, "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
