"""Threshold grids of the token-set measures beside Jaccard (nsm_set_*_floor_grid without floors, include/nsm_hip_measures.h)
beside their two yardsticks on the same tables in the same run: NSM_MEASURE_UNION through the same per-item sweep (what the
sweep route costs a measure against Jaccard in the same kernel family) and the dedicated Jaccard grid nsm_jaccard_raw_grid /
nsm_jaccard_levels_grid (what the sweep route costs against the headline kernels).  Writes profiles/measures_bench.json and
prints it as ONE JSON line.

    python tools/bench_measures.py [--reps 5] [--window 0.5] [--c2 50000] [--term 20000] [--capacity 16777216]
                                   [--out profiles/measures_bench.json]

Cases: synthetic.c2_corpus() (RAW, W = 16) at thresholds 0.5 and 0.8; Term-shaped items (synthetic.term_cohort,
term_levels: 3..5 suffix-nested levels) in levels mode at 0.5.  Per case and route ``ms``: the C ENTRY itself into a hit
buffer allocated once (its counter reset inside the window, as every caller must), between two HIP events after a warm-up,
at least ``--reps`` calls and at least ``--window`` seconds of them; ``records``: what the entry counts (beyond
``--capacity`` the counter keeps counting and the records are dropped: the timing stands); ``stats_per_pair``: the sweep's
four counters per pair of the grid -- pairs in visited classes, pairs past the size bound, pairs past the signature bound,
exact intersections (levels: pairs visited, past the step-1 size bound, past the signature bound, scored exactly).  The
size bound is the measure's own: Dice prunes on sizes as Jaccard does, containment only downwards, overlap not at all.
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

ROUTES = (("mean", _lib.MEASURE_MEAN), ("smaller", _lib.MEASURE_SMALLER), ("left", _lib.MEASURE_LEFT),
          ("union_through_sweep", _lib.MEASURE_UNION))


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
    """One row: ``sweep(code, stats_ptr)`` launches the per-item floor grid without floors under measure ``code``,
    ``dedicated()`` the Jaccard threshold grid; both fill ``out``."""
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
    ms, calls = timed(lambda: run(dedicated), reps, window)
    row["routes"][dedicated_name] = {"ms": round(ms, 3), "calls": calls, "records": int(out.count.item())}
    assert row["routes"][dedicated_name]["records"] == row["routes"]["union_through_sweep"]["records"], "the two Jaccard routes disagree"
    union = row["routes"]["union_through_sweep"]["ms"]
    row["sweep_over_dedicated"] = round(union / ms, 3)
    row["measure_over_union_sweep"] = {label: round(row["routes"][label]["ms"] / union, 3) for label, _ in ROUTES[:3]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="least number of timed calls")
    ap.add_argument("--window", type=float, default=0.5, help="least length of a timed window, seconds")
    ap.add_argument("--c2", type=int, default=50_000)
    ap.add_argument("--term", type=int, default=20_000)
    ap.add_argument("--capacity", type=int, default=1 << 24, help="records of the hit buffer")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "measures_bench.json"))
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

    left, right = synthetic.c2_corpus(args.c2, args.c2)
    lt, rt = tables.SetTable.from_padded(left, "left", dev), tables.SetTable.from_padded(right, "right", dev)
    ls, rs = lt.struct(), rt.struct()
    for thr in (0.5, 0.8):
        add("c2_raw_w%d" % lt.width, thr, args.c2, args.c2,
            lambda code, st: _lib.check(lib.nsm_set_raw_floor_grid(ls, rs, code, thr, 0, 0, _lib.FLAG_PRUNE, *tail(st)), "sweep"),
            lambda: _lib.check(lib.nsm_jaccard_raw_grid(ls, rs, thr, _lib.FLAG_PRUNE, out.records.data_ptr(), out.capacity,
                                                        out.count.data_ptr(), stream), "grid"),
            "nsm_jaccard_raw_grid")

    a = synthetic.term_cohort(args.term, 7)
    b = synthetic.term_cohort(args.term, 8, plant_from=a)
    la, lb = synthetic.term_levels(a), synthetic.term_levels(b)
    vocab = tables.Vocabulary()
    width = tables.pick_width(max(len(it[-1]) for it in la), max(len(it[-1]) for it in lb))
    # the sweep's tables: an item is one row (no category partition), no inverted index; the dedicated grid's: its defaults
    sl = tables.SetTable.from_levels(la, "left", dev, vocab, width=width, partition=False, index=False)
    sr = tables.SetTable.from_levels(lb, "right", dev, vocab, width=width, partition=False, index=False)
    dl = tables.SetTable.from_levels(la, "left", dev, vocab, width=width)
    dr = tables.SetTable.from_levels(lb, "right", dev, vocab, width=width)
    sls, srs, dls, drs = sl.struct(), sr.struct(), dl.struct(), dr.struct()
    thr = 0.5
    add("term_levels_w%d" % width, thr, len(la), len(lb),
        lambda code, st: _lib.check(lib.nsm_set_levels_floor_grid(sls, srs, code, thr, 0, 0, _lib.CAT_NONE, _lib.FLAG_PRUNE, 0, 0,
                                                                  *tail(st)), "levels sweep"),
        lambda: _lib.check(lib.nsm_jaccard_levels_grid(dls, drs, thr, _lib.CAT_NONE, _lib.FLAG_PRUNE, out.records.data_ptr(),
                                                       out.capacity, out.count.data_ptr(), stream), "levels grid"),
        "nsm_jaccard_levels_grid")

    result = {"bench": "token-set measures: threshold grids through the per-item sweep vs the Jaccard routes",
              "device": torch.cuda.get_device_name(dev), "least_calls": args.reps, "least_window_s": args.window, "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
