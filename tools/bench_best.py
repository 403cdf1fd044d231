"""Best matches (a profile sweep at T = 1, then nsm_*_raw_floor_grid with floor = best - margin) beside their two
yardsticks on the same tables in the same run: the top-k query at k = 1, which cuts ties in j order, and the profile sweep
alone.  Writes profiles/best_bench.json and prints it as ONE JSON line.

    python tools/bench_best.py [--reps 5] [--window 0.5] [--c3 200000] [--term 20000] [--c2 50000]
                               [--capacity 16777216] [--out profiles/best_bench.json]

Cases, all at threshold 0 and margin 0 -- every item's best match with all its ties, where the threshold grid is N M
records: synthetic.c3_corpus() fuzzy, Term-shaped fuzzy operands (synthetic.term_cohort), c2_corpus() Jaccard.  Each with
``mutual`` off (left floors only) and on (both floors).

Per case ``entry_ms``: the C ENTRIES themselves into buffers allocated once, between two HIP events after a warm-up, at
least ``--reps`` calls and at least ``--window`` seconds of them, in this order in one process: top-k (k = 1), the profile
sweep (pass 1), the floor grid with left floors (pass 2), the floor grid with both floors (pass 2, mutual), the profile
sweep again.  The spread between the two profile timings is the margin: a floor pass slower than the profile sweep by
more than that is a finding (``finding``: true) -- its bounds are compared against a value >= the profile's, so it should
not be -- to be explained with the four ``stats`` counters per pair that the row holds for every pass.  The floors are
formed on the device (``best - margin``, one float64 subtraction per item), outside the timed windows.  Every window
also holds its entry's fixed launches: the floor pass a memset of its counter and the sweep, the profile its init launch,
the sweep and its finish launch, top-k a memset and the sweep.  On a small case (Term) those launches are a visible share
of the call, so a ratio near 1 there says little about the sweeps themselves.  ``records``: what
the floor pass emits; a count beyond ``--capacity`` is reported as it is (the counter keeps counting; the timing stands).

``wrapper_ms``: the Python faces grid.*_raw_best end to end -- both sweeps, the copies of the bests to the host and of
the floors back, the device sort and the copy of the records.  Not a kernel time.
"""
import argparse
import ctypes
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "napkon-string-matching_amd")]

import torch  # noqa: E402

from napkon_string_matching_amd import _lib, grid, synthetic, tables  # noqa: E402
from napkon_string_matching_amd.compare import score_functions as sf  # noqa: E402

THRESHOLD, MARGIN = 0.0, 0.0


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


def case(name, lt, rt, n, m, kind, reps, window, capacity):
    """One row.  ``kind``: "indel" or "jaccard"."""
    dev = lt.orig.device
    lib = _lib.load()
    top_entry, prof_entry, floor_entry = (getattr(lib, f"nsm_{kind}_raw_{what}") for what in ("top_k", "profile", "floor_grid"))
    ls, rs = lt.struct(), rt.struct()
    stream = torch.cuda.current_stream(dev).cuda_stream
    per_pair = lambda st: [v / (n * m) for v in st.tolist()]

    pairs = torch.zeros(1, dtype=torch.int64, device=dev)
    left_best = torch.empty(int(lt.orig.max()) + 1, dtype=torch.float64, device=dev)
    right_best = torch.empty(int(rt.orig.max()) + 1, dtype=torch.float64, device=dev)
    lad = (ctypes.c_double * 1)(THRESHOLD)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    top = grid.HitBuffer(n, dev)
    out = grid.HitBuffer(capacity, dev)

    def top_call(st=0):
        top.reset()
        _lib.check(top_entry(ls, rs, THRESHOLD, 1, _lib.FLAG_PRUNE, top.records.data_ptr(), top.count.data_ptr(), st, stream), "top-k entry")

    def profile_call(st=0):
        _lib.check(prof_entry(ls, rs, lad, 1, _lib.FLAG_PRUNE, pairs.data_ptr(), left_best.data_ptr(), right_best.data_ptr(), st,
                              stream), "profile entry")

    def floor_call(lf, rf, st=0):
        out.reset()
        _lib.check(floor_entry(ls, rs, THRESHOLD, lf.data_ptr(), rf.data_ptr() if rf is not None else 0, _lib.FLAG_PRUNE,
                               out.records.data_ptr(), out.capacity, out.count.data_ptr(), st, stream), "floor grid entry")

    def counters(call):
        stats.zero_()
        call(stats.data_ptr())
        return per_pair(stats)  # (synchronises)

    top_ms, calls_t = timed(top_call, reps, window)
    prof_a, calls_a = timed(profile_call, reps, window)
    lf, rf = left_best - MARGIN, right_best - MARGIN
    one_ms, calls_1 = timed(lambda: floor_call(lf, None), reps, window)
    records_one = int(out.count.item())
    both_ms, calls_2 = timed(lambda: floor_call(lf, rf), reps, window)
    records_both = int(out.count.item())
    prof_b, calls_b = timed(profile_call, reps, window)
    spread = abs(prof_a - prof_b)
    row = {"case": name, "n": n, "m": m, "threshold": THRESHOLD, "margin": MARGIN,
           "entry_ms": {"top_k_1": round(top_ms, 3), "profile": [round(prof_a, 3), round(prof_b, 3)], "margin": round(spread, 3),
                        "floor_pass": round(one_ms, 3), "floor_pass_mutual": round(both_ms, 3),
                        "best": round(0.5 * (prof_a + prof_b) + one_ms, 3), "best_mutual": round(0.5 * (prof_a + prof_b) + both_ms, 3),
                        "calls": [calls_t, calls_a, calls_1, calls_2, calls_b]},
           "floor_over_profile": [round(one_ms / (0.5 * (prof_a + prof_b)), 3), round(both_ms / (0.5 * (prof_a + prof_b)), 3)],
           "finding": bool(max(one_ms, both_ms) > max(prof_a, prof_b) + spread),
           "records": {"top_k_1": int(top.count.item()), "best": records_one, "best_mutual": records_both, "capacity": capacity},
           "stats_per_pair": {"top_k_1": counters(top_call), "profile": counters(profile_call),
                              "floor_pass": counters(lambda st: floor_call(lf, None, st)),
                              "floor_pass_mutual": counters(lambda st: floor_call(lf, rf, st))}}
    del top, out
    face = getattr(grid, f"{kind}_raw_best")
    one_w, calls_w1 = timed(lambda: face(lt, rt, MARGIN, THRESHOLD, False), reps, window)
    both_w, calls_w2 = timed(lambda: face(lt, rt, MARGIN, THRESHOLD, True), reps, window)
    got = face(lt, rt, MARGIN, THRESHOLD, True)
    assert len(got) == records_both, "the entry and the Python face disagree"
    row["wrapper_ms"] = {"best": round(one_w, 3), "best_mutual": round(both_w, 3), "calls": [calls_w1, calls_w2]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="least number of timed calls")
    ap.add_argument("--window", type=float, default=0.5, help="least length of a timed window, seconds")
    ap.add_argument("--c3", type=int, default=200_000)
    ap.add_argument("--term", type=int, default=20_000)
    ap.add_argument("--c2", type=int, default=50_000)
    ap.add_argument("--capacity", type=int, default=1 << 24, help="records of the floor passes' hit buffer")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "best_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def add(*a):
        rows.append(case(*a, reps=args.reps, window=args.window, capacity=args.capacity))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    (lc, ll), (rc, rl) = synthetic.c3_corpus(args.c3, args.c3)
    alpha = len(synthetic.STRING_ALPHABET)
    lt, rt = tables.StrTable.from_codes(lc, ll, alpha, dev), tables.StrTable.from_codes(rc, rl, alpha, dev)
    add("c3_fuzzy", lt, rt, args.c3, args.c3, "indel")

    a = synthetic.term_cohort(args.term, 7)
    b = synthetic.term_cohort(args.term, 8, plant_from=a)
    la = [sf.fuzzy_operand(t) for it in synthetic.term_levels(a) for t in it[:1]]
    lb = [sf.fuzzy_operand(t) for it in synthetic.term_levels(b) for t in it[:1]]
    lt, rt = tables.encode_strings(la, lb, dev)
    add("term_fuzzy", lt, rt, len(la), len(lb), "indel")

    left, right = synthetic.c2_corpus(args.c2, args.c2)
    lt, rt = tables.SetTable.from_padded(left, "left", dev), tables.SetTable.from_padded(right, "right", dev)
    add("c2_jaccard", lt, rt, args.c2, args.c2, "jaccard")

    result = {"bench": "best matches (profile + floor grid) vs top-k (k = 1) and the profile sweep alone",
              "device": torch.cuda.get_device_name(dev), "least_calls": args.reps, "least_window_s": args.window, "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
