"""Threshold profiles (nsm_*_raw_profile) against their yardstick, the top-k query nsm_*_raw_top_k at k = 100 and the
ladder's first threshold (at k = 100 the floors prune least).  Writes profiles/profile_bench.json and prints
it as ONE JSON line.

    python tools/bench_profile.py [--reps 20] [--window 0.5] [--c3 200000] [--term 20000] [--c2 50000]
                                  [--out profiles/profile_bench.json]

Cases: synthetic.c3_corpus() fuzzy with a 16-step ladder starting at 0.8, 0.5 and 0.0; Term-shaped fuzzy operands
(synthetic.term_cohort) starting at 0.5; c2_corpus() Jaccard starting at 0.1 and 0.5; and the tally's worst case, all 64
thresholds reached by nearly every score (C3 fuzzy, 64 steps from 0.0).

Two timings per case, both between two HIP events after a warm-up, at least ``--reps`` calls and at least ``--window``
seconds of them (a window of a few dozen milliseconds measures the clock):

* ``entry_ms``: the C ENTRIES themselves into buffers allocated once -- what the device does for one call: for the
  profile the init launch, the sweep and the finish launch; for top-k zeroing the counter and the sweep (its records stay
  unsorted).  In one process and alternating: top-k, the profile, top-k again.  The spread between the two top-k
  timings is the margin: a profile slower than top-k by more than that is a finding (``finding``: true), to be explained
  with the ``stats`` counters per pair that the row also holds.
* ``wrapper_ms``: the Python faces grid.*_profile and grid.*_top_k end to end -- allocations, the sizing reductions and
  the device-to-host copies of the profile; allocation, the counter's read-back, the device sort and the copy of the
  records for top-k.  Not a kernel time.
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

K = 100
STEPS = 16


def timed(fn, reps, window):
    """ms per call of ``fn`` and its last result: warm-up, then max(reps, window / one call) calls between two events."""
    fn()  # warm-up
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    calls = max(reps, math.ceil(window * 1e3 / max(start.elapsed_time(stop), 1e-3)))
    start.record()
    for _ in range(calls):
        out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls, calls, out


def ladder(first, steps=STEPS):
    return [first + (1.0 - first) * q / steps for q in range(steps)]


def case(name, lt, rt, n, m, kind, t, reps, window, yardstick=True):
    """One row.  ``kind``: "indel" or "jaccard".  Without ``yardstick`` only the profile is timed (the top-k figures of
    the row with the same first threshold apply)."""
    first = t[0]
    dev = lt.orig.device
    lib = _lib.load()
    top_entry, prof_entry = getattr(lib, f"nsm_{kind}_raw_top_k"), getattr(lib, f"nsm_{kind}_raw_profile")
    top_face, prof_face = getattr(grid, f"{kind}_raw_top_k"), getattr(grid, f"{kind}_raw_profile")
    ls, rs = lt.struct(), rt.struct()
    stream = torch.cuda.current_stream(dev).cuda_stream
    k_eff = min(K, m)

    pairs = torch.zeros(len(t), dtype=torch.int64, device=dev)
    left_best = torch.empty(int(lt.orig.max()) + 1, dtype=torch.float64, device=dev)
    right_best = torch.empty(int(rt.orig.max()) + 1, dtype=torch.float64, device=dev)
    lad = (ctypes.c_double * len(t))(*t)

    def profile_call():
        _lib.check(prof_entry(ls, rs, lad, len(t), _lib.FLAG_PRUNE, pairs.data_ptr(), left_best.data_ptr(), right_best.data_ptr(),
                              0, stream), "profile entry")

    row = {"case": name, "n": n, "m": m, "first_threshold": first, "thresholds": len(t)}
    if yardstick:
        buf = grid.HitBuffer(n * k_eff, dev)

        def top_call():
            buf.reset()
            _lib.check(top_entry(ls, rs, float(first), k_eff, _lib.FLAG_PRUNE, buf.records.data_ptr(), buf.count.data_ptr(), 0, stream),
                       "top-k entry")

        top_a, calls_a, _ = timed(top_call, reps, window)
    prof_ms, calls_p, _ = timed(profile_call, reps, window)
    entry_pairs = [int(v) for v in pairs.cpu().numpy().view("uint64")]
    if yardstick:
        top_b, calls_b, _ = timed(top_call, reps, window)
        spread = abs(top_a - top_b)
        row.update({"entry_ms": {"profile": round(prof_ms, 3), "top_k_100": [round(top_a, 3), round(top_b, 3)], "margin": round(spread, 3),
                                 "calls": [calls_a, calls_p, calls_b]},
                    "profile_over_top_k": round(prof_ms / (0.5 * (top_a + top_b)), 3),
                    "finding": bool(prof_ms > max(top_a, top_b) + spread)})
        del buf
    else:
        row["entry_ms"] = {"profile": round(prof_ms, 3), "calls": [calls_p]}

    st_top, st_prof = [], []
    prof_w, calls_pw, prof = timed(lambda: prof_face(lt, rt, t, stats=st_prof), reps, window)
    assert [int(v) for v in prof.pairs] == entry_pairs, "the entry and the Python face disagree"
    row["wrapper_ms"] = {"profile": round(prof_w, 3), "calls": [calls_pw]}
    if yardstick:
        top_w, calls_tw, _ = timed(lambda: top_face(lt, rt, K, first, stats=st_top), reps, window)
        row["wrapper_ms"].update({"top_k_100": round(top_w, 3), "calls": [calls_pw, calls_tw]})
        row["top_k_stats_per_pair"] = [v / (n * m) for v in st_top]
    row.update({"pairs": entry_pairs, "matched_left": prof.matched_left().tolist(),
                "profile_stats_per_pair": [v / (n * m) for v in st_prof]})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="least number of timed calls")
    ap.add_argument("--window", type=float, default=0.5, help="least length of a timed window, seconds")
    ap.add_argument("--c3", type=int, default=200_000)
    ap.add_argument("--term", type=int, default=20_000)
    ap.add_argument("--c2", type=int, default=50_000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "profile_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def add(*a, **kw):
        rows.append(case(*a, reps=args.reps, window=args.window, **kw))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    (lc, ll), (rc, rl) = synthetic.c3_corpus(args.c3, args.c3)
    alpha = len(synthetic.STRING_ALPHABET)
    lt, rt = tables.StrTable.from_codes(lc, ll, alpha, dev), tables.StrTable.from_codes(rc, rl, alpha, dev)
    for first in (0.8, 0.5, 0.0):
        add("c3_fuzzy", lt, rt, args.c3, args.c3, "indel", ladder(first))
    add("c3_fuzzy_64_steps", lt, rt, args.c3, args.c3, "indel", ladder(0.0, 64), yardstick=False)

    a = synthetic.term_cohort(args.term, 7)
    b = synthetic.term_cohort(args.term, 8, plant_from=a)
    la = [sf.fuzzy_operand(t) for it in synthetic.term_levels(a) for t in it[:1]]
    lb = [sf.fuzzy_operand(t) for it in synthetic.term_levels(b) for t in it[:1]]
    lt, rt = tables.encode_strings(la, lb, dev)
    add("term_fuzzy", lt, rt, len(la), len(lb), "indel", ladder(0.5))

    left, right = synthetic.c2_corpus(args.c2, args.c2)
    lt, rt = tables.SetTable.from_padded(left, "left", dev), tables.SetTable.from_padded(right, "right", dev)
    for first in (0.1, 0.5):
        add("c2_jaccard", lt, rt, args.c2, args.c2, "jaccard", ladder(first))

    result = {"bench": "threshold profiles vs top-k (k = 100)", "device": torch.cuda.get_device_name(dev),
              "least_calls": args.reps, "least_window_s": args.window, "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
