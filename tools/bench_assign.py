"""One-to-one assignment (nsm_assign_hits, include/nsm_hip_assign.h) on the bench workloads' hit lists, beside what it
replaces and what it is added to.  Writes profiles/assign_bench.json and prints it as ONE JSON line.

    python tools/bench_assign.py [--reps 3] [--c3 200000] [--term 20000] [--c2 50000] [--c5w 200000] [--same 2000]
                                 [--only NAME[,NAME]] [--out profiles/assign_bench.json]

Lists: C3's hits at 0.8 (RAW fuzzy_match), the Term workload at 0.5 (levels fuzzy_match), C2 at 0.5 and at 0.1 (RAW Jaccard,
tie-heavy), one cohort pair of c5w at 0.5 (levels fuzzy_match with categories), and an all-identical cohort of
``--same`` x ``--same`` strings (every pair scores 1: the all-ties worst case).

Per list, all on the same tables in one process, each figure the median of ``--reps`` calls after one warm-up call, wall
clock around a call that ends synchronised:
  grid_sort_d2h_ms   the grid wrapper as it was before this entry existed: grid, nsm_sort_hits, D2H of every hit
  entry_ms           nsm_assign_hits alone on the ordered device list, per route (default / rounds / stream), with the
                     ``stats`` it reports: [rounds, live at the stream stage, matches by rounds, matches by stream]
  device_path_ms     grid.*_assign end to end: grid, sort, assign, sort of the assignment, D2H of the assignment
  host_definition_ms grid.assign_of_hits on the host list (ONE run; what a consumer does today after grid_sort_d2h)
``rounds`` is skipped (null) where the default route's first round matched less than 1/1000 of the live records: the
all-ties lists, where rounds-only takes one round per match.
With a library built with -DNSM_ASSIGN_STATS (NSM_HIP_LIBRARY) ``atomics`` holds, for the default and the rounds route,
the atomics the propose launches issued and the proposals (live records summed over the rounds) behind them.  Every timed
wrapper call gets a buffer that holds the list, so no grid runs twice."""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "napkon-string-matching_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from napkon_string_matching_amd import _lib, grid, synthetic, tables  # noqa: E402
from napkon_string_matching_amd.compare import score_functions as sf  # noqa: E402

ROUTES = {"default": 0, "rounds": _lib.ASSIGN_ROUNDS_ONLY, "stream": _lib.ASSIGN_STREAM_ONLY}


def wall_ms(fn, reps, dev):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 3)


def atomics_counter():
    lib = _lib.load()
    if not hasattr(lib, "nsm_assign_atomics"):
        return None
    lib.nsm_assign_atomics.argtypes, lib.nsm_assign_atomics.restype = [ctypes.c_void_p], None

    def read():
        out = (ctypes.c_ulonglong * 2)()
        lib.nsm_assign_atomics(out)
        return int(out[0]), int(out[1])

    return read


def case(name, full, assign, left, right, reps, dev):
    """One row.  ``full(defer)``: the grid wrapper; ``assign(route, stats)``: the *_assign wrapper."""
    fn = _lib.entry("nsm_assign_hits")
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    pending = full(True)
    n = pending.n
    cap = n + 1  # (no retry in the timed calls)
    row = {"list": name, "records": n}
    row["grid_sort_d2h_ms"] = wall_ms(lambda: full(False, cap), reps, dev)
    ids_l, ids_r = int(left.orig[: left.n].max()) + 1, int(right.orig[: right.n].max()) + 1
    row["left_ids"], row["right_ids"] = ids_l, ids_r
    buf = pending.buf
    scratch = torch.empty((max(n, 1), 2), dtype=torch.float64, device=dev)
    _lib.check(lib.nsm_sort_hits(buf.records.data_ptr(), scratch.data_ptr(), buf.capacity, buf.count.data_ptr(), n,
                                 max(ids_l, ids_r), stream), "nsm_sort_hits")
    del scratch
    out = grid.HitBuffer(max(1, min(n, ids_l, ids_r)), dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)

    def entry(flags):
        out.reset()
        st.zero_()
        _lib.check(fn(buf.records.data_ptr(), n, ids_l, ids_r, flags, out.records.data_ptr(), out.count.data_ptr(),
                      st.data_ptr(), stream), "nsm_assign_hits")

    row["entry_ms"], row["stats"], counts = {}, {}, {}
    read_atomics = atomics_counter()
    if read_atomics:
        row["atomics"] = {}
    for route, flags in (("default", 0), ("stream", ROUTES["stream"]), ("rounds", ROUTES["rounds"])):
        if route == "rounds":
            first = row["stats"]["default"]
            tie_bound = first[0] >= 1 and first[2] * 1000 < n and first[1] > 0
            if tie_bound:
                row["entry_ms"][route], row["stats"][route] = None, None
                continue
        before = read_atomics() if read_atomics else None
        row["entry_ms"][route] = wall_ms(lambda: entry(flags), reps, dev)
        row["stats"][route] = [int(v) for v in st.tolist()]
        counts[route] = int(out.count.item())
        if read_atomics and route != "stream":
            after = read_atomics()
            calls = reps + 1
            issued, proposals = (after[0] - before[0]) // calls, (after[1] - before[1]) // calls
            row["atomics"][route] = {"issued": issued, "proposals": proposals, "per_proposal": round(issued / max(1, proposals), 4),
                                     "per_record": round(issued / max(1, n), 4)}
    assert len(set(counts.values())) == 1, f"{name}: the routes disagree on the number of matches: {counts}"
    row["matches"] = counts["default"]
    del out, pending, buf
    row["device_path_ms"] = wall_ms(lambda: assign(None, None, cap), reps, dev)
    hits = full(False, cap)
    t0 = time.perf_counter()
    want = grid.assign_of_hits(hits)
    row["host_definition_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    got = assign(None, None, cap)
    assert len(got) == len(want) == row["matches"] and np.array_equal(got.i, want.i) and np.array_equal(got.j, want.j) and \
        np.array_equal(got.score.view(np.int64), want.score.view(np.int64)), f"{name}: device and host disagree"
    row["added_share"] = round((row["device_path_ms"] - row["grid_sort_d2h_ms"]) / max(row["grid_sort_d2h_ms"], 1e-9), 3)
    return row


def c5w_tables(rows, dev):
    mode = _lib.CAT_INTERSECT_OR_BOTH_EMPTY
    lex = synthetic.word_vocabulary(20_000)
    hap = synthetic.c5_cohort(rows, 11, lex=lex)
    pop = synthetic.c5_cohort(rows, 12, plant_from=hap, lex=lex)
    alphabet = synthetic.c5_alphabet(hap)
    return tables.encode_level_codes(synthetic.c5_level_codes(hap), synthetic.c5_level_codes(pop), len(alphabet), dev, hap["cat"],
                                     pop["cat"], mode), mode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--c3", type=int, default=200_000)
    ap.add_argument("--term", type=int, default=20_000)
    ap.add_argument("--c2", type=int, default=50_000)
    ap.add_argument("--c5w", type=int, default=200_000)
    ap.add_argument("--same", type=int, default=2000)
    ap.add_argument("--only", default="", help="comma-separated list names (c3, term, c2, c2low, c5w, same)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "assign_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    only = set(filter(None, args.only.split(",")))
    want = lambda name: not only or name in only
    rows = []

    def add(name, full, assign, left, right):
        rows.append(case(name, full, assign, left, right, args.reps, dev))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    def raw(name, kind, lt, rt, thr):
        full_fn, assign_fn = (grid.indel_raw_grid, grid.indel_raw_assign) if kind == "indel" else \
            (grid.jaccard_raw_grid, grid.jaccard_raw_assign)
        add(name, lambda defer, cap=None: full_fn(lt, rt, thr, capacity=cap, defer=defer),
            lambda route, stats, cap=None: assign_fn(lt, rt, thr, capacity=cap, route=route, stats=stats), lt, rt)

    def levels(name, tabs, thr, mode):
        add(name, lambda defer, cap=None: grid.indel_levels_grid(*tabs, thr, category_mode=mode, capacity=cap, defer=defer),
            lambda route, stats, cap=None: grid.indel_levels_assign(*tabs, thr, category_mode=mode, capacity=cap, route=route,
                                                                    stats=stats), tabs[0], tabs[2])

    if want("c3"):
        (lc, ll), (rc, rl) = synthetic.c3_corpus(args.c3, args.c3)
        alpha = len(synthetic.STRING_ALPHABET)
        raw(f"c3 {args.c3}x{args.c3} at 0.8", "indel", tables.StrTable.from_codes(lc, ll, alpha, dev),
            tables.StrTable.from_codes(rc, rl, alpha, dev), 0.8)
    if want("term"):
        a = synthetic.term_cohort(args.term, 1234)
        b = synthetic.term_cohort(args.term, 5678, plant_from=a)
        ops = lambda items: [[sf.fuzzy_operand(lv) for lv in it] for it in synthetic.term_levels(items)]
        levels(f"term {args.term}x{args.term} at 0.5", tables.encode_level_strings(ops(a), ops(b), dev), 0.5, _lib.CAT_NONE)
    if want("c2") or want("c2low"):
        left, right = synthetic.c2_corpus(args.c2, args.c2)
        lt, rt = tables.SetTable.from_padded(left, "left", dev), tables.SetTable.from_padded(right, "right", dev)
        if want("c2"):
            raw(f"c2 {args.c2}x{args.c2} at 0.5", "jaccard", lt, rt, 0.5)
        if want("c2low"):
            raw(f"c2 {args.c2}x{args.c2} at 0.1", "jaccard", lt, rt, 0.1)
    if want("c5w"):
        tabs, mode = c5w_tables(args.c5w, dev)
        levels(f"c5w hap x pop {args.c5w}x{args.c5w} at 0.5", tabs, 0.5, mode)
    if want("same"):
        lt, rt = tables.encode_strings(["abcd efgh"] * args.same, ["abcd efgh"] * args.same, dev)
        raw(f"identical cohort {args.same}x{args.same} at 0.5", "indel", lt, rt, 0.5)

    result = {"bench": "one-to-one assignment of hit lists (nsm_assign_hits) vs the host definition and the grid it follows",
              "device": torch.cuda.get_device_name(dev), "reps": args.reps, "library": str(_lib.LIB_PATH.name), "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
