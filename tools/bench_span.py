"""Merge forests (nsm_span_hits, include/nsm_hip_span.h) on the bench workloads' hit lists, beside the one-threshold answer
(nsm_group_hits), the host route and the grid it follows.  Writes profiles/span_bench.json and prints it as ONE JSON line.

    python tools/bench_span.py [--reps 3] [--c3 200000] [--term 20000] [--c2 50000] [--c5w 200000] [--same 2000]
                               [--only NAME[,NAME]] [--skip-host] [--out profiles/span_bench.json]

Lists (the ones tools/bench_groups.py uses): C3's hits at 0.8 (RAW fuzzy_match), the Term workload at 0.5 (levels
fuzzy_match), C2 at 0.5 and at 0.1 (RAW Jaccard), one cohort pair of c5w at 0.5 (levels fuzzy_match with categories), and an
all-identical cohort of ``--same`` x ``--same`` strings (every score equal: ties decide everything).

Per list, all on the same tables in one process, each figure the median of ``--reps`` calls after one warm-up call, wall
clock around a call that ends synchronised:
  grid_ms            the grid alone, its hits left unsorted in their device buffer
  entry_ms           nsm_span_hits alone on that buffer (two cohorts: left ids, then right ids), labels included, with the
                     ``stats`` it reports: [records with score >= min_score, forest records, rounds, edge visits]
  order_ms           nsm_sort_hits alone on a copy of the records (id_limit = the larger cohort): what the entry's gather +
                     order stage costs at least; ``order_share`` = order_ms / entry_ms
  group_entry_ms     nsm_group_hits on the same buffer: the ONE-threshold answer; ``entry_vs_group`` = entry_ms /
                     group_entry_ms is the ladder length from which one forest beats a sweep of groups calls
  device_path_ms     grid.*_forest end to end: grid, nsm_span_hits, nsm_sort_hits on the forest, D2H of the forest
  host_route_ms      what a consumer does without the entry: D2H of the unsorted list (``d2h_ms``) plus
                     grid.forest_of_hits on the host (``host_definition_ms``, ONE run)
  scipy_ms           scipy.sparse.csgraph.minimum_spanning_tree on negated scores (duplicates summed away first by taking
                     the maximum per pair), where scipy is importable: for scale only, its tie-break is not the canonical one
``entry_vs_host`` = host_route_ms / entry_ms, ``entry_vs_grid`` = entry_ms / grid_ms.  Every timed wrapper call gets a
buffer that holds the list, so no grid runs twice."""
import argparse
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


def case(name, full, forest_fn, left, right, reps, dev, skip_host=False):
    """One row.  ``full(defer, cap)``: the grid wrapper; ``forest_fn(cap)``: the *_forest wrapper."""
    span, group, lib = _lib.entry("nsm_span_hits"), _lib.entry("nsm_group_hits"), _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    pending = full(True)
    n = pending.n
    cap = n + 1  # (no retry in the timed calls)
    ids_l, ids_r = int(left.orig[: left.n].max()) + 1, int(right.orig[: right.n].max()) + 1
    nodes = ids_l + ids_r
    row = {"list": name, "records": n, "left_ids": ids_l, "right_ids": ids_r, "nodes": nodes}
    row["grid_ms"] = wall_ms(lambda: full(True, cap), reps, dev)
    buf = pending.buf
    out = grid.HitBuffer(nodes - 1, dev)
    label = torch.empty(nodes, dtype=torch.int32, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    lists = (_lib.NsmHitList * 1)(_lib.NsmHitList(buf.records.data_ptr() if n else None, n, 0, ids_l, ids_l, ids_r))

    def entry():
        st.zero_()
        out.reset()
        _lib.check(span(lists, 1, nodes, float("-inf"), 0, out.records.data_ptr(), out.count.data_ptr(), label.data_ptr(),
                        st.data_ptr(), stream), "nsm_span_hits")

    row["entry_ms"] = wall_ms(entry, reps, dev)
    row["stats"] = [int(v) for v in st.tolist()]
    device_label = label.cpu().numpy()

    # the order stage for scale: the library's sort on a copy of the records
    copy = grid.HitBuffer(max(1, n), dev)
    scratch = torch.empty((max(1, n), 2), dtype=torch.float64, device=dev)

    def order():
        copy.records[:n] = buf.records[:n]
        copy.count.fill_(n)
        _lib.check(lib.nsm_sort_hits(copy.records.data_ptr(), scratch.data_ptr(), copy.capacity, copy.count.data_ptr(), n,
                                     max(ids_l, ids_r), stream), "nsm_sort_hits")

    def copy_only():
        copy.records[:n] = buf.records[:n]
        copy.count.fill_(n)

    if n:
        row["order_ms"] = round(max(0.0, wall_ms(order, reps, dev) - wall_ms(copy_only, reps, dev)), 3)
        row["order_share"] = round(row["order_ms"] / max(row["entry_ms"], 1e-9), 3)

    gst = torch.zeros(2, dtype=torch.int64, device=dev)
    glabel = torch.empty(nodes, dtype=torch.int32, device=dev)

    def group_entry():
        gst.zero_()
        _lib.check(group(lists, 1, nodes, float("-inf"), 0, glabel.data_ptr(), gst.data_ptr(), stream), "nsm_group_hits")

    row["group_entry_ms"] = wall_ms(group_entry, reps, dev)
    assert np.array_equal(glabel.cpu().numpy(), device_label), f"{name}: the forest's labels are not the groups'"
    row["entry_vs_group"] = round(row["entry_ms"] / max(row["group_entry_ms"], 1e-9), 1)
    row["device_path_ms"] = wall_ms(lambda: forest_fn(cap), reps, dev)
    row["entry_vs_grid"] = round(row["entry_ms"] / max(row["grid_ms"], 1e-9), 3)
    got = forest_fn(cap)
    row["forest_records"] = len(got)
    assert row["stats"][:2] == [n, len(got)], f"{name}: stats {row['stats']}"
    if len(got):
        ts = np.linspace(float(got.score.min()), float(got.score.max()), 8)
        ladder = got.ladder(ts)
        row["ladder"] = {"thresholds": [round(float(t), 4) for t in ts], **{k: v.tolist() for k, v in ladder.items()}}
    if skip_host:
        return row

    # the host route: the list crosses to the host as it lies in the buffer, then sort + union-find in Python
    def d2h():
        host = buf.records[:n].cpu().numpy()
        ij = host.view(np.int32).reshape(n, 4)
        return grid.Hits(host[:, 0].copy(), ij[:, 2].copy(), ij[:, 3].copy())

    row["d2h_ms"] = wall_ms(d2h, reps, dev)
    hits = d2h()
    t0 = time.perf_counter()
    want = grid.forest_of_hits([(hits, 0, ids_l)], nodes, float("-inf"))
    row["host_definition_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    row["host_route_ms"] = round(row["d2h_ms"] + row["host_definition_ms"], 3)
    same = np.array_equal(got.score.view(np.int64), want.score.view(np.int64)) and np.array_equal(got.u, want.u) and \
        np.array_equal(got.v, want.v)
    assert same, f"{name}: device and host disagree"
    row["entry_vs_host"] = round(row["host_route_ms"] / max(row["entry_ms"], 1e-9), 1)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import minimum_spanning_tree
    except ImportError:
        row["scipy_ms"] = None
    else:
        t0 = time.perf_counter()
        u, v = hits.i.astype(np.int64), hits.j.astype(np.int64) + ids_l
        order_ = np.lexsort((-hits.score, v, u))  # the best score of every pair first
        u, v, s = u[order_], v[order_], hits.score[order_]
        first = np.r_[True, (u[1:] != u[:-1]) | (v[1:] != v[:-1])] if n else np.zeros(0, bool)
        graph = coo_matrix((-(s[first] + 1.0), (u[first], v[first])), shape=(nodes, nodes))  # (+1: no explicit zero weights)
        tree = minimum_spanning_tree(graph)
        row["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert tree.nnz == len(want), f"{name}: scipy's tree has {tree.nnz} edges"
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
    ap.add_argument("--skip-host", action="store_true", help="device figures only (A/B runs of variant libraries)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "span_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    only = set(filter(None, args.only.split(",")))
    want = lambda name: not only or name in only
    rows = []

    def add(name, full, forest_fn, left, right):
        rows.append(case(name, full, forest_fn, left, right, args.reps, dev, args.skip_host))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    def raw(name, kind, lt, rt, thr):
        full_fn, forest_fn = (grid.indel_raw_grid, grid.indel_raw_forest) if kind == "indel" else \
            (grid.jaccard_raw_grid, grid.jaccard_raw_forest)
        add(name, lambda defer, cap=None: full_fn(lt, rt, thr, capacity=cap, defer=defer),
            lambda cap=None: forest_fn(lt, rt, thr, capacity=cap), lt, rt)

    def levels(name, tabs, thr, mode):
        add(name, lambda defer, cap=None: grid.indel_levels_grid(*tabs, thr, category_mode=mode, capacity=cap, defer=defer),
            lambda cap=None: grid.indel_levels_forest(*tabs, thr, category_mode=mode, capacity=cap), tabs[0], tabs[2])

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

    result = {"bench": "merge forests of hit lists (nsm_span_hits) vs nsm_group_hits, the host route and the grid it follows",
              "device": torch.cuda.get_device_name(dev), "reps": args.reps, "library": str(_lib.LIB_PATH.name), "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
