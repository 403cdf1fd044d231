"""Match groups (nsm_group_hits, include/nsm_hip_groups.h) on the bench workloads' hit lists, beside the host route it
replaces and the grid it follows.  Writes profiles/groups_bench.json and prints it as ONE JSON line.

    python tools/bench_groups.py [--reps 3] [--c3 200000] [--term 20000] [--c2 50000] [--c5w 200000] [--same 2000]
                                 [--only NAME[,NAME]] [--counters FILE] [--skip-host] [--out profiles/groups_bench.json]

Lists (the ones tools/bench_assign.py uses): C3's hits at 0.8 (RAW fuzzy_match), the Term workload at 0.5 (levels
fuzzy_match), C2 at 0.5 and at 0.1 (RAW Jaccard), one cohort pair of c5w at 0.5 (levels fuzzy_match with categories), and an
all-identical cohort of ``--same`` x ``--same`` strings (one component, every record but 2 * same - 1 redundant).

Per list, all on the same tables in one process, each figure the median of ``--reps`` calls after one warm-up call, wall
clock around a call that ends synchronised:
  grid_ms            the grid alone, its hits left unsorted in their device buffer
  entry_ms           nsm_group_hits alone on that buffer (two cohorts: left ids, then right ids), with the ``stats`` it
                     reports: [records with score >= min_score, hooks made]
  device_path_ms     grid.*_groups end to end: grid, nsm_group_hits, D2H of the labels
  host_route_ms      what a consumer does without the entry: D2H of the unsorted list (``d2h_ms``) plus
                     grid.groups_of_hits on the host (``host_definition_ms``, ONE run)
  scipy_ms           scipy.sparse.csgraph.connected_components on the same host arrays, where scipy is importable
``entry_vs_host`` = host_route_ms / entry_ms, ``entry_vs_grid`` = entry_ms / grid_ms.
With a library built with -DNSM_GROUP_STATS (NSM_HIP_LIBRARY) ``counters`` holds CAS attempts, lost CAS and find hops per
record; ``--counters FILE`` copies that field from an earlier run's JSON (of such a build) into this run's rows.  Every
timed wrapper call gets a buffer that holds the list, so no grid runs twice."""
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


def counters_reader():
    lib = _lib.load()
    if not hasattr(lib, "nsm_group_counters"):
        return None
    lib.nsm_group_counters.argtypes, lib.nsm_group_counters.restype = [ctypes.c_void_p], None

    def read():
        out = (ctypes.c_ulonglong * 3)()
        lib.nsm_group_counters(out)
        return [int(v) for v in out]

    return read


def case(name, full, groups, left, right, reps, dev, skip_host=False):
    """One row.  ``full(defer, cap)``: the grid wrapper; ``groups(cap)``: the *_groups wrapper."""
    fn = _lib.entry("nsm_group_hits")
    stream = torch.cuda.current_stream(dev).cuda_stream
    pending = full(True)
    n = pending.n
    cap = n + 1  # (no retry in the timed calls)
    ids_l, ids_r = int(left.orig[: left.n].max()) + 1, int(right.orig[: right.n].max()) + 1
    nodes = ids_l + ids_r
    row = {"list": name, "records": n, "left_ids": ids_l, "right_ids": ids_r, "nodes": nodes}
    row["grid_ms"] = wall_ms(lambda: full(True, cap), reps, dev)
    buf = pending.buf
    label = torch.empty(nodes, dtype=torch.int32, device=dev)
    st = torch.zeros(2, dtype=torch.int64, device=dev)
    lists = (_lib.NsmHitList * 1)(_lib.NsmHitList(buf.records.data_ptr() if n else None, n, 0, ids_l, ids_l, ids_r))

    def entry():
        st.zero_()
        _lib.check(fn(lists, 1, nodes, float("-inf"), 0, label.data_ptr(), st.data_ptr(), stream), "nsm_group_hits")

    read = counters_reader()
    before = read() if read else None
    row["entry_ms"] = wall_ms(entry, reps, dev)
    row["stats"] = [int(v) for v in st.tolist()]
    if read:
        per = [(a - b) / (reps + 1) / max(1, n) for a, b in zip(read(), before)]
        row["counters"] = {"cas_per_record": round(per[0], 5), "lost_cas_per_record": round(per[1], 5),
                           "find_hops_per_record": round(per[2], 4)}
    device_label = label.cpu().numpy()
    row["groups"] = int((np.bincount(device_label, minlength=nodes) >= 2).sum())
    row["largest_group"] = int(np.bincount(device_label, minlength=nodes).max())
    row["device_path_ms"] = wall_ms(lambda: groups(cap), reps, dev)
    if skip_host:
        return row

    # the host route: the list crosses to the host as it lies in the buffer, then a union-find in Python
    def d2h():
        host = buf.records[:n].cpu().numpy()
        ij = host.view(np.int32).reshape(n, 4)
        return grid.Hits(host[:, 0].copy(), ij[:, 2].copy(), ij[:, 3].copy())

    row["d2h_ms"] = wall_ms(d2h, reps, dev)
    hits = d2h()
    t0 = time.perf_counter()
    want = grid.groups_of_hits([(hits, 0, ids_l)], nodes, float("-inf"))
    row["host_definition_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    row["host_route_ms"] = round(row["d2h_ms"] + row["host_definition_ms"], 3)
    assert np.array_equal(device_label, want), f"{name}: device and host disagree"
    assert np.array_equal(groups(cap).label, want), f"{name}: the wrapper and the host disagree"
    assert row["stats"] == [n, nodes - int((want == np.arange(nodes)).sum())], f"{name}: stats {row['stats']}"
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        row["scipy_ms"] = None
    else:
        t0 = time.perf_counter()
        graph = coo_matrix((np.ones(n, dtype=np.int8), (hits.i.astype(np.int64), hits.j.astype(np.int64) + ids_l)), shape=(nodes, nodes))
        count, _ = connected_components(graph, directed=False)
        row["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert count == nodes - row["stats"][1], f"{name}: scipy counts {count} components"
    row["entry_vs_host"] = round(row["host_route_ms"] / max(row["entry_ms"], 1e-9), 1)
    row["entry_vs_grid"] = round(row["entry_ms"] / max(row["grid_ms"], 1e-9), 3)
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
    ap.add_argument("--counters", default="", help="JSON of a run on a -DNSM_GROUP_STATS library: its counters are copied in")
    ap.add_argument("--skip-host", action="store_true", help="device figures only (A/B runs of variant libraries)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "groups_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    only = set(filter(None, args.only.split(",")))
    want = lambda name: not only or name in only
    rows = []

    def add(name, full, groups, left, right):
        rows.append(case(name, full, groups, left, right, args.reps, dev, args.skip_host))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    def raw(name, kind, lt, rt, thr):
        full_fn, groups_fn = (grid.indel_raw_grid, grid.indel_raw_groups) if kind == "indel" else \
            (grid.jaccard_raw_grid, grid.jaccard_raw_groups)
        add(name, lambda defer, cap=None: full_fn(lt, rt, thr, capacity=cap, defer=defer),
            lambda cap=None: groups_fn(lt, rt, thr, capacity=cap), lt, rt)

    def levels(name, tabs, thr, mode):
        add(name, lambda defer, cap=None: grid.indel_levels_grid(*tabs, thr, category_mode=mode, capacity=cap, defer=defer),
            lambda cap=None: grid.indel_levels_groups(*tabs, thr, category_mode=mode, capacity=cap), tabs[0], tabs[2])

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

    if args.counters:
        earlier = {r["list"]: r.get("counters") for r in json.loads(Path(args.counters).read_text())["rows"]}
        for row in rows:
            if "counters" not in row and earlier.get(row["list"]):
                row["counters"] = earlier[row["list"]]
    result = {"bench": "match groups of hit lists (nsm_group_hits) vs the host route and the grid it follows",
              "device": torch.cuda.get_device_name(dev), "reps": args.reps, "library": str(_lib.LIB_PATH.name), "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
