"""Edge support and truss peeling (nsm_support_hits, include/nsm_hip_support.h) on hit lists whose node spaces contain
triangles, beside the grid it follows and the host route it replaces.  Writes profiles/support_bench.json and prints it as
ONE JSON line.

    python tools/bench_support.py [--reps 3] [--term 20000] [--c3 200000] [--c5w 100000] [--random 200000] [--degrees 8,24,48,96]
                                  [--only NAME[,NAME]] [--skip-host] [--variant PATH ...] [--out profiles/support_bench.json]

Lists: the self-join (``same=True``) of the Term-shaped items at 0.5 (levels fuzzy_match) and of the C3 strings at 0.8 (RAW
fuzzy_match), and the three cohort-pair lists of three c5w cohorts at 0.5 in ONE node space (hap-pop, hap-suep, pop-suep).
With ``--only random``: uniform random self-join lists over ``--random`` nodes, one per mean degree of ``--degrees`` -- rows
between C5's (a handful of arcs) and Term's (hundreds), where the routing constant decides; they come from no grid, so their
``grid_ms`` is only the upload.

Per list, all on the same buffers in one process, each figure the median of ``--reps`` calls after one warm-up call, wall
clock around a call that ends synchronised:
  grid_ms            the grid(s) alone, hits left unsorted in their device buffers
  entry              per ``min_support`` 0, 1, 2: ``ms`` of nsm_support_hits alone on those buffers, and the ``stats`` it
                     reports: [edge records, distinct edges, distinct edges alive, rounds, sum of the final supports]
  groups_ms          the truss groups at min_support = 1 from the buffers: nsm_support_hits, the alive records compacted on
                     the device, nsm_group_hits, D2H of the labels
  device_path_ms     (self-joins) grid.*_groups(..., same=True, min_support=1) end to end, the grid included
  host_route_ms      what a consumer does without the entry: D2H of the unsorted lists (``d2h_ms``) plus scipy's
                     ``(A @ A).multiply(A)`` on the symmetric 0/1 adjacency (``scipy_ms``, ONE run), checked against stats[4]
  variants           with ``--variant PATH`` (libraries that export nsm_support_hits, built with another
                     -DNSM_SUPPORT_WAVE_MIN): the min_support = 0 entry of each on the same buffers
``entry_vs_host`` = host_route_ms / entry[0].ms, ``entry_vs_grid`` = entry[0].ms / grid_ms."""
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


def entry_call(fn, entries, nodes, min_support, words, st, stream):
    lists = (_lib.NsmHitList * len(entries))()
    out = (ctypes.c_void_p * len(entries))()
    for k, (slot, (ptr, n, lb, li, rb, ri)) in enumerate(zip(lists, entries)):
        slot.hits, slot.n, slot.left_base, slot.left_ids, slot.right_base, slot.right_ids = (ptr if n else None), n, lb, li, rb, ri
        out[k] = words[k].data_ptr() if n else None

    def call():
        st.zero_()
        status = fn(lists, len(entries), nodes, float("-inf"), min_support, out, st.data_ptr(), stream)
        if status:
            raise RuntimeError(f"nsm_support_hits returned {status}")

    return call


def case(name, grids, nodes, reps, dev, skip_host, variants, wrapper=None):
    """One row.  ``grids``: per list ``(run(defer, cap) -> PendingHits or Hits, left_base, left_ids, right_base, right_ids)``."""
    fn = _lib.entry("nsm_support_hits")
    stream = torch.cuda.current_stream(dev).cuda_stream
    pendings = [run(True, None) for run, *_ in grids]
    caps = [p.n + 1 for p in pendings]  # (no retry in the timed calls)
    entries = [(p.buf.records.data_ptr(), p.n, lb, li, rb, ri) for p, (_run, lb, li, rb, ri) in zip(pendings, grids)]
    records = [p.buf.records for p in pendings]
    row = {"list": name, "records": [p.n for p in pendings], "nodes": nodes}
    row["grid_ms"] = wall_ms(lambda: [run(True, cap) for (run, *_), cap in zip(grids, caps)], reps, dev)
    words = [torch.empty(max(1, p.n), dtype=torch.int32, device=dev) for p in pendings]
    st = torch.zeros(5, dtype=torch.int64, device=dev)
    row["entry"] = []
    for s in (0, 1, 2):
        call = entry_call(fn, entries, nodes, s, words, st, stream)
        ms = wall_ms(call, reps, dev)
        row["entry"].append({"min_support": s, "ms": ms, "stats": [int(v) for v in st.tolist()]})
        print(json.dumps({name: row["entry"][-1]}), file=sys.stderr, flush=True)
    for path in variants:
        lib = ctypes.CDLL(path)
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        lib.nsm_support_hits.argtypes = [ctypes.POINTER(_lib.NsmHitList), i32, i32, ctypes.c_double, i32, ctypes.POINTER(vp), vp, vp]
        lib.nsm_support_hits.restype = ctypes.c_int
        ms = wall_ms(entry_call(lib.nsm_support_hits, entries, nodes, 0, words, st, stream), reps, dev)
        assert [int(v) for v in st.tolist()] == row["entry"][0]["stats"], f"{path}: other stats"
        row.setdefault("variants", []).append({"library": Path(path).name, "ms": ms})
        print(json.dumps({name: row["variants"][-1]}), file=sys.stderr, flush=True)

    def truss_groups():
        alive, _keep = grid._truss_entries(entries, records, nodes, float("-inf"), 1, dev)
        return grid.group_lists_device(alive, nodes, float("-inf"), dev)

    row["groups_ms"] = wall_ms(truss_groups, reps, dev)
    label = truss_groups()
    sizes = np.bincount(label, minlength=nodes)
    row["truss_groups"], row["largest_truss_group"] = int((sizes >= 2).sum()), int(sizes.max())
    plain = np.bincount(grid.group_lists_device(entries, nodes, float("-inf"), dev), minlength=nodes)
    row["plain_groups"], row["largest_plain_group"] = int((plain >= 2).sum()), int(plain.max())
    if wrapper is not None:
        row["device_path_ms"] = wall_ms(lambda: wrapper(caps[0]), reps, dev)
        assert np.array_equal(wrapper(caps[0]).label, label), f"{name}: the wrapper and the entry disagree"
    if skip_host:
        return row

    def d2h():
        out = []
        for p in pendings:
            host = p.buf.records[: p.n].cpu().numpy()
            ij = host.view(np.int32).reshape(p.n, 4)
            out.append((ij[:, 2].copy(), ij[:, 3].copy()))
        return out

    row["d2h_ms"] = wall_ms(d2h, reps, dev)
    try:
        from scipy.sparse import coo_matrix
    except ImportError:
        row["scipy_ms"] = None
        return row
    host = d2h()
    t0 = time.perf_counter()
    u = np.concatenate([i.astype(np.int64) + lb for (i, _j), (_r, lb, _li, _rb, _ri) in zip(host, grids)])
    v = np.concatenate([j.astype(np.int64) + rb for (_i, j), (_r, _lb, _li, rb, _ri) in zip(host, grids)])
    keep = u != v
    adj = coo_matrix((np.ones(2 * int(keep.sum()), dtype=np.int32), (np.r_[u[keep], v[keep]], np.r_[v[keep], u[keep]])),
                     shape=(nodes, nodes)).tocsr()
    adj.data[:] = 1  # (duplicates and the other orientation were summed)
    common = (adj @ adj).multiply(adj)
    total = int(common.sum())
    row["scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    assert total == 2 * row["entry"][0]["stats"][4], f"{name}: scipy counts {total}, the entry {row['entry'][0]['stats'][4]}"
    row["host_route_ms"] = round(row["d2h_ms"] + row["scipy_ms"], 3)
    row["entry_vs_host"] = round(row["host_route_ms"] / max(row["entry"][0]["ms"], 1e-9), 1)
    row["entry_vs_grid"] = round(row["entry"][0]["ms"] / max(row["grid_ms"], 1e-9), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--term", type=int, default=20_000)
    ap.add_argument("--c3", type=int, default=200_000)
    ap.add_argument("--c5w", type=int, default=100_000)
    ap.add_argument("--random", type=int, default=200_000)
    ap.add_argument("--degrees", default="8,24,48,96")
    ap.add_argument("--only", default="", help="comma-separated list names (term, c3, c5w; random only when named)")
    ap.add_argument("--skip-host", action="store_true", help="device figures only (A/B runs of variant libraries)")
    ap.add_argument("--variant", action="append", default=[], help="a library that exports nsm_support_hits (another routing constant)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "support_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    only = set(filter(None, args.only.split(",")))
    want = lambda name: not only or name in only
    rows = []

    def add(*a, **kw):
        rows.append(case(*a, reps=args.reps, dev=dev, skip_host=args.skip_host, variants=args.variant, **kw))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    if want("term"):
        a = synthetic.term_cohort(args.term, 1234)
        ops = [[sf.fuzzy_operand(lv) for lv in it] for it in synthetic.term_levels(a)]
        tabs = tables.encode_level_strings(ops, ops, dev)
        n = args.term
        add(f"term self-join {n}x{n} at 0.5",
            [(lambda defer, cap: grid.indel_levels_grid(*tabs, 0.5, capacity=cap, defer=defer), 0, n, 0, n)], n,
            wrapper=lambda cap: grid.indel_levels_groups(*tabs, 0.5, capacity=cap, same=True, min_support=1))
    if want("c3"):
        (lc, ll), _right = synthetic.c3_corpus(args.c3, args.c3)
        alpha = len(synthetic.STRING_ALPHABET)
        lt, rt = tables.StrTable.from_codes(lc, ll, alpha, dev), tables.StrTable.from_codes(lc, ll, alpha, dev)
        n = args.c3
        add(f"c3 self-join {n}x{n} at 0.8", [(lambda defer, cap: grid.indel_raw_grid(lt, rt, 0.8, capacity=cap, defer=defer), 0, n, 0, n)],
            n, wrapper=lambda cap: grid.indel_raw_groups(lt, rt, 0.8, capacity=cap, same=True, min_support=1))
    if want("c5w"):
        mode = _lib.CAT_INTERSECT_OR_BOTH_EMPTY
        lex = synthetic.word_vocabulary(20_000)
        n = args.c5w
        hap = synthetic.c5_cohort(n, 11, lex=lex)
        pop = synthetic.c5_cohort(n, 12, plant_from=hap, lex=lex)
        suep = synthetic.c5_cohort(n, 13, plant_from=hap, lex=lex)
        alphabet = len(synthetic.c5_alphabet(hap))
        cohorts = [hap, pop, suep]
        grids = []
        for a, b in ((0, 1), (0, 2), (1, 2)):
            tabs = tables.encode_level_codes(synthetic.c5_level_codes(cohorts[a]), synthetic.c5_level_codes(cohorts[b]), alphabet, dev,
                                             cohorts[a]["cat"], cohorts[b]["cat"], mode)
            run = (lambda tabs: lambda defer, cap: grid.indel_levels_grid(*tabs, 0.5, category_mode=mode, capacity=cap, defer=defer))(tabs)
            grids.append((run, a * n, n, b * n, n))
        add(f"c5w hap, pop, suep pairwise {n} rows each at 0.5", grids, 3 * n)
    if "random" in only:
        n = args.random
        for degree in (int(v) for v in args.degrees.split(",")):
            rng = np.random.RandomState(degree)
            count = n * degree // 2
            host = np.empty((count, 2), dtype=np.float64)
            host[:, 0] = 1.0
            host.view(np.int32).reshape(count, 4)[:, 2:] = rng.randint(0, n, (count, 2))

            def run(defer, cap, host=host, count=count):
                buf = grid.HitBuffer(count, dev)
                buf.records.copy_(torch.from_numpy(host))
                return grid.PendingHits(buf, count, n)

            add(f"random self-join {n} nodes, mean degree {degree}", [(run, 0, n, 0, n)], n)
    result = {"bench": "edge support and truss peeling of hit lists (nsm_support_hits) vs the grid it follows and D2H + scipy",
              "device": torch.cuda.get_device_name(dev), "reps": args.reps, "library": str(_lib.LIB_PATH.name), "rows": rows}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
