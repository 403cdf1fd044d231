"""Listed pairs (nsm_*_pairs) against what they replace, one plugin call per pair.  Writes profiles/pairs_bench.json and
prints it as ONE JSON line.

    python tools/bench_pairs.py [--calls 20] [--scalar 100] [--pairs 1000000] [--term 20000] [--c3 200000] [--c2 50000]
                                [--c5w 100000] [--out profiles/pairs_bench.json]

Cases: Term-shaped items (synthetic.term_cohort, bench.py's `term` corpus) with one-to-one pairs (k, k) and with random
pairs, as RAW fuzzy_match (the first level's string) and as compare_terms x fuzzy_match over the levels; C3 strings; C2
sets; c5w-shaped levels (synthetic.c5_cohort over word-like text) with intersection_vs_union.

Per case:
* ``entry_ms``: the C entry alone into buffers allocated once (records and row maps on the device): a warm-up call, then
  ``--calls`` calls between two HIP events; ``pairs_per_s`` from it.
* ``wrapper_ms``: the Python face grid.*_pairs end to end -- row maps, the records' copy to the device and back.
* ``scalar_ms``: the mean of ``--scalar`` calls of the scalar face on pairs of the same list -- ``plugin(a, b)`` for the RAW
  cases, ``ComparableData.compare_terms(a, b, plugin)`` for the levels cases -- each a table build, a 1 x 1 grid and a
  device-to-host sync (wall clock).  ``scalar_over_entry_per_pair`` = scalar_ms / (entry_ms / P).
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "napkon-string-matching_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from napkon_string_matching_amd import _lib, grid, synthetic, tables  # noqa: E402
from napkon_string_matching_amd.compare import score_functions as sf  # noqa: E402
from napkon_string_matching_amd.types.comparable_data import ComparableData  # noqa: E402


def case(name, entry, args, left, right, i, j, scalar, n_scalar, calls):
    """One row.  ``args``: the entry's tables; ``left`` / ``right``: the tables the ids name; ``scalar(p)`` scores pair p of
    the list through the scalar face."""
    dev = left.orig.device
    fn = getattr(_lib.load(), entry)
    face = getattr(grid, entry[len("nsm_"):])
    n = len(i)
    host = np.zeros((n, 2), dtype=np.float64)
    host.view(np.int32).reshape(n, 4)[:, 2] = i
    host.view(np.int32).reshape(n, 4)[:, 3] = j
    records = torch.from_numpy(host).to(dev)
    lmap, rmap = grid._row_map(left.orig, left.n, dev), grid._row_map(right.orig, right.n, dev)
    structs = [t.struct() for t in args]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call():
        _lib.check(fn(*structs, lmap.data_ptr(), lmap.numel(), rmap.data_ptr(), rmap.numel(), records.data_ptr(), n, stream), entry)

    call()  # warm-up
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        call()
    stop.record()
    stop.synchronize()
    entry_ms = start.elapsed_time(stop) / calls
    scores = records[:, 0].cpu().numpy()
    face(*args, i, j)  # warm-up
    t0 = time.perf_counter()
    for _ in range(3):
        got = face(*args, i, j)
    wrapper_ms = (time.perf_counter() - t0) / 3 * 1e3
    assert np.array_equal(got, scores), "the entry and the Python face disagree"
    picks = np.linspace(0, n - 1, n_scalar).astype(np.int64)
    scalar(int(picks[0]))  # warm-up
    t0 = time.perf_counter()
    single = [scalar(int(p)) for p in picks]
    scalar_ms = (time.perf_counter() - t0) / len(picks) * 1e3
    same = bool(np.array_equal(np.array(single, dtype=np.float64), scores[picks]))
    return {"case": name, "entry": entry, "n": left.n, "m": right.n, "pairs": n, "entry_ms": round(entry_ms, 4), "calls": calls,
            "pairs_per_s": round(n / (entry_ms * 1e-3)), "wrapper_ms": round(wrapper_ms, 3), "scalar_ms": round(scalar_ms, 3),
            "scalar_calls": len(picks), "scalar_over_entry_per_pair": round(scalar_ms / (entry_ms / n)),
            "scalar_equals_entry": same, "mean_score": float(scores.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--scalar", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--term", type=int, default=20_000)
    ap.add_argument("--c3", type=int, default=200_000)
    ap.add_argument("--c2", type=int, default=50_000)
    ap.add_argument("--c5w", type=int, default=100_000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pairs_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2024)
    rows = []

    def add(*args):
        rows.append(case(*args, a.scalar, a.calls))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)

    def lists(n, m):
        return (("one_to_one", np.arange(min(n, m)), np.arange(min(n, m))),
                ("random", rng.integers(0, n, a.pairs), rng.integers(0, m, a.pairs)))

    # ---- Term-shaped items: RAW fuzzy on the first level, compare_terms x fuzzy_match over the levels
    ta = synthetic.term_cohort(a.term, 7)
    tb = synthetic.term_cohort(a.term, 8, plant_from=ta)
    lev_a, lev_b = synthetic.term_levels(ta), synthetic.term_levels(tb)
    raw_a, raw_b = [it[0] for it in lev_a], [it[0] for it in lev_b]
    lt, rt = tables.encode_strings([sf.fuzzy_operand(s) for s in raw_a], [sf.fuzzy_operand(s) for s in raw_b], dev)
    ops = lambda items: [[sf.fuzzy_operand(lv) for lv in it] for it in items]
    li, ls, ri, rs = tables.encode_level_strings(ops(lev_a), ops(lev_b), dev, partition=False)
    for label, i, j in lists(len(lev_a), len(lev_b)):
        add(f"term_raw_fuzzy_{label}", "nsm_indel_raw_pairs", (lt, rt), lt, rt, i, j, lambda p: sf.fuzzy_match(raw_a[i[p]], raw_b[j[p]]))
        add(f"term_levels_fuzzy_{label}", "nsm_indel_levels_pairs", (li, ls, ri, rs), li, ri, i, j,
            lambda p: ComparableData.compare_terms(lev_a[i[p]], lev_b[j[p]], sf.fuzzy_match))

    # ---- C3 strings
    (lc, ll), (rc, rl) = synthetic.c3_corpus(a.c3, a.c3)
    alpha = synthetic.STRING_ALPHABET
    lt, rt = tables.StrTable.from_codes(lc, ll, len(alpha), dev), tables.StrTable.from_codes(rc, rl, len(alpha), dev)
    text = lambda codes, lens, k: "".join(alpha[c] for c in codes[k, : lens[k]])
    _, i, j = lists(a.c3, a.c3)[1]
    add("c3_fuzzy_random", "nsm_indel_raw_pairs", (lt, rt), lt, rt, i, j,
        lambda p: sf.fuzzy_match(text(lc, ll, i[p]), text(rc, rl, j[p])))

    # ---- C2 sets
    left, right = synthetic.c2_corpus(a.c2, a.c2)
    lt, rt = tables.SetTable.from_padded(left, "left", dev), tables.SetTable.from_padded(right, "right", dev)
    toks = lambda ids, k: [f"t{v}" for v in ids[k] if v >= 0]
    _, i, j = lists(a.c2, a.c2)[1]
    add("c2_jaccard_random", "nsm_jaccard_raw_pairs", (lt, rt), lt, rt, i, j,
        lambda p: sf.intersection_vs_union(toks(left, i[p]), toks(right, j[p])))

    # ---- c5w-shaped levels Jaccard
    lex = synthetic.word_vocabulary(20_000)
    ca = synthetic.c5_cohort(a.c5w, 11, lex=lex)
    cb = synthetic.c5_cohort(a.c5w, 12, plant_from=ca, lex=lex)
    lt = tables.SetTable.from_nested_arrays(ca["ids"], ca["plen"], ca["nlev"], "left", dev, width=16, partition=False, index=False)
    rt = tables.SetTable.from_nested_arrays(cb["ids"], cb["plen"], cb["nlev"], "right", dev, width=16, partition=False, index=False)
    _, i, j = lists(a.c5w, a.c5w)[1]
    item = lambda c, k: synthetic.c5_level_token_lists(c, slice(k, k + 1))[0]
    add("c5w_levels_jaccard_random", "nsm_jaccard_levels_pairs", (lt, rt), lt, rt, i, j,
        lambda p: ComparableData.compare_terms(item(ca, int(i[p])), item(cb, int(j[p])), sf.intersection_vs_union))

    result = {"bench": "listed pairs vs one plugin call per pair", "device": torch.cuda.get_device_name(dev), "rows": rows}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
