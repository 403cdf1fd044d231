"""The six Jaccard grid kernels at their batch, tile, queue and hash seams (tests/support/jaccard_seams.py), on the GPU: every
case through every route that can take it, each result equal to the C oracle's -- same hits, same scores bit for bit, same
order -- compared as arrays.  Each test first asserts its premises from the BUILT tables (cnt, seg_start, post_format, row
count), so a case that drifted off its seam fails instead of passing vacuously.  No tolerances.
"""
import functools

import numpy as np
import pytest
import torch

from tests.support import jaccard_seams as js

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _want(family, key, thr):
    return js.case_oracle(_CASES[family](*key), thr)


_CASES = {"A": js.batch_case, "B": js.levels_batch_case, "C": js.prefix_case, "D": js.cluster_case, "E": js.dense_case,
          "F": js.queue_case, "G": js.run_case}


def _same(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} hits, the oracle has {len(want)}"
    assert np.array_equal(got.i, want["i"]) and np.array_equal(got.j, want["j"]), f"{what}: other pairs or another order"
    assert np.array_equal(got.score.view(np.uint64), want["score"].view(np.uint64)), f"{what}: a score differs in its bits"


def _raw_routes(case, dev, lt, rt, want, thr=None, capacity=None):
    """index=True on both posting formats, the per-tile index, the signature kernel with and without the prune, and the
    library's own choice.  (A table built without a global index sends index=True to the per-tile index.)"""
    from napkon_string_matching_amd import grid

    thr = case["thr"] if thr is None else thr
    W = case["width"]
    run = lambda right, **kw: grid.jaccard_raw_grid(lt, right, thr, capacity=capacity, **kw)
    if rt.post is not None:
        assert rt.post_format == 2 and rt.post_row_bits > 0
        rt64 = js.build_right(case, dev, compact=False)
        assert rt64.post_format == 0 and rt64.post_row_bits == 0 and rt64.n == rt.n
        _same(run(rt64, index=True), want, "global index, 64-bit postings")
    _same(run(rt, index=True), want, "index=True")
    if W <= 32:
        _same(run(rt, index="tile"), want, "per-tile index")
    _same(run(rt, index=False, prune=True), want, "signature kernel, pruned")
    _same(run(rt, index=False, prune=False), want, "signature kernel, exhaustive")
    _same(run(rt), want, "the library's choice")


def _levels_routes(case, dev, lt, rt, want, thr=None, capacity=None):
    from napkon_string_matching_amd import grid

    thr = case["thr"] if thr is None else thr
    mode = case.get("mode", js.CAT_NONE)
    run = lambda right, **kw: grid.jaccard_levels_grid(lt, right, thr, category_mode=mode, capacity=capacity, **kw)
    assert rt.post is not None and rt.post_format == 1
    rt64 = js.build_right(case, dev, compact=False)
    assert rt64.post_format == 0 and rt64.n == rt.n
    _same(run(rt, index=True), want, "global index")
    _same(run(rt64, index=True), want, "global index, 64-bit postings")
    if case["width"] <= 32:
        _same(run(rt, index="tile"), want, "per-tile index")
    _same(run(rt, index=False), want, "filter kernel")
    _same(run(rt), want, "the library's choice")


@pytest.mark.parametrize("name", [s[0] for s in js.batch_sizes()])
def test_raw_global_batch_geometry(dev, name):
    """Family A: rows_per_batch 1 .. 64 of jaccard_raw_global_kernel (jaccard_raw_global.hip:263-269), the sizes around the
    seam at 2 and 8, widths 32 and 64 at 2, and the second trip through the grid-stride loop."""
    case = js.batch_case(name)
    lt, rt = js.build_tables(case, dev)
    print(name, js.check_batch(case, lt, rt))
    want = _want("A", (name,), case["thr"])
    js.check_batch_hits(case, want)
    _raw_routes(case, dev, lt, rt, want, capacity=(1 << 12) if name == "w16_r2_smallest" else None)


@pytest.mark.parametrize("name", [s[0] for s in js.levels_batch_sizes()])
def test_levels_global_batch_geometry(dev, name):
    """Family B: 8192 batches and the second trip of jaccard_levels_global_kernel's grid-stride loop
    (jaccard_levels_global.hip:69, 236-239) at all three widths, plain and with a category partition."""
    case = js.levels_batch_case(name)
    lt, rt = js.build_tables(case, dev)
    print(name, js.check_levels_batch(case, lt, rt))
    want = _want("B", (name,), case["thr"])
    js.check_levels_batch_hits(case, want)
    _levels_routes(case, dev, lt, rt, want, capacity=4 if name == "w16_above_part" else None)


@pytest.mark.parametrize("W,thr", [(W, thr) for W in (16, 32) for thr in js.LONGEST[W]])
def test_raw_global_prefix_edge(dev, W, thr):
    """Family C: first common ids in the last slot the prefix admits on both sides, at kmin and one below
    (jaccard_raw_global.hip:89, 173, 216), cls_end 1 .. 5."""
    case = js.prefix_case(W, thr)
    lt, rt = js.build_tables(case, dev)
    print(case["name"], js.check_prefix(case, lt, rt))
    want = _want("C", (W, thr), thr)
    js.check_prefix_hits(case, want)
    _raw_routes(case, dev, lt, rt, want, capacity=64 if (W, thr) == (16, 0.5) else None)


@pytest.mark.parametrize("kind", ["raw", "levels"])
@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("dense", [False, True])
def test_tile_index_wrapped_probe_run(dev, kind, W, dense):
    """Family D: a probe run across the end of the per-tile hash table (jaccard_raw_index.hip:104-108, 171-180;
    jaccard_levels_index.hip:162-166, 222-231), in a sparse and in a dense tile."""
    case = js.cluster_case(W, kind, dense)
    lt, rt = js.build_tables(case, dev, index=case.get("index"))
    print(case["name"], js.check_cluster(case, lt, rt))
    for thr in case["thrs"]:
        want = _want("D", (W, kind, dense), thr)
        assert len(np.unique(want["j"])) == 64
        (_raw_routes if kind == "raw" else _levels_routes)(case, dev, lt, rt, want, thr=thr, capacity=32 if not dense else None)


@pytest.mark.parametrize("kind", ["raw", "levels"])
@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("variant", ["at", "over", "partial"])
def test_tile_index_dense_rule(dev, kind, W, variant):
    """Family E: tiles of exactly 3/4 T and 3/4 T + 1 ids, and a dense partial tile whose second pass holds 17 lanes
    (jaccard_raw_impl.hpp:46-51, jaccard_raw_index.hip:85-89, jaccard_levels_index.hip:73, 148)."""
    case = js.dense_case(W, kind, variant)
    lt, rt = js.build_tables(case, dev)
    print(case["name"], js.check_dense(case, lt, rt))
    want = _want("E", (W, kind, variant), case["thr"])
    js.check_dense_hits(case, want)
    (_raw_routes if kind == "raw" else _levels_routes)(case, dev, lt, rt, want, capacity=2 if variant == "over" else None)


@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("layout", ["alone", "last", "all"])
def test_levels_candidate_queues(dev, W, layout):
    """Family F: queue depths 27 .. 33 and 61 .. 63 of one lane, of lane 63 while lane 0 is empty, and of all 64 lanes at
    once (jaccard_levels_impl.hpp:137-144, 185-186, 200-204; jaccard_levels_index.hip:141-145, 255-257)."""
    for c in js.F_DEPTHS:
        case = js.queue_case(W, c, layout)
        lt, rt = js.build_tables(case, dev)
        for kernel in ("signature", "index"):
            js.check_queue(case, lt, rt, kernel)
        want = _want("F", (W, c, layout), case["thr"])
        js.check_queue_hits(case, want)
        _levels_routes(case, dev, lt, rt, want, capacity=8 if c == 33 else None)


@pytest.mark.parametrize("W", [16, 32])
def test_levels_candidate_queues_across_ranges(dev, W):
    """Family F: candidates across the boundary of two waves' row ranges, and a category segment cut by a chunk boundary."""
    for kernel, case in js.queue_straddle_cases(W):
        lt, rt = js.build_tables(case, dev)
        print(case["name"], kernel, js.check_queue(case, lt, rt, kernel, straddle=True))
        if case.get("partition"):
            ss = js.column(lt, "seg_start")
            assert lt.n > 512 and ss[1] < 512 < ss[2], "the chunk boundary does not cut the category segment"
        want = js.case_oracle(case)
        js.check_queue_hits(case, want)
        _levels_routes(case, dev, lt, rt, want)


@pytest.mark.parametrize("W", [16, 32])
def test_raw_signature_run_lengths(dev, W):
    """Family G: size classes of 0, 1, 7, 8, 9, 15, 16, 17, 24 and 25 rows inside a chunk of the pruned jaccard_raw_kernel
    (the two-register-set pipeline of eight-row batches, jaccard_raw_impl.hpp:168-189), one class cut by the chunk's end."""
    case = js.run_case(W)
    lt, rt = js.build_tables(case, dev)
    m = js.check_runs(case, lt, rt)
    print(case["name"], m)
    want = _want("G", (W,), case["thr"])
    js.check_runs_hits(case, want, lt, m["runs"])
    _raw_routes(case, dev, lt, rt, want, capacity=16)
