"""The launcher model and the case families of tests/support/jaccard_seams.py, checked without a GPU: the model against the
table of `longest` values, every premise of every case on tables built by the numpy path of the builders, and -- through the
C oracle alone -- that every case holds the hits and the near-misses it claims.

The largest case is family A's 524 225 x 64 table (rows_per_batch = 64): the oracle scores it in about 0.8 s
(test_batch_geometry prints the measured time); the whole file runs in about half a minute.
"""
import time

import numpy as np
import pytest
import torch

from tests.support import jaccard_seams as js

CPU = torch.device("cpu")


def test_model_longest_table():
    for W, row in js.LONGEST.items():
        for thr, want in row.items():
            assert js.longest(W, thr) == want, f"W={W} thr={thr}: model {js.longest(W, thr)}, launcher rule {want}"
    # cls_end takes all of 1 .. 5 over family C's thresholds, and slot_shift bounds rows_per_batch as family A assumes
    for W in (16, 32):
        assert {js.cls_end(W, thr) for thr in js.LONGEST[W]} == {1, 2, 3, 4, 5}
    assert [js.WAVE >> js.slot_shift(16, thr) for thr in (0.95, 0.9, 0.8, 0.6, 0.5)] == [64, 32, 16, 8, 4]


def test_model_geometry():
    """The rules restated from the launchers, at values worked out by hand from the cited lines."""
    assert js.kmin(16, 0.5)[24] == 8 and js.kmin(16, 1.0)[7] == js.NEVER and js.kmin(16, 0.01)[32] == 1
    assert js.prefix(16, 0.5)[0][16] == 9 and js.prefix(16, 1.0)[0][5] == 1
    assert js.rows_per_batch(16382, 16, 0.5) == 1 and js.rows_per_batch(16383, 16, 0.5) == 2
    assert js.rows_per_batch(20000, 16, 0.5) == 2 and js.rows_per_batch(1 << 20, 16, 0.8) == 16
    assert {r: js.smallest_n_left(r, 16, 0.95) for r in (2, 64)} == {2: 8191 * 2 + 1, 64: 8191 * 64 + 1}
    assert js.smallest_n_left(64, 16, 0.9) is None
    assert js.jac_rows_per_chunk(182, 2) == 128 and js.jac_rows_per_chunk(1 << 20, 16384) == 4096
    assert js.lev_rows_per_chunk(600, 1) == 512 and js.lev_rows_per_chunk(1 << 20, 8, True) == 512
    assert js.raw_index_geometry(2100, 1700) == (192, 27 * 3)  # 1536 -> 768 -> 384 -> 192 rows; 27 tiles x ceil(11 chunks / 4)
    assert js.lev_index_slices(600, 64) == 2 and js.lev_index_wave_ranges(0, 600, 2, 16)[:2] == [(0, 76), (76, 152)]
    assert js.index_slots(16) == 1024 and js.index_slots(32) == 2048
    assert not js.is_dense(768, 16) and js.is_dense(769, 16) and not js.is_dense(1536, 32) and js.is_dense(1537, 32)
    below = np.arange(65536)
    assert abs(int((js.home(below, 16) >= 1020).sum()) - 256) <= 8 and abs(int((js.home(below, 32) >= 2044).sum()) - 128) <= 8
    assert not js.weak(16, 0.9, 16, 16) and js.weak(16, 0.3, 12, 12)


@pytest.mark.parametrize("name", [s[0] for s in js.batch_sizes()])
def test_batch_geometry(name):
    case = js.batch_case(name)
    lt, rt = js.build_tables(case, CPU)
    print(name, js.check_batch(case, lt, rt))
    t0 = time.perf_counter()
    want = js.case_oracle(case)
    print(f"oracle: {case['left'].shape[0]} x {case['right'].shape[0]} pairs in {time.perf_counter() - t0:.2f} s")
    js.check_batch_hits(case, want)


def test_batch_geometry_covers_every_rows_per_batch():
    seen = {js.rows_per_batch(n, W, thr) for _, W, thr, n, _ in js.batch_sizes() if W == 16}
    assert seen == {1, 2, 4, 8, 16, 32, 64}
    assert {W for _, W, thr, n, _ in js.batch_sizes() if js.rows_per_batch(n, W, thr) == 2} == {16, 32, 64}
    assert {W for _, W, thr, n, _ in js.batch_sizes() if js.n_batches(n, W, thr) > js.WAVE_SLOTS} == {16, 32, 64}, "second trip"
    assert {W for _, W, n, _ in js.levels_batch_sizes() if js.levels_n_batches(n, W) > js.WAVE_SLOTS} == {16, 32, 64}


@pytest.mark.parametrize("name", [s[0] for s in js.levels_batch_sizes()])
def test_levels_batch_geometry(name):
    case = js.levels_batch_case(name)
    lt, rt = js.build_tables(case, CPU)
    print(name, js.check_levels_batch(case, lt, rt))
    want = js.case_oracle(case)
    js.check_levels_batch_hits(case, want)
    shared = js.shares_id(case["left"][0], np.unique(case["right"][0]))
    assert shared.sum() > len(want) + 100, "no candidates that fail the score"


@pytest.mark.parametrize("W", [16, 32])
def test_prefix_edge(W):
    for thr in js.LONGEST[W]:
        case = js.prefix_case(W, thr)
        lt, rt = js.build_tables(case, CPU)
        print(case["name"], js.check_prefix(case, lt, rt))
        js.check_prefix_hits(case, js.case_oracle(case))


@pytest.mark.parametrize("kind", ["raw", "levels"])
@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("dense", [False, True])
def test_hash_clusters(kind, W, dense):
    case = js.cluster_case(W, kind, dense)
    lt, rt = js.build_tables(case, CPU, index=case.get("index"))
    print(case["name"], js.check_cluster(case, lt, rt))
    for thr in case["thrs"]:
        want = js.case_oracle(case, thr)
        assert len(np.unique(want["j"])) == 64, "a right row of the tile has no hit"
        n_left = len(case["left"] if kind == "raw" else case["left"][0])
        assert len(np.unique(want["i"])) < n_left, "every left row hits: no candidate fails"


@pytest.mark.parametrize("kind", ["raw", "levels"])
@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("variant", ["at", "over", "partial"])
def test_dense_rule(kind, W, variant):
    case = js.dense_case(W, kind, variant)
    lt, rt = js.build_tables(case, CPU)
    print(case["name"], js.check_dense(case, lt, rt))
    js.check_dense_hits(case, js.case_oracle(case))


@pytest.mark.parametrize("W", [16, 32])
@pytest.mark.parametrize("layout", ["alone", "last", "all"])
def test_candidate_queues(W, layout):
    for c in js.F_DEPTHS:
        case = js.queue_case(W, c, layout)
        lt, rt = js.build_tables(case, CPU)
        for kernel in ("signature", "index"):
            js.check_queue(case, lt, rt, kernel)
        js.check_queue_hits(case, js.case_oracle(case))


@pytest.mark.parametrize("W", [16, 32])
def test_candidate_queues_across_ranges(W):
    for kernel, case in js.queue_straddle_cases(W):
        lt, rt = js.build_tables(case, CPU)
        print(case["name"], kernel, js.check_queue(case, lt, rt, kernel, straddle=True))
        js.check_queue_hits(case, js.case_oracle(case))
        if case.get("partition"):
            ss = js.column(lt, "seg_start")
            assert lt.n > 512 and ss[1] < 512 < ss[2], "the chunk boundary does not cut the category segment"


@pytest.mark.parametrize("W", [16, 32])
def test_signature_run_lengths(W):
    case = js.run_case(W)
    lt, rt = js.build_tables(case, CPU)
    m = js.check_runs(case, lt, rt)
    print(case["name"], m)
    js.check_runs_hits(case, js.case_oracle(case), lt, m["runs"])
