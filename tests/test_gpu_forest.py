"""Merge forests on the GPU (``nsm_span_hits``, csrc/span.hip) against the definition: the records of the Prim reference in
tests/support/merge_forest.py, bitwise, on every family (tests/test_cpu_forest.py checks ``grid.forest_of_hits``, the
properties and the families against that reference).

The C entry is called through ctypes with buffers of exactly the documented sizes: ``forest`` holds max(nodes - 1, 0)
records and ``label`` ``nodes`` words, each followed by sentinel words that must be unchanged; the inputs must be
byte-identical afterwards.  ``stats`` must equal the model (records with ``score >= min_score``; forest records =
``nodes`` - components) and the rounds must stay inside ceil(log2(max(nodes, 2))) + 1.  The Python layers are compared with
``forest_of_hits`` of the hit lists the corresponding grid or ``compare`` returns."""
import random

import numpy as np
import pandas as pd
import pytest

from support import arena as arena_mod
from support import merge_forest as mf
from support import probe_tables
from support import threshold_probes as tp

pytestmark = pytest.mark.gpu
BADARG, UNSUPPORTED = 10001, 10002
NO_COMPACT = 1
SENTINEL = -7
SENTINEL_SCORE = -77.5


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _upload(dev, lists):
    """(ctypes array of descriptors, the device tensors behind them)."""
    import torch

    from napkon_string_matching_amd import _lib

    descs = (_lib.NsmHitList * max(1, len(lists)))()
    keep = []
    for slot, l in zip(descs, lists):
        recs = torch.from_numpy(l.records()).to(dev) if len(l) else None
        keep.append(recs)
        slot.hits, slot.n = (recs.data_ptr() if recs is not None else None), len(l)
        slot.left_base, slot.left_ids, slot.right_base, slot.right_ids = l.left_base, l.left_ids, l.right_base, l.right_ids
    return descs, keep


def _entry(dev, lists, nodes, min_score, flags=0, stats0=(0, 0, 0, 0), with_stats=True, with_label=True):
    """``nsm_span_hits``: (status, count, the records as written, the labels, stats).  ``forest`` has room for
    max(nodes - 1, 0) records and 2 sentinel records behind them, ``label`` 4 sentinel words behind its ``nodes``; every
    record and word starts as a sentinel.  The inputs must be byte-identical afterwards."""
    import torch

    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_span_hits")
    descs, keep = _upload(dev, lists)
    room = max(nodes - 1, 0)
    forest = torch.full((room + 2, 2), SENTINEL_SCORE, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    label = torch.full((nodes + 4,), SENTINEL, dtype=torch.int32, device=dev)
    st = torch.tensor(list(stats0), dtype=torch.int64, device=dev)
    rc = fn(descs, len(lists), nodes, float(min_score), flags, forest.data_ptr(), count.data_ptr(),
            label.data_ptr() if with_label else None, st.data_ptr() if with_stats else None, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for l, recs in zip(lists, keep):
        if recs is not None:
            assert np.array_equal(recs.cpu().numpy().view(np.int64), l.records().view(np.int64)), "the input was written"
    n = int(count.item())
    host = forest.cpu().numpy()
    assert 0 <= n <= room
    assert (host[n:] == SENTINEL_SCORE).all(), "wrote beyond the count (or beyond the buffer)"
    ij = host.view(np.int32).reshape(-1, 4)
    lab = label.cpu().numpy()
    assert (lab[nodes:] == SENTINEL).all(), "wrote beyond the nodes"
    return rc, n, (host[:n, 0].copy(), ij[:n, 2].copy(), ij[:n, 3].copy()), lab[:nodes], [int(v) for v in st.tolist()]


# ------------------------------------------------------------------------------------------------------------ C entry
@pytest.mark.parametrize("name", mf.NAMES)
def test_entry_equals_the_definition(dev, name):
    c, want, want_label = mf.case(name), mf.answer(name), mf.labels(name)
    rc, n, records, label, stats = _entry(dev, c.lists, c.nodes, c.min_score)
    assert rc == 0
    assert n == c.nodes - mf.components(want_label) == len(want[0])
    assert mf.same_records(mf.canonical(*records), want), name
    assert np.array_equal(label, want_label), f"{name}: first difference at node {int(np.flatnonzero(label != want_label)[0])}"
    assert stats[:2] == [mf.counted(c), n], (name, stats)
    edges = len(mf.edges_of(c.lists, c.min_score))
    if edges:
        assert 1 <= stats[2] <= mf.round_bound(c.nodes), (name, stats)
        assert stats[3] == edges * stats[2]  # (every round visits every edge: dropping dead ones did not pay)
    else:
        assert stats[2:] == [0, 0]
    if name == "hierarchy_1024":
        assert stats[2] >= 10
    # NSM_SPAN_NO_COMPACT: the same records, no fewer visits
    rc, n2, records2, label2, stats2 = _entry(dev, c.lists, c.nodes, c.min_score, flags=NO_COMPACT)
    assert rc == 0 and n2 == n and mf.same_records(mf.canonical(*records2), want) and np.array_equal(label2, want_label)
    assert stats2[:2] == stats[:2] and stats2[3] >= stats[3] and stats2[3] == edges * stats2[2]
    assert stats2[2] <= mf.round_bound(c.nodes) and (stats2[2] >= 1) == (edges > 0)


def test_stats_are_added_to_and_stats_and_label_may_be_null(dev):
    c, want = mf.case("one_pair_two_bases"), mf.answer("one_pair_two_bases")
    rc, n, records, label, stats = _entry(dev, c.lists, c.nodes, c.min_score, stats0=(100, 200, 300, 400))
    assert rc == 0 and mf.same_records(mf.canonical(*records), want)
    assert (mf.counted(c), len(want[0])) == (13, 10)
    assert stats[:2] == [100 + 13, 200 + 10] and stats[2] > 300 and stats[3] >= 400 + 13
    rc, n, records, label, stats = _entry(dev, c.lists, c.nodes, c.min_score, stats0=(5, 6, 7, 8), with_stats=False)
    assert rc == 0 and stats == [5, 6, 7, 8] and mf.same_records(mf.canonical(*records), want)
    assert np.array_equal(label, mf.labels("one_pair_two_bases"))
    rc, n, records, label, stats = _entry(dev, c.lists, c.nodes, c.min_score, with_label=False)
    assert rc == 0 and (label == SENTINEL).all() and mf.same_records(mf.canonical(*records), want) and stats[1] == 10


def test_no_lists_and_one_node(dev):
    rc, n, records, label, stats = _entry(dev, [], 70, 0.0)
    assert rc == 0 and n == 0 and label.tolist() == list(range(70)) and stats == [0, 0, 0, 0]
    loop = mf.same_space([0.5, 0.7], [0, 0], [0, 0], 1)
    rc, n, records, label, stats = _entry(dev, [loop], 1, 0.0)  # (forest has room for no record)
    assert rc == 0 and n == 0 and label.tolist() == [0] and stats == [2, 0, 0, 0]


@pytest.mark.parametrize("which,where,field,value", [
    (0, "first", "i", "left_ids"), (1, "last", "j", "right_ids"), (2, "first", "i", -1), (1, "middle", "j", -5),
    (1, "middle", "i", 2 ** 31 - 1)])
def test_an_id_out_of_range_is_refused_before_anything_is_written(dev, which, where, field, value):
    from napkon_string_matching_amd import _lib

    c = mf.case("one_pair_two_bases")
    lists = list(c.lists)
    l = lists[which]
    r = {"first": 0, "last": len(l) - 1, "middle": len(l) // 2}[where]
    i, j, score = l.i.copy(), l.j.copy(), l.score.copy()
    (i if field == "i" else j)[r] = getattr(l, value) if isinstance(value, str) else value
    score[r] = -1.0  # below min_score: ALL records are checked, whatever their score
    lists[which] = mf.HitList(score, i, j, l.left_base, l.left_ids, l.right_base, l.right_ids)
    for flags in (0, NO_COMPACT):
        rc, n, records, label, stats = _entry(dev, lists, c.nodes, 0.5, flags=flags, stats0=(21, 22, 23, 24))
        assert rc == BADARG and "outside" in _lib.load().nsm_last_error().decode()
        assert n == 0 and stats == [21, 22, 23, 24] and (label == SENTINEL).all()  # (_entry has checked every forest record)


def test_a_capturing_stream_is_refused_before_any_launch(dev):
    import torch

    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_span_hits")
    c = mf.case("one_pair_two_bases")
    descs, keep = _upload(dev, c.lists)
    forest = torch.full((c.nodes - 1, 2), SENTINEL_SCORE, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    label = torch.full((c.nodes,), SENTINEL, dtype=torch.int32, device=dev)
    st = torch.tensor([11, 12, 13, 14], dtype=torch.int64, device=dev)
    other = torch.zeros(8, device=dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            other.add_(1.0)  # (a graph of one node: the refused call adds none)
            rc = fn(descs, len(c.lists), c.nodes, 0.5, 0, forest.data_ptr(), count.data_ptr(), label.data_ptr(), st.data_ptr(),
                    stream.cuda_stream)
        graph.replay()
    torch.cuda.synchronize(dev)
    assert rc == UNSUPPORTED and "captured" in _lib.load().nsm_last_error().decode()
    assert (label == SENTINEL).all() and st.tolist() == [11, 12, 13, 14] and other.tolist() == [1.0] * 8
    assert int(count.item()) == 0 and (forest == SENTINEL_SCORE).all()


# ---------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("name", mf.FAMILIES)
def test_guard_bands(dev, name):
    """Everything the entry is handed lies in one arena of random bytes: every list's records, ``forest`` carved at exactly
    16 * (nodes - 1) bytes, the count at 8, ``label`` at 4 * nodes, the stats at 32.  The records are byte-identical
    afterwards, no guard byte has changed."""
    import torch

    from napkon_string_matching_amd import _lib

    c, want, want_label = mf.case(name), mf.answer(name), mf.labels(name)
    room = sum(len(l) * 16 for l in c.lists) + 16 * (c.nodes - 1) + 8 + 4 * c.nodes + 32 + \
        (len(c.lists) + 5) * (arena_mod.GUARD + arena_mod.ALIGN)
    arena = arena_mod.Arena(room, dev, seed=19)
    descs = (_lib.NsmHitList * len(c.lists))()
    names = []
    for k, (slot, l) in enumerate(zip(descs, c.lists)):
        if len(l):
            arena.carve(f"hits{k}", len(l) * 16)
            arena.fill(f"hits{k}", l.records())
            names.append(f"hits{k}")
        slot.hits, slot.n = (arena.ptr(f"hits{k}") if len(l) else None), len(l)
        slot.left_base, slot.left_ids, slot.right_base, slot.right_ids = l.left_base, l.left_ids, l.right_base, l.right_ids
    arena.carve("forest", 16 * (c.nodes - 1))
    arena.carve("count", 8)
    arena.zero("count")
    arena.carve("label", 4 * c.nodes)
    arena.carve("stats", 32)
    arena.zero("stats")
    rc = _lib.entry("nsm_span_hits")(descs, len(c.lists), c.nodes, float(c.min_score), 0, arena.ptr("forest"), arena.ptr("count"),
                                     arena.ptr("label"), arena.ptr("stats"), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert rc == 0
    arena.check(unchanged=names)
    n = int(arena.read("count", np.int64)[0])
    assert n == len(want[0])
    recs = arena.read("forest", np.float64).reshape(-1, 2)
    ij = recs.view(np.int32).reshape(-1, 4)
    assert mf.same_records(mf.canonical(recs[:n, 0], ij[:n, 2], ij[:n, 3]), want)
    # the records beyond the count still hold the arena's bytes
    assert np.array_equal(arena.read("forest")[16 * n:], arena.poison("forest")[16 * n:])
    assert np.array_equal(arena.read("label", np.int32), want_label)
    assert arena.read("stats", np.int64).tolist()[:2] == [mf.counted(c), n]


# ------------------------------------------------------------------------------------------------------- decomposition
@pytest.mark.parametrize("name", ["one_pair_two_bases", "empty_among", "tied_at_0.25", "every_record_thrice", "hierarchy_1024"])
def test_decomposition_one_list_per_call_equals_one_call(dev, name):
    c, want = mf.case(name), mf.answer(name)
    lists = c.lists
    if len(lists) == 1:  # one list: its records in three parts
        l = lists[0]
        cut = [0, len(l) // 3, len(l) // 2, len(l)]
        lists = [mf.HitList(l.score[a:b], l.i[a:b], l.j[a:b], l.left_base, l.left_ids, l.right_base, l.right_ids)
                 for a, b in zip(cut, cut[1:])]
    records = None
    for k, l in enumerate(lists):
        fed = [l] + ([] if records is None else [mf.as_list(records, c.nodes)])  # (the forest as the device wrote it)
        rc, n, records, label, _ = _entry(dev, fed, c.nodes, c.min_score)
        assert rc == 0
        assert mf.same_records(mf.canonical(*records), mf.prim_forest(lists[:k + 1], c.nodes, c.min_score)), (name, k)
        assert np.array_equal(label, mf.bfs_labels(lists[:k + 1], c.nodes, c.min_score))
    assert mf.same_records(mf.canonical(*records), want)


# ------------------------------------------------------------------------------------------------------- Python layers
@pytest.mark.parametrize("name", ["one_pair_two_bases", "path_shuffled", "tied_at_0.75", "empty_among", "distinct_1", "signed_zeros",
                                  "bipartite_300x300"])
def test_span_hits_on_host_lists(dev, name):
    from napkon_string_matching_amd import grid

    c, want = mf.case(name), mf.answer(name)
    stats = []
    got = grid.span_hits(c.entries(), c.nodes, c.min_score, device=dev, stats=stats)
    assert isinstance(got, grid.MergeForest) and got.score.dtype == np.float64 and got.u.dtype == np.int32
    assert mf.same_records((got.score, got.u, got.v), want)  # ordered on the device
    assert got.nodes == c.nodes and got.min_score == c.min_score and got.bases == (0,) and got.cohort_sizes == (c.nodes,)
    assert stats[:2] == [mf.counted(c), len(want[0])]
    assert np.array_equal(got.cut(c.min_score).label, mf.labels(name))


def test_span_hits_refuses_bad_lists(dev):
    from napkon_string_matching_amd import grid

    hits = lambda i, j: grid.Hits(np.array([0.5]), np.array([i], dtype=np.int32), np.array([j], dtype=np.int32))
    for i, j in ((-1, 0), (0, -1), (5, 0), (0, 3)):
        with pytest.raises(ValueError):
            grid.span_hits([(hits(i, j), 0, 2)], 5, device=dev)
    assert len(grid.span_hits([], 0, device=dev)) == 0
    assert len(grid.span_hits([], 3, device=dev)) == 0
    stats = []
    assert grid.span_hits([(hits(1, 0), 0, 2)], 5, device=dev, stats=stats).as_tuples() == [(0.5, 1, 2)] and stats[:2] == [1, 1]


GRIDS = ["raw_indel_64", "raw_jaccard_16", "levels_indel_one_word", "levels_jaccard"]


def _grid_calls(g, dev):
    """(grid(thr), forest(thr, **kw), groups(thr, **kw)) of a probe grid through the wrappers of its mode."""
    from napkon_string_matching_amd import grid

    cap = g.pairs
    if g.raw:
        lt, rt = probe_tables.raw_indel_tables(g, dev) if g.kind == "indel" else probe_tables.raw_jaccard_tables(g, dev)
        full, forest, groups = (grid.indel_raw_grid, grid.indel_raw_forest, grid.indel_raw_groups) if g.kind == "indel" else \
            (grid.jaccard_raw_grid, grid.jaccard_raw_forest, grid.jaccard_raw_groups)
        return (lambda thr: full(lt, rt, thr, capacity=cap), lambda thr, **kw: forest(lt, rt, thr, capacity=cap, **kw),
                lambda thr, **kw: groups(lt, rt, thr, capacity=cap, **kw))
    tabs = probe_tables.levels_indel_tables(g, dev, False) if g.kind == "indel" else probe_tables.levels_jaccard_tables(g, dev, False)
    full, forest, groups = (grid.indel_levels_grid, grid.indel_levels_forest, grid.indel_levels_groups) if g.kind == "indel" else \
        (grid.jaccard_levels_grid, grid.jaccard_levels_forest, grid.jaccard_levels_groups)
    return (lambda thr: full(*tabs, thr, category_mode=g.mode, capacity=cap),
            lambda thr, **kw: forest(*tabs, thr, category_mode=g.mode, capacity=cap, **kw),
            lambda thr, **kw: groups(*tabs, thr, category_mode=g.mode, capacity=cap, **kw))


@pytest.mark.parametrize("thr", [0.3, 0.6])
@pytest.mark.parametrize("name", GRIDS)
def test_table_forests_equal_the_definition_on_the_grids_hits(dev, name, thr):
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    n_l, n_r = len(g.left), len(g.right)
    full, forest, groups = _grid_calls(g, dev)
    hits = full(thr)
    assert len(hits) > 0
    same = lambda a, b: mf.same_records((a.score, a.u, a.v), (b.score, b.u, b.v))
    # two cohorts: left item k is node k, right item k node n_l + k
    stats = []
    got = forest(thr, stats=stats)
    want = grid.forest_of_hits([(hits, 0, n_l)], n_l + n_r, float("-inf"))
    assert got.bases == (0, n_l) and got.cohort_sizes == (n_l, n_r) and got.nodes == n_l + n_r and got.min_score == thr
    assert same(got, want) and len(got) > 0
    assert stats[:2] == [len(hits), len(want)] and 1 <= stats[2] <= mf.round_bound(n_l + n_r)
    # cut(t) is what the groups entry says at min_score = t, on the same tables
    floors = sorted({thr, float(np.median(hits.score)), float(hits.score.max()), float(np.nextafter(hits.score.max(), np.inf))})
    for t in floors:
        cut = got.cut(t)
        assert np.array_equal(cut.label, groups(thr, min_score=t).label), (name, thr, t)
        assert cut.bases == (0, n_l) and cut.cohort_sizes == (n_l, n_r)
    with pytest.raises(ValueError):
        got.cut(float(np.nextafter(thr, -np.inf)))
    # one node space (left item k and right item k are one node): records (k, k) are no edges
    one = forest(thr, same=True)
    assert one.bases == (0,) and one.cohort_sizes == (n_r,) and same(one, grid.forest_of_hits([(hits, 0, 0)], n_r, float("-inf")))
    # only the records at or above a higher floor are edges: the prefix
    floor = float(np.median(hits.score))
    high = forest(thr, min_score=floor)
    keep = want.score >= floor
    assert high.min_score == floor and mf.same_records((high.score, high.u, high.v), (want.score[keep], want.u[keep], want.v[keep]))
    if g.raw and g.kind == "indel":  # a small first buffer: the grid's retry ends in the same forest
        lt, rt = probe_tables.raw_indel_tables(g, dev)
        assert same(grid.indel_raw_forest(lt, rt, thr, capacity=8), want)


def test_fuzzy_match_forest_and_cluster_tree_with_and_without_a_wide_item(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match

    rng = random.Random(21)
    text = lambda k: " ".join("".join(rng.choice("abcde") for _ in range(rng.randint(2, 6))) for _ in range(k))
    left, right = [text(rng.randint(1, 4)) for _ in range(12)], [text(rng.randint(1, 4)) for _ in range(14)]
    right[5], right[9] = left[2], left[2]
    items = left + [left[2], left[7] + "x", right[3]]
    same = lambda a, b: mf.same_records((a.score, a.u, a.v), (b.score, b.u, b.v))
    for wide in (False, True):
        if wide:
            left[3] = "x" * 513  # beyond the fast kernels: the general route, the merged list spanned
            items[3] = "x" * 513
            items.append("x" * 512 + "y")
        thr = 0.4
        hits = fuzzy_match.raw_grid(left, right, thr, device=dev)
        got = fuzzy_match.forest(left, right, thr, device=dev)
        assert got.bases == (0, 12) and got.cohort_sizes == (12, 14) and got.min_score == thr
        assert same(got, grid.forest_of_hits([(hits, 0, 12)], 26, thr)) and len(got) > 0
        assert (got.merge_score([2, 2], [12 + 5, 12 + 9]) == hits.score.max()).all()  # (identical strings: a direct edge)
        self_hits = fuzzy_match.raw_grid(items, items, thr, device=dev)
        tree = fuzzy_match.cluster_tree(items, thr, device=dev)
        assert tree.bases == (0,) and tree.cohort_sizes == (len(items),)
        assert same(tree, grid.forest_of_hits([(self_hits, 0, 0)], len(items), thr))
        for t in (0.4, 0.8):  # the tree cut at t is the clusters at t
            clusters = fuzzy_match.clusters(items, t, device=dev)
            assert [c.tolist() for c in clusters] == [m[0].tolist() for m in tree.cut(t).members(2)]
        if wide:
            assert tree.merge_score([3], [len(items) - 1])[0] > 0.9
    assert len(fuzzy_match.cluster_tree([], 0.5, device=dev)) == 0
    empty = fuzzy_match.forest([], right, 0.5, device=dev)
    assert len(empty) == 0 and empty.nodes == 14 and empty.cut(0.5).label.tolist() == list(range(14))


def test_intersection_vs_union_forest_and_cluster_tree_with_and_without_a_wide_item(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import intersection_vs_union

    rng = random.Random(22)
    words = [f"w{q}" for q in range(10)]
    row = lambda: rng.sample(words, rng.randint(1, 4))
    left, right = [row() for _ in range(12)], [row() for _ in range(14)]
    right[5] = list(left[2])
    many = [f"x{q}" for q in range(70)]
    items = left + [list(left[2])]
    same = lambda a, b: mf.same_records((a.score, a.u, a.v), (b.score, b.u, b.v))
    for wide in (False, True):
        if wide:
            left[4], right[6] = many[:65], many[3:68] + words[:2]  # 65 distinct tokens and more: the general route
            items[4] = many[:65]
            items.append(many[1:66])
        thr = 0.3
        hits = intersection_vs_union.raw_grid(left, right, thr, device=dev)
        got = intersection_vs_union.forest(left, right, thr, device=dev)
        assert got.bases == (0, 12) and same(got, grid.forest_of_hits([(hits, 0, 12)], 26, thr)) and len(got) > 0
        assert got.merge_score([2], [12 + 5])[0] == 1.0
        self_hits = intersection_vs_union.raw_grid(items, items, thr, device=dev)
        tree = intersection_vs_union.cluster_tree(items, thr, device=dev)
        assert same(tree, grid.forest_of_hits([(self_hits, 0, 0)], len(items), thr))
        for t in (0.3, 0.6):
            clusters = intersection_vs_union.clusters(items, t, device=dev)
            assert [c.tolist() for c in clusters] == [m[0].tolist() for m in tree.cut(t).members(2)]
        if wide:
            assert got.merge_score([4], [12 + 6])[0] > 0.8 and tree.merge_score([4], [len(items) - 1])[0] > 0.9


# ------------------------------------------------------------------------------------------------------------ Matcher
def _cohort(seed, n, words):
    rng = random.Random(seed)
    rows = []
    for k in range(n):
        toks = [rng.choice(words) for _ in range(rng.randint(1, 6))]
        term = [" ".join(toks[q:q + 2]) for q in range(0, len(toks), 2)]
        rows.append([f"{seed}-{k}", f"v{k}", "s", [f"c{k % 3}"], term, toks, "p"])
    return pd.DataFrame(rows, columns=["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"])


def test_matcher_match_forest_on_three_cohorts(dev):
    """``match_forest(m).mapping(t).dict() == match_groups(min_score=t).dict()`` for t >= m, and the forest is
    ``forest_of_hits(lists_of_results(results))``."""
    from napkon_string_matching_amd import grid, groups
    from napkon_string_matching_amd.matcher import Matcher
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    words = [f"word{q}" for q in range(12)]
    cohorts = {"Pop": Questionnaire(_cohort(2, 25, words)), "hap": Questionnaire(_cohort(1, 20, words)),
               "suep": Questionnaire(_cohort(3, 22, words))}
    matching = dict(score_func="fuzzy_match", compare_column="Term", score_threshold=0.6, cached=False)
    matcher = Matcher(None, {"matching": matching}, questionnaires=cohorts)
    matcher.match_questionnaires()
    assert len(matcher.results) == 3
    names, identifiers, lists = groups.lists_of_results(matcher.results)
    nodes = sum(len(v) for v in identifiers)
    held = matcher.match_forest()
    assert isinstance(held, groups.ResultForest) and held.cohorts == names and held.identifiers == identifiers
    want = grid.forest_of_hits(lists, nodes, float("-inf"))
    assert mf.same_records((held.forest.score, held.forest.u, held.forest.v), (want.score, want.u, want.v)) and len(want) > 0
    assert held.forest.cohort_sizes == tuple(len(v) for v in identifiers) and held.forest.nodes == nodes
    for t in (0.6, 0.75):
        assert held.mapping(t).dict() == matcher.match_groups(min_score=t).dict() and len(held.mapping(0.6)) > 0
    assert held.mapping(float("-inf")).dict() == matcher.match_groups().dict()
    everything = matcher.match_groups()
    assert held.mapping(0.75, id_reference=everything).dict() == matcher.match_groups(min_score=0.75, id_reference=everything).dict()
    ladder = held.ladder([0.6, 0.75, 0.9])
    assert ladder["groups"].tolist() == [len(held.mapping(t)) for t in (0.6, 0.75, 0.9)]
    assert (np.diff(ladder["components"]) >= 0).all() and ladder["components"][0] == nodes - int((want.score >= 0.6).sum())
    # from a floor: the prefix of the full forest, and nothing below it
    high = matcher.match_forest(min_score=0.75)
    assert high.mapping(0.75).dict() == matcher.match_groups(min_score=0.75).dict()
    assert len(high.forest) == int((want.score >= 0.75).sum())
    with pytest.raises(ValueError):
        high.mapping(0.7)
