"""Match groups on the GPU (``nsm_group_hits``, csrc/groups.hip) against the definition: the labels of the breadth-first
reference in tests/support/match_groups.py, element for element, on every family (tests/test_cpu_groups.py checks
``grid.groups_of_hits`` and the families against that reference).

The C entry is called through ctypes with buffers of exactly the documented sizes; ``stats`` must equal the model (records
with ``score >= min_score``; hooks = components before - components after).  The Python layers are compared with
``groups_of_hits`` of the hit lists the corresponding grid or ``compare`` returns."""
import random

import numpy as np
import pandas as pd
import pytest

from support import arena as arena_mod
from support import match_groups as mg
from support import probe_tables
from support import threshold_probes as tp

pytestmark = pytest.mark.gpu
BADARG, UNSUPPORTED = 10001, 10002
CONTINUE = 1
SENTINEL = -7


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


def _entry(dev, lists, nodes, min_score, flags=0, label0=None, stats0=(0, 0), with_stats=True):
    """``nsm_group_hits``: (status, the ``nodes`` labels, stats).  ``label`` starts as ``label0`` or as sentinels and has
    4 sentinel words behind it; the inputs must be byte-identical afterwards."""
    import torch

    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_group_hits")
    descs, keep = _upload(dev, lists)
    label = torch.full((nodes + 4,), SENTINEL, dtype=torch.int32, device=dev)
    if label0 is not None:
        label[:nodes] = torch.from_numpy(np.asarray(label0, dtype=np.int32)).to(dev)
    st = torch.tensor(list(stats0), dtype=torch.int64, device=dev)
    rc = fn(descs, len(lists), nodes, float(min_score), flags, label.data_ptr(), st.data_ptr() if with_stats else None,
            torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    for l, recs in zip(lists, keep):
        if recs is not None:
            assert np.array_equal(recs.cpu().numpy().view(np.int64), l.records().view(np.int64)), "the input was written"
    host = label.cpu().numpy()
    assert (host[nodes:] == SENTINEL).all(), "wrote beyond the nodes"
    return rc, host[:nodes], [int(v) for v in st.tolist()]


# ------------------------------------------------------------------------------------------------------------ C entry
@pytest.mark.parametrize("name", mg.NAMES)
def test_entry_equals_the_definition(dev, name):
    c, want = mg.case(name), mg.answer(name)
    rc, label, stats = _entry(dev, c.lists, c.nodes, c.min_score)
    assert rc == 0
    assert np.array_equal(label, want), f"{name}: first difference at node {int(np.flatnonzero(label != want)[0])}"
    assert stats == [mg.counted(c), c.nodes - mg.components(want)], (name, stats)


def test_stats_are_added_to_and_may_be_null(dev):
    c, want = mg.case("pairs_1025"), mg.answer("pairs_1025")
    rc, label, stats = _entry(dev, c.lists, c.nodes, c.min_score, stats0=(100, 200))
    assert rc == 0 and stats == [100 + 1025, 200 + 1025] and np.array_equal(label, want)
    rc, label, stats = _entry(dev, c.lists, c.nodes, c.min_score, stats0=(5, 6), with_stats=False)
    assert rc == 0 and stats == [5, 6] and np.array_equal(label, want)


@pytest.mark.parametrize("name", ["three_cohorts", "empty_among", "path_shuffled", "bipartite_300x300"])
def test_continue_one_list_per_call_equals_one_call(dev, name):
    c, want = mg.case(name), mg.answer(name)
    lists = c.lists
    if len(lists) == 1:  # one list: its records in three parts
        l = lists[0]
        cut = [0, len(l) // 3, len(l) // 2, len(l)]
        lists = [mg.HitList(l.score[a:b], l.i[a:b], l.j[a:b], l.left_base, l.left_ids, l.right_base, l.right_ids)
                 for a, b in zip(cut, cut[1:])]
    label, total = None, [0, 0]
    for k, l in enumerate(lists):
        before = c.nodes if label is None else mg.components(label)
        rc, label, total = _entry(dev, [l], c.nodes, c.min_score, flags=0 if k == 0 else CONTINUE, label0=label, stats0=total)
        assert rc == 0
        assert np.array_equal(label, mg.bfs_labels(lists[:k + 1], c.nodes, c.min_score)), (name, k)
        assert before - mg.components(label) >= 0
    assert np.array_equal(label, want)
    assert total == [mg.counted(c), c.nodes - mg.components(want)]  # the hooks of all calls: components lost in all


def test_continue_without_lists_normalises_a_forest(dev):
    forest = np.array([0, 0, 1, 2, 4, 4, 5, 7, 3], dtype=np.int32)
    rc, label, stats = _entry(dev, [], 9, 0.0, flags=CONTINUE, label0=forest)
    assert rc == 0 and label.tolist() == [0, 0, 0, 0, 4, 4, 4, 7, 0] and stats == [0, 0]
    # a deep forest over several blocks: every node points at its predecessor
    chain = np.maximum(np.arange(5000) - 1, 0).astype(np.int32)
    rc, label, _ = _entry(dev, [], 5000, 0.0, flags=CONTINUE, label0=chain)
    assert rc == 0 and (label == 0).all()
    # ... and lists linked into a forest that is not flat
    c = mg.case("self_loops")
    start = np.arange(200, dtype=np.int32)
    start[[60, 61, 62]] = [5, 60, 61]
    rc, label, stats = _entry(dev, c.lists, 200, 0.5, flags=CONTINUE, label0=start)
    want = mg.bfs_labels(c.lists, 200, 0.5, start=start)
    assert rc == 0 and np.array_equal(label, want) and label[62] == 5
    assert stats == [mg.counted(c), mg.components(start) - mg.components(want)]


def test_without_continue_label_is_output_only(dev):
    c = mg.case("nodes_257")
    garbage = np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, c.nodes).astype(np.int32)
    rc, label, _ = _entry(dev, c.lists, c.nodes, c.min_score, label0=garbage)
    assert rc == 0 and np.array_equal(label, mg.answer("nodes_257"))
    rc, label, stats = _entry(dev, [], 70, 0.0, label0=garbage[:70])  # no lists at all: every word is still written
    assert rc == 0 and label.tolist() == list(range(70)) and stats == [0, 0]


# ------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_in_the_documented_order(dev):
    import torch

    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_group_hits")
    error = lambda: _lib.load().nsm_last_error().decode()
    c = mg.case("three_cohorts")
    descs, keep = _upload(dev, c.lists)
    label = torch.full((c.nodes,), SENTINEL, dtype=torch.int32, device=dev)
    st = torch.tensor([11, 12], dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda lists, n_lists, nodes, flags, lab: fn(lists, n_lists, nodes, 0.0, flags, lab, st.data_ptr(), stream)
    ptr = label.data_ptr()

    def broken(**fields):
        copy = (_lib.NsmHitList * 3)(*[_lib.NsmHitList(d.hits, d.n, d.left_base, d.left_ids, d.right_base, d.right_ids) for d in descs])
        for key, value in fields.items():
            setattr(copy[1], key, value)
        return copy

    assert call(None, 3, c.nodes, 0, ptr) == BADARG and "null lists" in error()
    assert call(descs, -1, c.nodes, 0, ptr) == BADARG and "negative count" in error()
    assert call(descs, 3, -1, 0, ptr) == BADARG and "negative count" in error()
    assert call(descs, 3, c.nodes, 0, None) == BADARG and "null label" in error()
    assert call(descs, 3, c.nodes, 4, ptr) == BADARG and "flag" in error()
    assert call(broken(hits=None), 3, c.nodes, 0, ptr) == BADARG and "list 1 has null hits" in error()
    for field in ("left_base", "left_ids", "right_base", "right_ids"):
        assert call(broken(**{field: -1}), 3, c.nodes, 0, ptr) == BADARG and "list 1 has a negative" in error()
    assert call(broken(right_ids=46), 3, c.nodes, 0, ptr) == BADARG and "list 1 reaches beyond" in error()
    assert call(descs, 3, c.nodes - 1, 0, ptr) == BADARG and "reaches beyond" in error()
    # earlier checks win
    assert call(None, 3, -1, 4, None) == BADARG and "null lists" in error()
    assert call(broken(hits=None), 3, -1, 4, None) == BADARG and "negative count" in error()
    assert call(broken(hits=None), 3, c.nodes, 4, None) == BADARG and "null label" in error()
    assert call(broken(hits=None, left_base=-1), 3, c.nodes, 4, ptr) == BADARG and "flag" in error()
    assert call(broken(hits=None, left_base=-1), 3, c.nodes, 0, ptr) == BADARG and "null hits" in error()
    assert call(broken(left_base=-1, right_ids=1000), 3, c.nodes, 0, ptr) == BADARG and "negative" in error()
    assert call(None, 0, 0, 0, None) == 0  # nodes == 0
    torch.cuda.synchronize(dev)
    assert (label == SENTINEL).all() and st.tolist() == [11, 12], "a refused call wrote"
    assert call(descs, 3, c.nodes, 0, ptr) == 0  # (and the buffers the refusals were handed are good ones)
    torch.cuda.synchronize(dev)
    assert np.array_equal(label.cpu().numpy(), mg.answer("three_cohorts"))


@pytest.mark.parametrize("flags", [0, CONTINUE])
@pytest.mark.parametrize("which,where,field,value", [
    (0, "first", "i", "left_ids"), (1, "last", "j", "right_ids"), (2, "first", "i", -1), (1, "middle", "j", -5),
    (1, "middle", "i", 2 ** 31 - 1)])
def test_an_id_out_of_range_is_refused_before_anything_is_written(dev, flags, which, where, field, value):
    from napkon_string_matching_amd import _lib

    c = mg.case("three_cohorts")
    lists = list(c.lists)
    l = lists[which]
    r = {"first": 0, "last": len(l) - 1, "middle": len(l) // 2}[where]
    i, j, score = l.i.copy(), l.j.copy(), l.score.copy()
    (i if field == "i" else j)[r] = getattr(l, value) if isinstance(value, str) else value
    score[r] = -1.0  # below min_score: ALL records are checked, whatever their score
    lists[which] = mg.HitList(score, i, j, l.left_base, l.left_ids, l.right_base, l.right_ids)
    start = np.arange(c.nodes, dtype=np.int32)
    start[1] = 0
    rc, label, stats = _entry(dev, lists, c.nodes, 0.5, flags=flags, label0=start if flags else None, stats0=(21, 22))
    assert rc == BADARG and "outside" in _lib.load().nsm_last_error().decode()
    assert stats == [21, 22]
    assert np.array_equal(label, start) if flags else (label == SENTINEL).all()


@pytest.mark.parametrize("node,value", [(0, 1), (1, 2), (134, -1), (70, 71), (70, -2 ** 31)])
def test_a_bad_forest_is_refused_before_anything_is_written(dev, node, value):
    from napkon_string_matching_amd import _lib

    c = mg.case("three_cohorts")
    start = np.arange(c.nodes, dtype=np.int32)
    start[5] = 2
    start[node] = value
    rc, label, stats = _entry(dev, c.lists, c.nodes, 0.5, flags=CONTINUE, label0=start, stats0=(21, 22))
    assert rc == BADARG and "label[v] outside" in _lib.load().nsm_last_error().decode()
    assert np.array_equal(label, start) and stats == [21, 22]


def test_a_capturing_stream_is_refused_before_any_launch(dev):
    import torch

    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_group_hits")
    c = mg.case("three_cohorts")
    descs, keep = _upload(dev, c.lists)
    label = torch.full((c.nodes,), SENTINEL, dtype=torch.int32, device=dev)
    st = torch.tensor([11, 12], dtype=torch.int64, device=dev)
    other = torch.zeros(8, device=dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            other.add_(1.0)  # (a graph of one node: the refused call adds none)
            rc = fn(descs, 3, c.nodes, 0.0, 0, label.data_ptr(), st.data_ptr(), stream.cuda_stream)
        graph.replay()
    torch.cuda.synchronize(dev)
    assert rc == UNSUPPORTED and "captured" in _lib.load().nsm_last_error().decode()
    assert (label == SENTINEL).all() and st.tolist() == [11, 12] and other.tolist() == [1.0] * 8


# ---------------------------------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("name", mg.FAMILIES)
def test_guard_bands(dev, name):
    """Everything the entry is handed lies in one arena of random bytes: every list's records, ``label`` carved at exactly
    4 * nodes bytes, the stats at 16.  The records are byte-identical afterwards, no guard byte has changed."""
    import torch

    from napkon_string_matching_amd import _lib

    c, want = mg.case(name), mg.answer(name)
    room = sum(len(l) * 16 for l in c.lists) + 4 * c.nodes + 16 + (len(c.lists) + 3) * (arena_mod.GUARD + arena_mod.ALIGN)
    arena = arena_mod.Arena(room, dev, seed=17)
    descs = (_lib.NsmHitList * len(c.lists))()
    names = []
    for k, (slot, l) in enumerate(zip(descs, c.lists)):
        if len(l):
            arena.carve(f"hits{k}", len(l) * 16)
            arena.fill(f"hits{k}", l.records())
            names.append(f"hits{k}")
        slot.hits, slot.n = (arena.ptr(f"hits{k}") if len(l) else None), len(l)
        slot.left_base, slot.left_ids, slot.right_base, slot.right_ids = l.left_base, l.left_ids, l.right_base, l.right_ids
    arena.carve("label", 4 * c.nodes)
    arena.carve("stats", 16)
    arena.zero("stats")
    rc = _lib.entry("nsm_group_hits")(descs, len(c.lists), c.nodes, float(c.min_score), 0, arena.ptr("label"), arena.ptr("stats"),
                                      torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert rc == 0
    arena.check(unchanged=names)
    assert np.array_equal(arena.read("label", np.int32), want)
    assert arena.read("stats", np.int64).tolist() == [mg.counted(c), c.nodes - mg.components(want)]


# ------------------------------------------------------------------------------------------------------- Python layers
@pytest.mark.parametrize("name", ["three_cohorts", "path_shuffled", "ladder_at_0.75", "empty_among", "nodes_1"])
def test_group_hits_on_host_lists(dev, name):
    from napkon_string_matching_amd import grid

    c, want = mg.case(name), mg.answer(name)
    stats = []
    got = grid.group_hits(c.entries(), c.nodes, c.min_score, device=dev, stats=stats)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert stats == [mg.counted(c), c.nodes - mg.components(want)]
    # fed one list at a time
    label = None
    for entry in c.entries():
        label = grid.group_hits([entry], c.nodes, c.min_score, start=label, device=dev)
    assert np.array_equal(label, want)


def test_group_hits_refuses_bad_lists(dev):
    from napkon_string_matching_amd import grid

    hits = lambda i, j: grid.Hits(np.array([0.5]), np.array([i], dtype=np.int32), np.array([j], dtype=np.int32))
    for i, j in ((-1, 0), (0, -1), (5, 0), (0, 3)):
        with pytest.raises(ValueError):
            grid.group_hits([(hits(i, j), 0, 2)], 5, device=dev)
    with pytest.raises(ValueError):
        grid.group_hits([], 2, start=np.array([0, 2], dtype=np.int32), device=dev)
    assert grid.group_hits([], 0, device=dev).shape == (0,)
    assert grid.group_hits([], 3, device=dev).tolist() == [0, 1, 2]


GRIDS = ["raw_indel_64", "raw_jaccard_16", "levels_indel_one_word", "levels_jaccard"]


def _grid_calls(g, dev):
    """(grid(thr), groups(thr, **kw)) of a probe grid through the wrappers of its mode."""
    from napkon_string_matching_amd import grid

    cap = g.pairs
    if g.raw:
        lt, rt = probe_tables.raw_indel_tables(g, dev) if g.kind == "indel" else probe_tables.raw_jaccard_tables(g, dev)
        full, groups = (grid.indel_raw_grid, grid.indel_raw_groups) if g.kind == "indel" else \
            (grid.jaccard_raw_grid, grid.jaccard_raw_groups)
        return (lambda thr: full(lt, rt, thr, capacity=cap), lambda thr, **kw: groups(lt, rt, thr, capacity=cap, **kw))
    tabs = probe_tables.levels_indel_tables(g, dev, False) if g.kind == "indel" else probe_tables.levels_jaccard_tables(g, dev, False)
    full, groups = (grid.indel_levels_grid, grid.indel_levels_groups) if g.kind == "indel" else \
        (grid.jaccard_levels_grid, grid.jaccard_levels_groups)
    return (lambda thr: full(*tabs, thr, category_mode=g.mode, capacity=cap),
            lambda thr, **kw: groups(*tabs, thr, category_mode=g.mode, capacity=cap, **kw))


@pytest.mark.parametrize("thr", [0.3, 0.6])
@pytest.mark.parametrize("name", GRIDS)
def test_table_groups_equal_the_definition_on_the_grids_hits(dev, name, thr):
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    n_l, n_r = len(g.left), len(g.right)
    assert 70 <= n_l <= 90 and n_r == tp.N_RIGHT
    full, groups = _grid_calls(g, dev)
    hits = full(thr)
    assert len(hits) > 0
    # two cohorts: left item k is node k, right item k node n_l + k
    stats = []
    got = groups(thr, stats=stats)
    want = grid.groups_of_hits([(hits, 0, n_l)], n_l + n_r, float("-inf"))
    assert got.bases == (0, n_l) and got.cohort_sizes == (n_l, n_r)
    assert np.array_equal(got.label, want)
    assert stats == [len(hits), n_l + n_r - mg.components(want)]
    assert np.array_equal(got.of(0), want[:n_l]) and np.array_equal(got.of(1), want[n_l:])
    assert len(got.members()) == int((np.bincount(want, minlength=len(want)) >= 2).sum()) > 0
    # one node space (left item k and right item k are one node): records (k, k) link nothing
    same = groups(thr, same=True)
    assert same.bases == (0,) and same.cohort_sizes == (n_r,)
    assert np.array_equal(same.label, grid.groups_of_hits([(hits, 0, 0)], n_r, float("-inf")))
    # only the records at or above a higher floor link
    floor = float(np.median(hits.score))
    assert np.array_equal(groups(thr, min_score=floor).label, grid.groups_of_hits([(hits, 0, n_l)], n_l + n_r, floor))
    if g.raw and g.kind == "indel":  # a small first buffer: the grid's retry ends in the same groups
        lt, rt = probe_tables.raw_indel_tables(g, dev)
        assert np.array_equal(grid.indel_raw_groups(lt, rt, thr, capacity=8).label, want)


def test_fuzzy_match_groups_and_clusters_with_and_without_a_wide_item(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match

    rng = random.Random(21)
    text = lambda k: " ".join("".join(rng.choice("abcde") for _ in range(rng.randint(2, 6))) for _ in range(k))
    left, right = [text(rng.randint(1, 4)) for _ in range(12)], [text(rng.randint(1, 4)) for _ in range(14)]
    right[5], right[9] = left[2], left[2]
    items = left + [left[2], left[7] + "x", right[3]]
    for wide in (False, True):
        if wide:
            left[3] = "x" * 513  # beyond the fast kernels: the general route, the merged list grouped
            items[3] = "x" * 513
            items.append("x" * 512 + "y")
        for thr in (0.4, 0.8):
            hits = fuzzy_match.raw_grid(left, right, thr, device=dev)
            got = fuzzy_match.groups(left, right, thr, device=dev)
            assert got.bases == (0, 12) and np.array_equal(got.label, grid.groups_of_hits([(hits, 0, 12)], 26, float("-inf")))
            assert got.label[12 + 5] == got.label[12 + 9] == got.label[2]
            self_hits = fuzzy_match.raw_grid(items, items, thr, device=dev)
            want = grid.MatchGroups(grid.groups_of_hits([(self_hits, 0, 0)], len(items), float("-inf")), (0,), (len(items),))
            clusters = fuzzy_match.clusters(items, thr, device=dev)
            assert [c.tolist() for c in clusters] == [m[0].tolist() for m in want.members()]
            assert any({2, 12} <= set(c.tolist()) for c in clusters) and all(len(c) >= 2 for c in clusters)
            if wide:
                assert any({3, len(items) - 1} <= set(c.tolist()) for c in clusters)
    assert fuzzy_match.clusters([], 0.5, device=dev) == []
    assert fuzzy_match.groups([], right, 0.5, device=dev).label.tolist() == list(range(14))


def test_intersection_vs_union_groups_and_clusters_with_and_without_a_wide_item(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import intersection_vs_union

    rng = random.Random(22)
    words = [f"w{q}" for q in range(10)]
    row = lambda: rng.sample(words, rng.randint(1, 4))
    left, right = [row() for _ in range(12)], [row() for _ in range(14)]
    right[5] = list(left[2])
    many = [f"x{q}" for q in range(70)]
    items = left + [list(left[2])]
    for wide in (False, True):
        if wide:
            left[4], right[6] = many[:65], many[3:68] + words[:2]  # 65 distinct tokens and more: the general route
            items[4] = many[:65]
            items.append(many[1:66])
        for thr in (0.3, 0.6):
            hits = intersection_vs_union.raw_grid(left, right, thr, device=dev)
            got = intersection_vs_union.groups(left, right, thr, device=dev)
            assert np.array_equal(got.label, grid.groups_of_hits([(hits, 0, 12)], 26, float("-inf")))
            assert got.label[12 + 5] == got.label[2]
            self_hits = intersection_vs_union.raw_grid(items, items, thr, device=dev)
            want = grid.MatchGroups(grid.groups_of_hits([(self_hits, 0, 0)], len(items), float("-inf")), (0,), (len(items),))
            clusters = intersection_vs_union.clusters(items, thr, device=dev)
            assert [c.tolist() for c in clusters] == [m[0].tolist() for m in want.members()]
            assert any({2, 12} <= set(c.tolist()) for c in clusters)
            if wide:
                assert (4, 6) in set(zip(hits.i.tolist(), hits.j.tolist())) and got.label[12 + 6] == got.label[4]
                assert any({4, len(items) - 1} <= set(c.tolist()) for c in clusters)


# ------------------------------------------------------------------------------------------------------------ Matcher
def _cohort(seed, n, words):
    rng = random.Random(seed)
    rows = []
    for k in range(n):
        toks = [rng.choice(words) for _ in range(rng.randint(1, 6))]
        term = [" ".join(toks[q:q + 2]) for q in range(0, len(toks), 2)]
        rows.append([f"{seed}-{k}", f"v{k}", "s", [f"c{k % 3}"], term, toks, "p"])
    return pd.DataFrame(rows, columns=["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"])


def test_matcher_match_groups_on_three_cohorts(dev):
    """``Matcher.match_groups`` is ``mapping_of_labels(groups_of_hits(lists_of_results(results)))``: one call over the three
    frames, entries that no single frame shows; its ids survive a second run through ``id_reference``; and ``compare``
    accepts the mapping as a whitelist."""
    from napkon_string_matching_amd import grid, groups
    from napkon_string_matching_amd.matcher import Matcher
    from napkon_string_matching_amd.types.comparable import ComparisonResults
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    words = [f"word{q}" for q in range(12)]
    cohorts = {"Pop": Questionnaire(_cohort(2, 25, words)), "hap": Questionnaire(_cohort(1, 20, words)),
               "suep": Questionnaire(_cohort(3, 22, words))}
    matching = dict(score_func="fuzzy_match", compare_column="Term", score_threshold=0.6, cached=False)
    matcher = Matcher(None, {"matching": matching}, questionnaires=cohorts)
    matcher.match_questionnaires()
    assert len(matcher.results) == 3
    names, identifiers, lists = groups.lists_of_results(matcher.results)
    assert names == ["hap", "pop", "suep"] and all(len(hits) > 0 for hits, _, _ in lists)
    nodes = sum(len(v) for v in identifiers)
    for floor in (None, 0.75):
        label = grid.groups_of_hits(lists, nodes, float("-inf") if floor is None else floor)
        want = groups.mapping_of_labels(label, names, identifiers)
        got = matcher.match_groups(min_score=floor)
        assert got.dict() == want.dict() and len(want) > 0
    everything = matcher.match_groups()
    # transitivity across frames: some entry holds a hap and a suep identifier that no hap-suep row pairs
    paired = {(a, b) for comp in matcher.results.results.values() if (comp.left_name, comp.right_name) == ("Hap", "Suep")
              for a, b in zip(comp.dataframe()["HapIdentifier"], comp.dataframe()["SuepIdentifier"])}
    assert any((a, b) not in paired for entry in everything.dict().values() for a in entry.get("hap", []) for b in entry.get("suep", []))
    # the ids of a first run are kept by the next
    again = matcher.match_groups(min_score=0.75, id_reference=everything)
    assert set(again.dict()) & set(everything.dict()) and len(again) >= len(everything) > 0
    # as a whitelist: the entries of the hap-pop frame alone name both cohorts, and their items leave the comparison
    pair_key = next(key for key, comp in matcher.results.items() if (comp.left_name, comp.right_name) == ("Hap", "Pop"))
    pair = groups.mapping_of_results(ComparisonResults({pair_key: matcher.results[pair_key]}))
    listed = {ident for entry in pair.dict().values() for ids in entry.values() for ident in ids}
    kept = cohorts["hap"].compare(cohorts["Pop"], pair, None, left_name="hap", right_name="pop", **dict(matching, score_threshold=0.2))
    frame = kept.dataframe()
    assert len(listed) > 0 and not (set(frame["HapIdentifier"]) | set(frame["PopIdentifier"])) & listed
    plain = cohorts["hap"].compare(cohorts["Pop"], None, None, left_name="hap", right_name="pop", **dict(matching, score_threshold=0.2))
    assert 0 < len(frame) < len(plain.dataframe())
