"""Edge support and truss groups on the GPU (``nsm_support_hits``, csrc/support.hip) against the definitions
``grid.support_of_hits`` / ``grid.truss_of_hits`` (tests/test_cpu_support.py checks those against literals, scipy, networkx
and a restatement of the device scheme), word for word.

The C entry is called through ctypes with ``support`` arrays of exactly the documented sizes, poisoned and with guard words
behind them; ``stats`` must equal the model: edge records, distinct edges, distinct edges alive at the end, rounds, and the
sum of the final supports over the alive distinct edges (three times the triangles of the final graph).  The Python layers
with ``min_support`` are compared with ``groups_of_hits`` of the records whose ``truss_of_hits`` word is ``>= 0``."""
import numpy as np
import pandas as pd
import pytest

from support import edge_support as es
from support import probe_tables
from support import threshold_probes as tp

pytestmark = pytest.mark.gpu
BADARG, UNSUPPORTED = 10001, 10002
POISON = -77


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _records(hits):
    host = np.empty((len(hits), 2), dtype=np.float64)
    host[:, 0] = hits.score
    ij = host.view(np.int32).reshape(len(hits), 4)
    ij[:, 2], ij[:, 3] = hits.i, hits.j
    return host


def _entry(dev, lists, nodes, min_score=0.0, min_support=0, stats0=(0, 0, 0, 0, 0), with_stats=True, ids=None):
    """``nsm_support_hits``: (status, the words per list, stats).  Every ``support[l]`` starts as poison and has 4 guard
    words behind it; the records must be byte-identical afterwards.  ``ids``: per list (left_ids, right_ids), by default up
    to the end of the node space."""
    import ctypes

    import torch

    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_support_hits")
    descs = (_lib.NsmHitList * max(1, len(lists)))()
    out = (ctypes.c_void_p * max(1, len(lists)))()
    recs, words = [], []
    for k, (slot, (hits, lb, rb)) in enumerate(zip(descs, lists)):
        n = len(hits)
        recs.append(torch.from_numpy(_records(hits)).to(dev) if n else None)
        words.append(torch.full((n + 4,), POISON, dtype=torch.int32, device=dev))
        slot.hits, slot.n = (recs[-1].data_ptr() if n else None), n
        slot.left_base, slot.right_base = lb, rb
        slot.left_ids, slot.right_ids = (nodes - lb, nodes - rb) if ids is None else ids[k]
        out[k] = words[-1].data_ptr() if n else None
    st = torch.tensor(list(stats0), dtype=torch.int64, device=dev)
    rc = fn(descs, len(lists), nodes, float(min_score), min_support, out, st.data_ptr() if with_stats else None,
            torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = []
    for (hits, _lb, _rb), rec, word in zip(lists, recs, words):
        if rec is not None:
            assert np.array_equal(rec.cpu().numpy().view(np.int64), _records(hits).view(np.int64)), "the input was written"
        host = word.cpu().numpy()
        assert (host[len(hits):] == POISON).all(), "wrote beyond the records"
        got.append(host[:len(hits)])
    return rc, got, [int(v) for v in st.tolist()]


def _model_stats(lists, nodes, min_score, want, rounds):
    records, distinct = es.edge_counts(lists, nodes, min_score)
    tri, alive = es.final_triangles_x3(lists, nodes, want)
    return [records, distinct, alive, rounds, tri]


def _check_entry(dev, lists, nodes, min_score, min_support):
    from napkon_string_matching_amd import grid

    want, rounds = grid.truss_of_hits(lists, nodes, min_support, min_score)
    rc, got, stats = _entry(dev, lists, nodes, min_score, min_support)
    assert rc == 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"list {k}: first difference at record {int(np.flatnonzero(g != w)[0])}"
    assert stats == _model_stats(lists, nodes, min_score, want, rounds)
    return want, rounds, stats


# ---------------------------------------------------------------------------------------------------------- definitions
@pytest.mark.parametrize("name", sorted(es.HAND))
def test_hand_graphs(dev, name):
    from napkon_string_matching_amd import grid

    edges, nodes, want = es.HAND[name]
    stats = []
    got = grid.support_hits(es.one_list(edges), nodes, device=dev, stats=stats)
    assert got[0].dtype == np.int32 and got[0].tolist() == want
    assert stats == [len(edges), len(edges), len(edges), 1, sum(want)]
    _check_entry(dev, es.one_list(edges), nodes, 0.0, 0)


@pytest.mark.parametrize("seed", range(3))
def test_seeded_lists_equal_the_definition(dev, seed):
    from napkon_string_matching_amd import grid

    lists, nodes = es.seeded_lists(seed)
    assert len(lists) == 4 and any(np.isnan(h.score).any() for h, _, _ in lists)
    for floor in (0.0, 0.6, float(np.nextafter(0.6, 0.0)), float(np.nextafter(0.6, 1.0)), float("-inf")):
        for s in (0, 1, 2):
            want, _rounds, stats = _check_entry(dev, lists, nodes, floor, s)
        assert stats[0] > stats[1] > 0
    # 0.6 is a score: the floor just above it drops records the floor on it keeps
    on, above = grid.support_of_hits(lists, nodes, 0.6), grid.support_of_hits(lists, nodes, float(np.nextafter(0.6, 1.0)))
    below = grid.support_of_hits(lists, nodes, float(np.nextafter(0.6, 0.0)))
    assert all(np.array_equal(a, b) for a, b in zip(on, below)) and any((a >= 0).sum() > (b >= 0).sum() for a, b in zip(on, above))
    # the Python layer: one call, the words of every list
    got = grid.support_hits(lists, nodes, 0.4, 2, device=dev)
    assert all(np.array_equal(a, b) for a, b in zip(got, grid.truss_of_hits(lists, nodes, 2, 0.4)[0]))


def test_stats_are_added_to_and_may_be_null(dev):
    lists, nodes = es.seeded_lists(1)
    want, rounds, stats = _check_entry(dev, lists, nodes, 0.4, 2)
    rc, got, added = _entry(dev, lists, nodes, 0.4, 2, stats0=(100, 200, 300, 400, 500))
    assert rc == 0 and added == [a + b for a, b in zip((100, 200, 300, 400, 500), stats)]
    rc, got, kept = _entry(dev, lists, nodes, 0.4, 2, stats0=(5, 6, 7, 8, 9), with_stats=False)
    assert rc == 0 and kept == [5, 6, 7, 8, 9] and all(np.array_equal(a, b) for a, b in zip(got, want))


# ----------------------------------------------------------------------------------------------------------- seam graph
@pytest.mark.parametrize("size", es.seam_sizes())
def test_seam_graph(dev, size):
    """|A|, |B| and |C| around every routing seam: the shorter row of (u, v) below, at and above NSM_SUPPORT_WAVE_MIN, and
    around the wavefront's 64 and 128; C holds node 0 and the last node."""
    from napkon_string_matching_amd import grid

    assert {31, 32, 33} <= set(es.seam_sizes()) and es.routing_constants() == {"NSM_SUPPORT_WAVE_MIN": 32}
    for a, b, c in es.seam_cases(size):
        lists, nodes, want = es.seam_graph(a, b, c)
        got = grid.support_hits(lists, nodes, device=dev)[0]
        assert np.array_equal(got, want), (a, b, c, int(np.flatnonzero(got != want)[0]))
        # ... and peeled at 1: (u, v) and the edges into C stay, the edges into A and B go
        peeled = grid.support_hits(lists, nodes, min_support=1, device=dev)[0]
        assert np.array_equal(peeled, np.where(want == 0, -2, want) if c else np.full(len(want), -2)), (a, b, c)


@pytest.mark.parametrize("a,b,c", [(3000, 5, 70), (5, 3000, 70), (3000, 3000, 3000), (0, 0, 3000)])
def test_seam_graph_with_a_hub(dev, a, b, c):
    lists, nodes, want = es.seam_graph(a, b, c)
    rc, got, stats = _entry(dev, lists, nodes)
    assert rc == 0 and np.array_equal(got[0], want)
    assert stats == [len(want), a + b + 2 * c + 1, a + b + 2 * c + 1, 1, 3 * c]
    rc, got, stats = _entry(dev, lists, nodes, min_support=2)
    assert rc == 0 and (got[0] == -2).all()
    # the edges into A, B and C go in round 1, (u, v) in round 2, round 3 removes nothing
    assert stats == [len(want), a + b + 2 * c + 1, 0, 3, 0]


# ----------------------------------------------------------------------------------------------------- degenerate inputs
def test_degenerate_inputs(dev):
    from napkon_string_matching_amd import grid

    tri = es.HAND["triangle"][0]
    # no edge at all: every record is below min_score, a self-loop or a NaN
    low = [(es.hits_of(tri + [(1, 1)], [0.1, 0.2, float("nan"), 1.0]), 0, 0)]
    rc, got, stats = _entry(dev, low, 3, 0.5, 1)
    assert rc == 0 and got[0].tolist() == [-1] * 4 and stats == [0, 0, 0, 1, 0]
    # exactly one edge (once, and as five records in both orientations)
    for edges in ([(2, 0)], [(2, 0), (0, 2), (2, 0), (0, 2), (0, 2)]):
        rc, got, stats = _entry(dev, es.one_list(edges), 3)
        assert rc == 0 and got[0].tolist() == [0] * len(edges) and stats == [len(edges), 1, 1, 1, 0]
        rc, got, stats = _entry(dev, es.one_list(edges), 3, min_support=1)
        assert rc == 0 and got[0].tolist() == [-2] * len(edges) and stats == [len(edges), 1, 0, 2, 0]
    # no lists, and lists without a record: nothing is launched, nothing is written
    assert _entry(dev, [], 5, stats0=(1, 2, 3, 4, 5)) == (0, [], [1, 2, 3, 4, 5])
    rc, got, stats = _entry(dev, [(es.hits_of([]), 0, 0), (es.hits_of([]), 2, 1)], 5, stats0=(1, 2, 3, 4, 5))
    assert rc == 0 and [len(g) for g in got] == [0, 0] and stats == [1, 2, 3, 4, 5]
    assert grid.support_hits([], 5, device=dev) == [] and grid.support_hits([], 0, min_support=2, device=dev) == []
    # empty lists among full ones
    lists, nodes = es.seeded_lists(2)
    mixed = [(es.hits_of([]), 0, 0), lists[0], (es.hits_of([]), 3, 3), lists[3], lists[1], (es.hits_of([]), 0, 1)]
    _check_entry(dev, mixed, nodes, 0.4, 2)
    # one node: every record is a self-loop
    rc, got, stats = _entry(dev, es.one_list([(0, 0), (0, 0)]), 1, min_support=1)
    assert rc == 0 and got[0].tolist() == [-1, -1] and stats == [0, 0, 0, 1, 0]


@pytest.mark.parametrize("ranges", ["equal", "overlapping", "disjoint"])
def test_node_ranges(dev, ranges):
    """One list whose two sides are the same nodes, overlap by half, or are two cohorts (a bipartite graph: support 0)."""
    rng = np.random.RandomState(5)
    n = 40
    left_base, right_base, nodes = {"equal": (0, 0, n), "overlapping": (0, n // 2, n + n // 2), "disjoint": (0, n, 2 * n)}[ranges]
    edges = rng.randint(0, n, (500, 2))
    lists = [(es.hits_of(edges, rng.choice(es.SCORES, len(edges))), left_base, right_base)]
    ids = [(n, n)]
    for s in (0, 1, 2):
        want, _rounds, stats = _check_entry(dev, lists, nodes, 0.4, s)
        rc, got, _ = _entry(dev, lists, nodes, 0.4, s, ids=ids)  # the id counts as a grid passes them
        assert rc == 0 and np.array_equal(got[0], want[0])
        if ranges == "disjoint":
            assert set(want[0].tolist()) <= ({-1, 0} if s == 0 else {-1, -2}) and stats[4] == 0
        else:
            assert stats[2] > 0 and stats[4] > 0


# -------------------------------------------------------------------------------------------------------------- peeling
@pytest.mark.parametrize("name,edges,nodes,s,alive,rounds", es.PEELS, ids=[p[0] for p in es.PEELS])
def test_peeling(dev, name, edges, nodes, s, alive, rounds):
    want, got_rounds, stats = _check_entry(dev, es.one_list(edges), nodes, 0.0, s)
    assert got_rounds == rounds and stats[:4] == [len(edges), len(edges), alive, rounds]
    assert stats[4] == es.final_triangles_x3(es.one_list(edges), nodes, want)[0]


def test_the_pinned_cascade(dev):
    c = es.CASCADE
    edges = es.random_graph(c["seed"], c["nodes"], c["edges"])
    rng = np.random.RandomState(1)
    both = edges + [(b, a) for a, b in edges] + [edges[k] for k in rng.randint(0, len(edges), 30)]  # a self-join, duplicates
    both = [both[k] for k in rng.permutation(len(both))]
    want, rounds, stats = _check_entry(dev, es.one_list(both), c["nodes"], 0.0, 2)
    assert rounds == 8 and stats[:4] == [len(both), 90, 12, 8] and stats[4] % 3 == 0 and stats[4] >= 2 * 12


# ------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("min_support", [0, 2])
@pytest.mark.parametrize("which,where,field,value", [
    (0, "first", "i", "left_ids"), (1, "last", "j", "right_ids"), (2, "first", "i", -1), (3, "middle", "j", -5),
    (1, "middle", "i", 2 ** 31 - 1)])
def test_an_id_out_of_range_is_refused_before_anything_is_written(dev, min_support, which, where, field, value):
    from napkon_string_matching_amd import _lib, grid

    lists, nodes = es.seeded_lists(0)
    hits, lb, rb = lists[which]
    r = {"first": 0, "last": len(hits) - 1, "middle": len(hits) // 2}[where]
    i, j, score = hits.i.copy(), hits.j.copy(), hits.score.copy()
    (i if field == "i" else j)[r] = {"left_ids": nodes - lb, "right_ids": nodes - rb}.get(value, value)
    score[r] = -1.0  # below min_score: ALL records are checked, whatever their score
    lists[which] = (grid.Hits(score, i, j), lb, rb)
    rc, got, stats = _entry(dev, lists, nodes, 0.4, min_support, stats0=(21, 22, 23, 24, 25))
    assert rc == BADARG and "outside" in _lib.load().nsm_last_error().decode()
    assert stats == [21, 22, 23, 24, 25] and all((g == POISON).all() for g in got)


def test_a_capturing_stream_is_refused_before_any_launch(dev):
    import ctypes

    import torch

    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_support_hits")
    hits = es.hits_of(es.DIAMOND)
    recs = torch.from_numpy(_records(hits)).to(dev)
    descs = (_lib.NsmHitList * 1)(_lib.NsmHitList(recs.data_ptr(), len(hits), 0, 4, 0, 4))
    words = torch.full((len(hits),), POISON, dtype=torch.int32, device=dev)
    out = (ctypes.c_void_p * 1)(words.data_ptr())
    st = torch.tensor([11, 12, 13, 14, 15], dtype=torch.int64, device=dev)
    other = torch.zeros(8, device=dev)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            other.add_(1.0)  # (a graph of one node: the refused call adds none)
            rc = fn(descs, 1, 4, 0.0, 1, out, st.data_ptr(), stream.cuda_stream)
        graph.replay()
    torch.cuda.synchronize(dev)
    assert rc == UNSUPPORTED and "captured" in _lib.load().nsm_last_error().decode()
    assert (words == POISON).all() and st.tolist() == [11, 12, 13, 14, 15] and other.tolist() == [1.0] * 8


# -------------------------------------------------------------------------------------------------------- Python layers
def _truss_labels(lists, nodes, min_score, min_support):
    """The meaning of ``min_support``: ``groups_of_hits`` over the records whose ``truss_of_hits`` word is ``>= 0``."""
    from napkon_string_matching_amd import grid

    words, _ = grid.truss_of_hits(lists, nodes, min_support, min_score)
    kept = [(grid.Hits(h.score[w >= 0], h.i[w >= 0], h.j[w >= 0]), lb, rb) for (h, lb, rb), w in zip(lists, words)]
    return grid.groups_of_hits(kept, nodes, min_score), sum(int((w == -2).sum()) for w in words)


@pytest.mark.parametrize("seed", range(2))
def test_group_hits_with_min_support_on_host_lists(dev, seed):
    from napkon_string_matching_amd import grid

    lists, nodes = es.seeded_lists(seed)
    labels = []
    for s in (0, 1, 2, 3):
        want, removed = _truss_labels(lists, nodes, 0.4, s)
        got = grid.group_hits(lists, nodes, 0.4, device=dev, min_support=s)
        assert got.dtype == np.int32 and np.array_equal(got, want) and (removed > 0) == (s > 0)
        labels.append(got)
    assert np.array_equal(labels[0], grid.group_hits(lists, nodes, 0.4, device=dev))
    for coarse, fine in zip(labels, labels[1:]):  # a larger min_support refines the groups
        assert np.array_equal(coarse[fine], coarse)
    assert len(set(labels[3].tolist())) > len(set(labels[0].tolist()))
    # linked into a forest: the truss is taken of the lists, the labels go on from `start`
    start = np.arange(nodes, dtype=np.int32)
    start[[3, 4]] = [1, 3]
    got = grid.group_hits(lists, nodes, 0.4, start=start, device=dev, min_support=2)
    words, _ = grid.truss_of_hits(lists, nodes, 2, 0.4)
    kept = [(grid.Hits(h.score[w >= 0], h.i[w >= 0], h.j[w >= 0]), lb, rb) for (h, lb, rb), w in zip(lists, words)]
    assert np.array_equal(got, grid.groups_of_hits(kept, nodes, 0.4, start=start))
    # everything removed, and no list at all
    assert grid.group_hits(es.one_list(es.DIAMOND), 4, device=dev, min_support=2).tolist() == [0, 1, 2, 3]
    assert grid.group_hits([], 3, device=dev, min_support=1).tolist() == [0, 1, 2]


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


@pytest.mark.parametrize("name", GRIDS)
def test_table_groups_with_min_support_on_the_grids_hits(dev, name):
    """The four ``*_groups`` wrappers in one node space (left item k and right item k are one node): the grid's hits stay
    on the device, the truss is taken there, and the labels equal the definition on the hits the grid returns."""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    n_l, n_r = len(g.left), len(g.right)
    full, groups = _grid_calls(g, dev)
    thr = 0.3
    hits = full(thr)
    assert len(hits) > 0
    plain = groups(thr, same=True)
    assert np.array_equal(plain.label, grid.groups_of_hits([(hits, 0, 0)], n_r, float("-inf")))
    seen = []
    for s in (1, 2):
        for floor in (None, float(np.median(hits.score))):
            want, removed = _truss_labels([(hits, 0, 0)], n_r, float("-inf") if floor is None else floor, s)
            stats = []
            got = groups(thr, same=True, min_support=s, min_score=floor, stats=stats)
            assert got.bases == (0,) and got.cohort_sizes == (n_r,)
            assert np.array_equal(got.label, want), (name, s, floor)
            assert np.array_equal(plain.label[got.label], plain.label)  # a refinement of the plain groups
            seen.append((removed, len(got.members())))
    assert any(removed > 0 for removed, _ in seen), seen
    # two cohorts are a bipartite graph: every support is 0 and every group dissolves
    assert groups(thr, min_support=1).label.tolist() == list(range(n_l + n_r))


def test_clusters_on_the_fuzzy_chain(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match

    chain = es.FUZZY_CHAIN
    hits = fuzzy_match.raw_grid(chain, chain, 0.5, device=dev)
    assert sorted(zip(hits.score.tolist(), hits.i.tolist(), hits.j.tolist())) == sorted(
        (1.0 - abs(a - b) / 4.0, a, b) for a in range(5) for b in range(5) if abs(a - b) <= 2)
    words = grid.support_hits([(hits, 0, 0)], 5, 0.5, device=dev)[0]
    for i, j, w in zip(hits.i.tolist(), hits.j.tolist(), words.tolist()):
        assert w == (-1 if i == j else es.FUZZY_CHAIN_SUPPORT_AT_HALF[(min(i, j), max(i, j))])
    as_lists = lambda clusters: [c.tolist() for c in clusters]
    assert as_lists(fuzzy_match.clusters(chain, 0.75, device=dev)) == [[0, 1, 2, 3, 4]]
    assert as_lists(fuzzy_match.clusters(chain, 0.75, device=dev, min_support=0)) == [[0, 1, 2, 3, 4]]
    assert as_lists(fuzzy_match.clusters(chain, 0.75, device=dev, min_support=1)) == []
    assert as_lists(fuzzy_match.clusters(chain, 0.5, device=dev, min_support=1)) == [[0, 1, 2, 3, 4]]
    assert as_lists(fuzzy_match.clusters(chain, 0.5, device=dev, min_support=2)) == []
    # ... and through groups(): two separate lists are bipartite
    assert fuzzy_match.groups(chain, chain, 0.5, device=dev, same=True, min_support=1).label.tolist() == [0] * 5
    assert fuzzy_match.groups(chain, chain, 0.5, device=dev, min_support=1).label.tolist() == list(range(10))


def test_clusters_of_token_sets_and_the_wide_item_route(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    # a triangle of near-duplicates, a chain hanging on it, and a pair
    sets = [["a", "b", "c", "d"], ["a", "b", "c", "e"], ["a", "b", "c", "f"], ["a", "f", "g", "h"], ["g", "h", "i", "j"],
            ["x", "y"], ["x", "y", "z"]]
    hits = intersection_vs_union.raw_grid(sets, sets, 0.3, device=dev)
    want, removed = _truss_labels([(hits, 0, 0)], len(sets), float("-inf"), 1)
    got = intersection_vs_union.groups(sets, sets, 0.3, device=dev, same=True, min_support=1)
    assert np.array_equal(got.label, want) and removed > 0
    assert [c.tolist() for c in intersection_vs_union.clusters(sets, 0.3, device=dev)] == [[0, 1, 2, 3, 4], [5, 6]]
    assert [c.tolist() for c in intersection_vs_union.clusters(sets, 0.3, device=dev, min_support=1)] == [[0, 1, 2]]
    # a string beyond the fast kernels sends the grid through the general route and the merged host list through group_hits
    chain = es.FUZZY_CHAIN + ["x" * 513, "x" * 512 + "y"]
    assert [c.tolist() for c in fuzzy_match.clusters(chain, 0.5, device=dev)] == [[0, 1, 2, 3, 4], [5, 6]]
    assert [c.tolist() for c in fuzzy_match.clusters(chain, 0.5, device=dev, min_support=1)] == [[0, 1, 2, 3, 4]]
    assert [c.tolist() for c in fuzzy_match.clusters(chain, 0.5, device=dev, min_support=2)] == []


# -------------------------------------------------------------------------------------------------------------- Matcher
def _cohort(tag, terms):
    rows = [[f"{tag}-{name}", f"v{k}", "s", ["c0"], [text], text.split(), "p"] for k, (name, text) in enumerate(terms)]
    return pd.DataFrame(rows, columns=["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"])


def test_matcher_match_groups_with_min_support(dev):
    """Three cohorts whose frames hold a consistent triple (hap ~ pop ~ suep, pairwise) and a chain a-b, b-c without a-c:
    under ``min_support=1`` the triple stays one entry and the chain dissolves; without the keyword the mapping is
    today's."""
    from napkon_string_matching_amd import grid, groups
    from napkon_string_matching_amd.matcher import Matcher
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    cohorts = {
        "hap": Questionnaire(_cohort("h", [("triple", "blood pressure systolic"), ("chain", "aaaa"), ("lone", "qqqq rrrr")])),
        "Pop": Questionnaire(_cohort("p", [("triple", "blood pressure systolic"), ("chain", "aabb"), ("lone", "ssss tttt")])),
        "suep": Questionnaire(_cohort("s", [("triple", "blood pressure systolic"), ("chain", "bbbb"), ("lone", "uuuu vvvv")])),
    }
    # (compare_terms weighs a single level with 1/2: the triple scores 0.5, the chain's neighbours 0.25, its ends 0)
    matching = dict(score_func="fuzzy_match", compare_column="Term", score_threshold=0.25, cached=False)
    matcher = Matcher(None, {"matching": matching}, questionnaires=cohorts)
    matcher.match_questionnaires()
    assert len(matcher.results) == 3
    names, identifiers, lists = groups.lists_of_results(matcher.results)
    nodes = sum(len(v) for v in identifiers)
    rows = {(a, b) for comp in matcher.results.results.values()
            for a, b in zip(comp.dataframe()[comp.left_name + "Identifier"], comp.dataframe()[comp.right_name + "Identifier"])}
    assert rows == {("h-triple", "p-triple"), ("p-triple", "s-triple"), ("h-triple", "s-triple"), ("h-chain", "p-chain"),
                    ("p-chain", "s-chain")}
    today = groups.mapping_of_labels(grid.groups_of_hits(lists, nodes, float("-inf")), names, identifiers)
    triple = {"hap": ["h-triple"], "pop": ["p-triple"], "suep": ["s-triple"]}
    chain = {"hap": ["h-chain"], "pop": ["p-chain"], "suep": ["s-chain"]}
    assert matcher.match_groups().dict() == today.dict() and sorted(today.dict().values(), key=str) == sorted([triple, chain], key=str)
    assert matcher.match_groups(min_support=0).dict() == today.dict()
    strict = matcher.match_groups(min_support=1)
    assert list(strict.dict().values()) == [triple]
    assert set(strict.dict()) <= set(today.dict())  # the entry keeps its id: its smallest node is the same
    assert matcher.match_groups(min_support=2).dict() == {}
    assert groups.mapping_of_results(matcher.results, min_support=1, device=dev).dict() == strict.dict()
