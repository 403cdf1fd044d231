"""Edge support and truss groups on the host: ``grid.support_of_hits`` / ``grid.truss_of_hits`` (the definitions that
``nsm_support_hits`` is tested against in tests/test_gpu_support.py) on hand graphs with literal values, against
``scipy.sparse`` and ``networkx``, against a numpy restatement of the device scheme; the symbol, its header and every
argument check that needs no device; and the ``min_support`` keyword where it must not reach the new entry."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from support import edge_support as es

ROOT = Path(__file__).resolve().parent.parent
BADARG = 10001


def _support(edges, nodes, **kw):
    from napkon_string_matching_amd import grid

    return grid.support_of_hits(es.one_list(edges), nodes, **kw)[0].tolist()


def _truss(edges, nodes, s):
    from napkon_string_matching_amd import grid

    words, rounds = grid.truss_of_hits(es.one_list(edges), nodes, s)
    return words[0], rounds


# ---------------------------------------------------------------------------------------------------------- hand values
@pytest.mark.parametrize("name", sorted(es.HAND))
def test_hand_graphs(name):
    edges, nodes, want = es.HAND[name]
    assert _support(edges, nodes) == want
    words, rounds = _truss(edges, nodes, 0)
    assert words.tolist() == want and rounds == 1


def test_the_literals_of_the_hand_graphs():
    assert es.HAND["triangle"][2] == [1, 1, 1] and set(es.HAND["k4"][2]) == {2} and set(es.HAND["k5"][2]) == {3}
    assert set(es.HAND["path"][2]) == {0} and set(es.HAND["k33"][2]) == {0} and set(es.HAND["bowtie"][2]) == {1}
    assert dict(zip(es.DIAMOND, es.HAND["diamond"][2])) == {(0, 1): 1, (0, 2): 1, (1, 2): 2, (1, 3): 1, (2, 3): 1}


@pytest.mark.parametrize("name,edges,nodes,s,alive,rounds", es.PEELS, ids=[p[0] for p in es.PEELS])
def test_peeling_literals(name, edges, nodes, s, alive, rounds):
    words, got_rounds = _truss(edges, nodes, s)
    assert int((words >= 0).sum()) == alive and int((words == -2).sum()) == len(edges) - alive and got_rounds == rounds
    assert (words[words >= 0] >= s).all()


def test_k5_plus_triangle_keeps_the_k5():
    words, _ = _truss(es.K5_TRIANGLE, 7, 2)
    assert words.tolist() == [3] * 10 + [-2] * 3


def test_min_support_1_never_cascades():
    from napkon_string_matching_amd import grid

    for seed in range(8):
        lists, nodes = es.seeded_lists(seed)
        for floor in (0.0, 0.6):
            assert grid.truss_of_hits(lists, nodes, 1, floor)[1] <= 2


def test_the_pinned_cascade():
    c = es.CASCADE
    assert c == dict(seed=11, nodes=24, edges=90, rounds=8, alive=12) and c["nodes"] <= 40 and c["rounds"] >= 6
    words, rounds = _truss(es.random_graph(c["seed"], c["nodes"], c["edges"]), c["nodes"], 2)
    assert rounds == 8 and int((words >= 0).sum()) == 12
    assert es.search_cascade(c["nodes"], c["edges"], c["rounds"], seeds=range(c["seed"] + 1)) == (11, 8, 12)


def test_the_fuzzy_chain():
    from napkon_string_matching_amd import grid
    from oracle import score_functions as ref

    for a in range(5):
        for b in range(5):
            assert ref.fuzzy_match(es.FUZZY_CHAIN[a], es.FUZZY_CHAIN[b]) == 1.0 - abs(a - b) / 4.0
    lists = es.fuzzy_chain_list(0.5)
    hits = lists[0][0]
    assert es.edge_counts(lists, 5, 0.5) == (14, 7)
    words = grid.support_of_hits(lists, 5, 0.5)[0]
    for i, j, w in zip(hits.i.tolist(), hits.j.tolist(), words.tolist()):
        assert w == (-1 if i == j else es.FUZZY_CHAIN_SUPPORT_AT_HALF[(min(i, j), max(i, j))])
    one, r1 = grid.truss_of_hits(lists, 5, 1, 0.5)
    two, r2 = grid.truss_of_hits(lists, 5, 2, 0.5)
    assert np.array_equal(one[0], words) and r1 == 1
    assert set(two[0].tolist()) == {-1, -2} and r2 == 3
    path = grid.support_of_hits(lists, 5, 0.75)[0]  # at 0.75 a path: the records two apart are no edge records
    assert sorted(set(path.tolist())) == [-1, 0] and int((path == 0).sum()) == 8


def test_words_of_records_that_are_no_edge_records():
    from napkon_string_matching_amd import grid

    hits = es.hits_of([(0, 1), (1, 2), (0, 2), (1, 1), (2, 0), (0, 1)], [1.0, 1.0, 1.0, 1.0, float("nan"), 0.25])
    assert grid.support_of_hits([(hits, 0, 0)], 3, 0.5)[0].tolist() == [1, 1, 1, -1, -1, -1]
    assert grid.support_of_hits([(hits, 0, 0)], 3, 0.25)[0].tolist() == [1, 1, 1, -1, -1, 1]
    assert grid.support_of_hits([], 3) == [] and grid.truss_of_hits([], 0, 3) == ([], 1)
    two_cohorts = [(es.hits_of([(a, b) for a in range(3) for b in range(4)]), 0, 3)]  # bipartite: no common neighbours
    assert set(grid.support_of_hits(two_cohorts, 7)[0].tolist()) == {0}
    assert set(grid.truss_of_hits(two_cohorts, 7, 1)[0][0].tolist()) == {-2}


# ------------------------------------------------------------------------------------------------- independent models
@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("floor", [0.0, 0.6])
def test_support_against_scipy(seed, floor):
    import scipy.sparse as sp

    from napkon_string_matching_amd import grid

    lists, nodes = es.seeded_lists(seed)
    rows, cols = [], []
    for hits, lb, rb in lists:
        keep = (hits.score >= floor) & (hits.i + lb != hits.j + rb)
        rows += (hits.i[keep] + lb).tolist() + (hits.j[keep] + rb).tolist()
        cols += (hits.j[keep] + rb).tolist() + (hits.i[keep] + lb).tolist()
    adj = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(nodes, nodes))
    adj.data[:] = 1.0  # (duplicates were summed)
    common = (adj @ adj).multiply(adj).toarray()
    got = grid.support_of_hits(lists, nodes, floor)
    for (hits, lb, rb), words in zip(lists, got):
        for s, i, j, w in zip(hits.score.tolist(), hits.i.tolist(), hits.j.tolist(), words.tolist()):
            assert w == (int(common[lb + i, rb + j]) if s >= floor and lb + i != rb + j else -1)
    assert max(int(w.max()) for w in got) >= 2


@pytest.mark.parametrize("seed", range(4))
def test_truss_against_networkx(seed):
    nx = pytest.importorskip("networkx")
    from napkon_string_matching_amd import grid

    lists, nodes = es.seeded_lists(seed)
    graph = nx.Graph()
    for hits, lb, rb in lists:
        graph.add_edges_from((lb + i, rb + j) for s, i, j in zip(hits.score.tolist(), hits.i.tolist(), hits.j.tolist())
                             if s >= 0.4 and lb + i != rb + j)
    for s in (1, 2, 3):
        truss = nx.k_truss(graph, s + 2)
        words, _rounds = grid.truss_of_hits(lists, nodes, s, 0.4)
        for (hits, lb, rb), word in zip(lists, words):
            for sc, i, j, w in zip(hits.score.tolist(), hits.i.tolist(), hits.j.tolist(), word.tolist()):
                u, v = lb + i, rb + j
                if not sc >= 0.4 or u == v:
                    assert w == -1
                elif truss.has_edge(u, v):
                    assert w == len(set(truss[u]) & set(truss[v])) >= s
                else:
                    assert w == -2


@pytest.mark.parametrize("seed", range(3))
def test_order_list_order_and_duplicates_do_not_matter(seed):
    from napkon_string_matching_amd import grid

    lists, nodes = es.seeded_lists(seed)
    rng = np.random.RandomState(seed)
    for s in (0, 2):
        want, rounds = grid.truss_of_hits(lists, nodes, s, 0.4)
        perms = [rng.permutation(len(hits)) for hits, _, _ in lists]
        shuffled = [(grid.Hits(h.score[p], h.i[p], h.j[p]), lb, rb) for (h, lb, rb), p in zip(lists, perms)]
        order = rng.permutation(len(lists)).tolist()
        got, got_rounds = grid.truss_of_hits([shuffled[k] for k in order], nodes, s, 0.4)
        assert got_rounds == rounds
        for slot, k in enumerate(order):
            assert np.array_equal(got[slot], want[k][perms[k]])
        # every record twice, and every list's records once more as a list of their own
        twice = [(grid.Hits(np.r_[h.score, h.score], np.r_[h.i, h.i], np.r_[h.j, h.j]), lb, rb) for h, lb, rb in lists]
        got, got_rounds = grid.truss_of_hits(twice + lists, nodes, s, 0.4)
        assert got_rounds == rounds
        for k, w in enumerate(want):
            assert np.array_equal(got[k], np.r_[w, w]) and np.array_equal(got[len(lists) + k], w)


@pytest.mark.parametrize("seed", range(4))
def test_the_device_scheme_restated_in_numpy(seed):
    from napkon_string_matching_amd import grid

    lists, nodes = es.seeded_lists(seed)
    for s in (0, 1, 2, 3):
        for floor in (0.0, 0.6):
            want, rounds = grid.truss_of_hits(lists, nodes, s, floor)
            got, got_rounds = es.scheme(lists, nodes, s, floor)
            assert got_rounds == rounds and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_the_scheme_on_the_cascade_and_the_seam_graph():
    from napkon_string_matching_amd import grid

    c = es.CASCADE
    lists = es.one_list(es.random_graph(c["seed"], c["nodes"], c["edges"]))
    got, rounds = es.scheme(lists, c["nodes"], 2)
    assert rounds == c["rounds"] and np.array_equal(got[0], grid.truss_of_hits(lists, c["nodes"], 2)[0][0])
    for size in (0, 1, 2, 33):
        for a, b, n_c in es.seam_cases(size):
            lists, nodes, want = es.seam_graph(a, b, n_c)
            assert np.array_equal(grid.support_of_hits(lists, nodes)[0], want), (a, b, n_c)
            assert np.array_equal(es.scheme(lists, nodes, 0)[0][0], want), (a, b, n_c)


def test_a_larger_min_support_refines_the_groups():
    from napkon_string_matching_amd import grid

    for seed in range(4):
        lists, nodes = es.seeded_lists(seed)
        labels = []
        for s in (0, 1, 2, 3):
            words, _ = grid.truss_of_hits(lists, nodes, s, 0.4)
            kept = [(grid.Hits(h.score[w >= 0], h.i[w >= 0], h.j[w >= 0]), lb, rb) for (h, lb, rb), w in zip(lists, words)]
            labels.append(grid.groups_of_hits(kept, nodes, 0.4))
        assert np.array_equal(labels[0], grid.groups_of_hits(lists, nodes, 0.4))
        for coarse, fine in zip(labels, labels[1:]):
            # every group of the finer labelling lies inside one group of the coarser one
            assert np.array_equal(coarse[fine], coarse)
            assert len(set(fine.tolist())) >= len(set(coarse.tolist()))
        assert len(set(labels[3].tolist())) > len(set(labels[0].tolist()))


# -------------------------------------------------------------------------------------------------------------- symbols
def test_symbol_header_and_binding():
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    assert _lib.SUPPORT_EXPORTS == ("nsm_support_hits",)
    others = (_lib.EXPORTS + _lib.ASSIGN_EXPORTS + _lib.GROUP_EXPORTS + _lib.SPAN_EXPORTS + _lib.MEASURE_EXPORTS + _lib.EDIT_EXPORTS)
    assert not set(_lib.SUPPORT_EXPORTS) & set(others)
    fn = _lib.entry("nsm_support_hits")
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    assert lib.nsm_abi_version() == 5 == _lib.ABI_VERSION
    declared = lambda path: set(re.findall(r"^\s*(?:int|uint64_t|const char\*)\s+(nsm_\w+)\s*\(", path.read_text(), flags=re.M))
    assert declared(ROOT / "include" / "nsm_hip_support.h") == set(_lib.SUPPORT_EXPORTS)
    assert declared(ROOT / "include" / "nsm_hip.h") == set(_lib.EXPORTS)
    text = (ROOT / "include" / "nsm_hip_support.h").read_text()
    assert '#include "nsm_hip_groups.h"' in text and "NSM_ABI_VERSION" in text and "#define NSM_ABI_VERSION" not in text
    assert es.routing_constants() == {"NSM_SUPPORT_WAVE_MIN": 32}


def test_argument_checks_that_need_no_device():
    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_support_hits")
    error = lambda: _lib.load().nsm_last_error().decode()
    one = (_lib.NsmHitList * 1)()
    out = (ctypes.c_void_p * 1)(0x1000)  # (never dereferenced: every case ends before the first HIP call)
    none = (ctypes.c_void_p * 1)(None)
    hits = 0x2000

    def with_list(**fields):
        one[0] = _lib.NsmHitList(None, 0, 0, 2, 2, 2)
        for key, value in fields.items():
            setattr(one[0], key, value)
        return one

    assert fn(None, 1, 4, 0.0, 0, out, None, None) == BADARG and "null lists" in error()
    assert fn(with_list(), 1, 4, 0.0, 0, None, None, None) == BADARG and "null support" in error()
    assert fn(with_list(), -1, 4, 0.0, 0, out, None, None) == BADARG and "negative count" in error()
    assert fn(with_list(), 1, -4, 0.0, 0, out, None, None) == BADARG and "negative count" in error()
    assert fn(with_list(), 1, 4, 0.0, -1, out, None, None) == BADARG and "negative count" in error()
    assert fn(with_list(n=3), 1, 4, 0.0, 0, out, None, None) == BADARG and "null hits" in error()
    assert fn(with_list(n=3, hits=hits), 1, 4, 0.0, 0, none, None, None) == BADARG and "list 0 has null support" in error()
    for field in ("left_base", "left_ids", "right_base", "right_ids"):
        assert fn(with_list(**{field: -1}), 1, 4, 0.0, 0, out, None, None) == BADARG and "negative base or id count" in error()
    assert fn(with_list(left_ids=5), 1, 4, 0.0, 0, out, None, None) == BADARG and "beyond" in error()
    assert fn(with_list(right_base=3), 1, 4, 0.0, 0, out, None, None) == BADARG and "beyond" in error()
    assert fn(with_list(left_base=0x7FFFFFFF, left_ids=0x7FFFFFFF), 1, 4, 0.0, 0, out, None, None) == BADARG and "beyond" in error()
    # the documented order: an earlier check wins
    assert fn(None, 1, -1, 0.0, -1, None, None, None) == BADARG and "null lists" in error()
    assert fn(with_list(n=3), 1, -1, 0.0, 0, None, None, None) == BADARG and "null support" in error()
    assert fn(with_list(n=3), 1, -1, 0.0, 0, out, None, None) == BADARG and "negative count" in error()
    assert fn(with_list(n=3, left_base=-1), 1, 4, 0.0, 0, out, None, None) == BADARG and "null hits" in error()
    assert fn(with_list(n=3, hits=hits, left_base=-1), 1, 4, 0.0, 0, none, None, None) == BADARG and "null support" in error()
    assert fn(with_list(left_base=-1, right_ids=1000), 1, 4, 0.0, 0, out, None, None) == BADARG and "negative base" in error()
    # nodes == 0, no lists, no records at all: nothing to do, no launch
    assert fn(None, 0, 0, 0.0, 0, None, None, None) == 0
    assert fn(None, 0, 4, 0.0, 3, None, None, None) == 0
    assert fn(with_list(), 1, 4, 0.0, 1, none, None, None) == 0
    assert fn(with_list(left_ids=0, right_base=0, right_ids=0), 1, 0, 0.0, 1, none, None, None) == 0


# -------------------------------------------------------------------------------------------------------- the keyword
@pytest.mark.parametrize("value", [-1, 1.5, "1", None, True])
def test_a_bad_min_support_is_a_value_error_before_any_device_work(value, monkeypatch):
    from napkon_string_matching_amd import _lib, grid, groups
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union
    from napkon_string_matching_amd.matcher import Matcher
    from napkon_string_matching_amd.types.comparable import ComparisonResults

    def no_device(*_args, **_kw):
        raise AssertionError("device work before the check")

    monkeypatch.setattr(grid, "_require_gpu", no_device)
    monkeypatch.setattr(_lib, "entry", no_device)
    for name in ("indel_raw_grid", "jaccard_raw_grid", "indel_levels_grid", "jaccard_levels_grid"):
        monkeypatch.setattr(grid, name, no_device)
    lists = es.one_list(es.DIAMOND)
    with pytest.raises(ValueError, match="min_support"):
        grid.check_min_support(value)
    with pytest.raises(ValueError, match="min_support"):
        grid.truss_of_hits(lists, 4, value)
    with pytest.raises(ValueError, match="min_support"):
        grid.support_hits(lists, 4, min_support=value)
    with pytest.raises(ValueError, match="min_support"):
        grid.support_lists_device([], 4, 0.0, value, None)
    with pytest.raises(ValueError, match="min_support"):
        grid.group_hits(lists, 4, min_support=value)
    for wrapper, args in ((grid.indel_raw_groups, 2), (grid.jaccard_raw_groups, 2), (grid.indel_levels_groups, 4),
                          (grid.jaccard_levels_groups, 2)):
        with pytest.raises(ValueError, match="min_support"):
            wrapper(*([None] * args), 0.5, min_support=value)
    for plugin in (fuzzy_match, intersection_vs_union):
        with pytest.raises(ValueError, match="min_support"):
            plugin.groups(["a b"], ["a b"], 0.5, device="cuda:0", min_support=value)
        with pytest.raises(ValueError, match="min_support"):
            plugin.clusters(["a b", "a c"], 0.5, device="cuda:0", min_support=value)
    with pytest.raises(ValueError, match="min_support"):
        groups.mapping_of_results(ComparisonResults({}), min_support=value)
    matcher = Matcher.__new__(Matcher)
    matcher.results = ComparisonResults({})
    with pytest.raises(ValueError, match="min_support"):
        matcher.match_groups(min_support=value)


def test_good_values_of_min_support():
    from napkon_string_matching_amd import grid

    assert [grid.check_min_support(v) for v in (0, 1, 7, np.int32(2), np.int64(3))] == [0, 1, 7, 2, 3]


def test_min_support_0_never_asks_for_the_new_symbol(monkeypatch):
    """The default everywhere: what ``group_hits`` and ``_groups_pending`` hand ``group_lists_device`` is what they handed
    it before the keyword existed, and ``_lib.entry`` is never asked for ``nsm_support_hits``."""
    from napkon_string_matching_amd import _lib, grid

    asked = []

    def entry(name):
        asked.append(name)
        if name == "nsm_support_hits":
            raise AssertionError("min_support = 0 looked the new entry up")
        raise _lib.NsmLibraryError("stop here")  # (no device on this machine: the call ends where the old one would start)

    class FakeDevice:
        type, index = "cuda", 0

    monkeypatch.setattr(_lib, "entry", entry)
    monkeypatch.setattr(grid, "_require_gpu", lambda device: FakeDevice())
    monkeypatch.setattr(grid, "_records_to_device", lambda hits, dev: None)
    lists = es.one_list(es.DIAMOND)
    for kw in ({}, {"min_support": 0}, {"min_support": np.int64(0)}):
        with pytest.raises(_lib.NsmLibraryError, match="stop here"):
            grid.group_hits(lists, 4, **kw)

    class Pending:
        n = 0

        class buf:
            class records:
                device = None

                @staticmethod
                def data_ptr():
                    return 0

    class Table:
        orig, n = None, 3

    monkeypatch.setattr(grid, "_id_count", lambda orig, n, what: n)
    for kw in ({}, {"min_support": 0}):
        with pytest.raises(_lib.NsmLibraryError, match="stop here"):
            grid._groups_pending(Pending, Table, Table, True, None, None, **kw)
    assert asked == ["nsm_group_hits"] * 5
    with pytest.raises(AssertionError, match="looked the new entry up"):
        grid._groups_pending(Pending, Table, Table, True, None, None, min_support=1)
