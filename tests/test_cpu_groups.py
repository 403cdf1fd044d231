"""Match groups without a GPU: ``grid.groups_of_hits`` (the definition, a union-find) against the breadth-first reference
of tests/support/match_groups.py on every family, the consequences of the definition (labels are component minima; the
order of records and lists does not matter; a higher ``min_score`` only refines the partition; hooks = components before
minus components after), ``groups.mapping_of_labels`` / ``lists_of_results``, and the symbols the new header declares.

Entry errors: every case ends in host code before the entry's first HIP call -- read off csrc/groups.hip: the argument
checks and the ``nodes == 0`` return precede ``hipStreamIsCapturing``, the first HIP call."""
import ctypes
import hashlib
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from support import match_groups as mg

ROOT = Path(__file__).resolve().parent.parent
BADARG = 10001


# ------------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("name", mg.NAMES)
def test_definition_equals_the_search(name):
    from napkon_string_matching_amd import grid

    c, want = mg.case(name), mg.answer(name)
    got = grid.groups_of_hits(c.entries(), c.nodes, c.min_score)
    assert got.dtype == np.int32 and got.shape == (c.nodes,)
    assert np.array_equal(got, want), name
    # labels are component minima: a label labels itself, no node lies below its label, untouched nodes are their own
    assert np.array_equal(got[got], got) and (got <= np.arange(c.nodes)).all()
    touched = np.zeros(c.nodes, dtype=bool)
    for l in c.lists:
        keep = l.score >= c.min_score
        touched[l.left_base + l.i[keep]] = True
        touched[l.right_base + l.j[keep]] = True
    assert np.array_equal(got[~touched], np.arange(c.nodes)[~touched])


def test_the_families_hold_what_they_claim():
    assert len(set(mg.NAMES)) == len(mg.NAMES) and set(mg.FAMILIES) <= set(mg.NAMES)
    for order in ("ascending", "descending", "shuffled"):
        assert (mg.answer(f"path_{order}") == 0).all() and mg.case(f"path_{order}").nodes == 5000
    assert (mg.answer("star_hub_largest") == 0).all() and (mg.answer("star_hub_smallest") == 0).all()
    assert (mg.answer("bipartite_300x300") == 0).all() and mg.case("bipartite_300x300").records() == 90000
    pairs = mg.answer("pairs_1025")
    assert mg.components(pairs) == 2200 - 1025 and np.bincount(pairs).max() == 2
    loops = mg.answer("self_loops")
    assert mg.components(loops) == 200 - 3 and loops[6] == 5 and loops[150] == loops[151] == 17
    three = mg.answer("three_cohorts")
    # a3 ~ b7 (AB), b7 ~ c5 (BC): node 3, node 47, node 95 -- and no list holds (a3, c5)
    assert three[3] == three[47] == three[95] == 3 and three[10] == three[51] == three[96] == three[134] == 10
    ac = mg.case("three_cohorts").lists[2]
    assert (3, 5) not in set(zip(ac.i.tolist(), ac.j.tolist()))
    assert sorted(mg.case(n).nodes for n in mg.NAMES if n.startswith("nodes_")) == [1, 63, 64, 65, 256, 257]
    for value in mg.LADDER:  # one ulp decides whether the edges scoring `value` link
        at, below, above = (mg.components(mg.answer(f"ladder_{t}_{value}")) for t in ("at", "below", "above"))
        assert at == below < above, value
    assert mg.components(mg.answer("ladder_above_1.0")) == 300  # nothing links, the NaN record least of all
    nan_case = mg.case("ladder_below_0.25")
    assert np.isnan(nan_case.lists[0].score[-1]) and mg.answer("ladder_below_0.25")[299] == 299


@pytest.mark.parametrize("name", mg.FAMILIES + ["empty_among", "overlapping_ranges"])
def test_order_of_records_and_lists_does_not_matter(name):
    from napkon_string_matching_amd import grid

    c = mg.case(name)
    for seed in (1, 2):
        s = mg.shuffled(c, seed)
        assert np.array_equal(grid.groups_of_hits(s.entries(), s.nodes, s.min_score), mg.answer(name))


def test_a_higher_min_score_only_refines():
    from napkon_string_matching_amd import grid

    c = mg.case("ladder_at_0.25")
    coarse = None
    for value in mg.LADDER + (2.0,):
        fine = grid.groups_of_hits(c.entries(), c.nodes, value)
        if coarse is not None:
            # every fine group lies inside one coarse group, and there are no fewer of them
            assert np.array_equal(coarse[fine], coarse) and mg.components(fine) >= mg.components(coarse)
        coarse = fine
    assert mg.components(coarse) == c.nodes


def test_start_links_into_a_forest_and_the_hook_model_holds():
    from napkon_string_matching_amd import grid

    c = mg.case("three_cohorts")
    whole = mg.answer("three_cohorts")
    label, hooks = None, 0
    for l in c.lists:  # one list per call
        before = c.nodes if label is None else mg.components(label)
        label = grid.groups_of_hits([l.entry()], c.nodes, c.min_score, start=label)
        hooks += before - mg.components(label)
    assert np.array_equal(label, whole)
    assert hooks == c.nodes - mg.components(whole)  # hooks made = components before - components after, summed
    # a hand-made forest that is no set of minima yet: no lists normalise it
    forest = np.array([0, 0, 1, 2, 4, 4, 5, 7, 3], dtype=np.int32)
    assert grid.groups_of_hits([], 9, start=forest).tolist() == [0, 0, 0, 0, 4, 4, 4, 7, 0]
    assert np.array_equal(grid.groups_of_hits([], 9, start=forest), mg.bfs_labels([], 9, 0.0, start=forest))
    for bad in ([0, 2], [0, -1], [0, 0, 1]):
        with pytest.raises(ValueError):
            grid.groups_of_hits([], 2, start=np.array(bad, dtype=np.int32))


def test_ids_outside_the_nodes_are_refused_whatever_the_score():
    from napkon_string_matching_amd import grid

    hits = lambda i, j: grid.Hits(np.array([-1.0]), np.array([i], dtype=np.int32), np.array([j], dtype=np.int32))
    for i, j, lb, rb in ((-1, 0, 0, 0), (0, -1, 0, 0), (5, 0, 0, 0), (0, 3, 0, 2), (0, 0, 6, 0), (0, 0, 0, -1)):
        with pytest.raises(ValueError):
            grid.groups_of_hits([(hits(i, j), lb, rb)], 5, min_score=0.5)
    assert grid.groups_of_hits([(hits(4, 2), 0, 2)], 5, min_score=-2.0).tolist() == [0, 1, 2, 3, 4]  # (4, 2 + 2): a self-loop
    assert grid.groups_of_hits([], 0).shape == (0,)


def test_match_groups_views():
    from napkon_string_matching_amd import grid

    label = mg.answer("three_cohorts")
    groups = grid.MatchGroups(label, (0, 40, 90), (40, 50, 45))
    assert np.array_equal(groups.of(1), label[40:90]) and len(groups.of(2)) == 45
    sizes = groups.sizes()
    assert sizes.sum() == 135 and sizes[3] == 4 and sizes[47] == 0
    members = groups.members()
    assert [tuple(part.tolist() for part in m) for m in members] == [
        ([3], [7, 8], [5]), ([10], [11], [6, 44]), ([20], [30], []), ([30], [], [20]), ([31], [], [21]), ([], [49], [0])]
    assert len(groups.members(min_size=1)) == mg.components(label) and groups.members(min_size=5) == []
    one = grid.MatchGroups(np.array([0, 0, 2, 0], dtype=np.int32), (0,), (4,))
    assert [m[0].tolist() for m in one.members()] == [[0, 1, 3]]


# ------------------------------------------------------------------------------------------------------------ mappings
def _comparable(left, right, rows):
    from napkon_string_matching_amd.types.comparable import Comparable

    frame = pd.DataFrame({f"{left}Identifier": [r[0] for r in rows], f"{right}Identifier": [r[1] for r in rows],
                          "MatchScore": [r[2] for r in rows]})
    return Comparable(frame, left_name=left, right_name=right)


def _results():
    from napkon_string_matching_amd.types.comparable import ComparisonResults

    return ComparisonResults({
        "hap vs pop": _comparable("Hap", "Pop", [("h2", "p1", 0.9), ("h2", "p1", 0.9), ("h1", "p3", 0.6), ("h9", "p9", 0.2)]),
        "pop vs suep": _comparable("Pop", "Suep", [("p1", "s7", 0.8), ("p3", "s7", 0.4)]),
        "hap vs suep": _comparable("Hap", "Suep", [("h5", "s1", 0.7)]),
    })


def _mapping(min_score, id_reference=None):
    from napkon_string_matching_amd import grid, groups

    cohorts, identifiers, lists = groups.lists_of_results(_results())
    nodes = sum(len(v) for v in identifiers)
    label = grid.groups_of_hits(lists, nodes, float("-inf") if min_score is None else min_score)
    return groups.mapping_of_labels(label, cohorts, identifiers, id_reference)


def test_lists_of_results_numbers_distinct_identifiers():
    from napkon_string_matching_amd import groups

    cohorts, identifiers, lists = groups.lists_of_results(_results())
    assert cohorts == ["hap", "pop", "suep"]
    assert identifiers == [["h1", "h2", "h5", "h9"], ["p1", "p3", "p9"], ["s1", "s7"]]  # h2 / p1 / s7 once each
    assert [(lb, rb) for _, lb, rb in lists] == [(0, 4), (4, 7), (0, 7)]
    assert lists[0][0].i.tolist() == [1, 1, 0, 3] and lists[0][0].j.tolist() == [0, 0, 1, 2]


def test_mapping_of_labels_entries_and_ids():
    from napkon_string_matching_amd.types.mapping import Mapping

    md5 = lambda cohort, ident: hashlib.md5(f"{cohort}\0{ident}".encode()).hexdigest()
    everything = _mapping(None).dict()
    # p3 ~ s7 joins the two hap items; only entries with at least two members; identifiers in node order
    assert everything == {md5("hap", "h1"): {"hap": ["h1", "h2"], "pop": ["p1", "p3"], "suep": ["s7"]},
                          md5("hap", "h5"): {"hap": ["h5"], "suep": ["s1"]},
                          md5("hap", "h9"): {"hap": ["h9"], "pop": ["p9"]}}
    assert all(re.fullmatch(r"[0-9a-f]{32}", key) for key in everything)
    half = _mapping(0.5).dict()
    assert half == {md5("hap", "h1"): {"hap": ["h1"], "pop": ["p3"]},
                    md5("hap", "h2"): {"hap": ["h2"], "pop": ["p1"], "suep": ["s7"]},
                    md5("hap", "h5"): {"hap": ["h5"], "suep": ["s1"]}}
    assert _mapping(0.95).dict() == {}
    assert Mapping(everything).dict() == everything and Mapping(half).dict() == half  # round trip


def test_id_reference_precedence_and_single_use():
    from napkon_string_matching_amd.types.mapping import Mapping

    md5 = lambda cohort, ident: hashlib.md5(f"{cohort}\0{ident}".encode()).hexdigest()
    reference = Mapping({"ref-b": {"suep": ["s7"], "hap": ["h1"]}, "ref-a": {"hap": ["h2"]}, "ref-c": {"pop": ["nobody"]},
                         "ref-d": {"hap": ["h5"]}})
    # at 0.5 h1 and s7 lie in different components: ref-b goes to the first in label order (h1's), the other one -- whose
    # FIRST reference id is ref-b as well, not ref-a -- falls through to its md5
    half = _mapping(0.5, reference).dict()
    assert half == {"ref-b": {"hap": ["h1"], "pop": ["p3"]},
                    md5("hap", "h2"): {"hap": ["h2"], "pop": ["p1"], "suep": ["s7"]},
                    "ref-d": {"hap": ["h5"], "suep": ["s1"]}}
    everything = _mapping(None, reference).dict()
    assert set(everything) == {"ref-b", "ref-d", md5("hap", "h9")} and everything["ref-b"]["hap"] == ["h1", "h2"]
    # a reference in another order: the first id in ITS order that holds a member wins
    swapped = Mapping({"ref-a": {"hap": ["h2"]}, "ref-b": {"suep": ["s7"], "hap": ["h1"]}})
    assert set(_mapping(None, swapped).dict()) == {"ref-a", md5("hap", "h5"), md5("hap", "h9")}
    # a run's own output is a valid reference for the next run: the ids stay
    first = _mapping(None)
    assert _mapping(None, first).dict() == first.dict()


def test_the_mapping_is_accepted_as_a_whitelist():
    from napkon_string_matching_amd.types.mapping import Mapping

    mapping = _mapping(None)
    assert mapping.get_all_mapping_for_groups("hap", "suep") == [(["h1", "h2"], ["s7"]), (["h5"], ["s1"])]
    assert isinstance(mapping, Mapping) and len(mapping) == 3


# ------------------------------------------------------------------------------------------------------------- symbols
def test_symbol_header_and_binding():
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    assert _lib.GROUP_EXPORTS == ("nsm_group_hits",)
    assert not set(_lib.GROUP_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.ASSIGN_EXPORTS))
    fn = _lib.entry("nsm_group_hits")
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 8
    assert lib.nsm_abi_version() == 5 == _lib.ABI_VERSION and _lib.GROUP_CONTINUE == 1
    assert ctypes.sizeof(_lib.NsmHitList) == 32
    declared = lambda path: set(re.findall(r"^\s*(?:int|uint64_t|const char\*)\s+(nsm_\w+)\s*\(", path.read_text(), flags=re.M))
    assert declared(ROOT / "include" / "nsm_hip_groups.h") == set(_lib.GROUP_EXPORTS)
    assert declared(ROOT / "include" / "nsm_hip.h") == set(_lib.EXPORTS)
    text = (ROOT / "include" / "nsm_hip_groups.h").read_text()
    assert '#include "nsm_hip.h"' in text and "#define NSM_GROUP_CONTINUE 1u" in text
    assert "#define NSM_ABI_VERSION 5" in (ROOT / "include" / "nsm_hip.h").read_text()


def test_argument_checks_that_need_no_device():
    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_group_hits")
    error = lambda: _lib.load().nsm_last_error().decode()
    one = (_lib.NsmHitList * 1)()
    label = 0x1000  # (never dereferenced: every case ends before the first HIP call)

    def with_list(**fields):
        one[0] = _lib.NsmHitList(None, 0, 0, 2, 2, 2)
        for key, value in fields.items():
            setattr(one[0], key, value)
        return one

    assert fn(None, 1, 4, 0.0, 0, label, None, None) == BADARG and "null lists" in error()
    assert fn(with_list(), -1, 4, 0.0, 0, label, None, None) == BADARG and "negative count" in error()
    assert fn(with_list(), 1, -4, 0.0, 0, label, None, None) == BADARG and "negative count" in error()
    assert fn(with_list(), 1, 4, 0.0, 0, None, None, None) == BADARG and "null label" in error()
    assert fn(with_list(), 1, 4, 0.0, 2, label, None, None) == BADARG and "flag" in error()
    assert fn(with_list(), 1, 4, 0.0, 0x80000001, label, None, None) == BADARG and "flag" in error()
    assert fn(with_list(n=3), 1, 4, 0.0, 0, label, None, None) == BADARG and "null hits" in error()
    for field in ("left_base", "left_ids", "right_base", "right_ids"):
        assert fn(with_list(**{field: -1}), 1, 4, 0.0, 0, label, None, None) == BADARG and "negative base or id count" in error()
    assert fn(with_list(left_ids=5), 1, 4, 0.0, 0, label, None, None) == BADARG and "beyond" in error()
    assert fn(with_list(right_base=3), 1, 4, 0.0, 0, label, None, None) == BADARG and "beyond" in error()
    assert fn(with_list(left_base=0x7FFFFFFF, left_ids=0x7FFFFFFF), 1, 4, 0.0, 0, label, None, None) == BADARG and "beyond" in error()
    # the documented order: an earlier check wins
    assert fn(None, 1, -1, 0.0, 2, None, None, None) == BADARG and "null lists" in error()
    assert fn(with_list(n=3), 1, 4, 0.0, 2, None, None, None) == BADARG and "null label" in error()
    assert fn(with_list(n=3, left_base=-1), 1, 4, 0.0, 2, label, None, None) == BADARG and "flag" in error()
    # nodes == 0: nothing to label, no launch
    assert fn(None, 0, 0, 0.0, 0, None, None, None) == 0
    assert fn(with_list(left_ids=0, right_base=0, right_ids=0), 1, 0, 0.0, 1, None, None, None) == 0
