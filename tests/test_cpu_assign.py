"""One-to-one assignment without a GPU: ``grid.assign_of_hits`` (the definition) against a plain walk and against the
round scheme's restatement (tests/support/assignments.py) on every family, the three consequences of the definition
(one-to-one and maximal; the prefix property; first-round matches are mutual bests), the device-free argument checks of
``nsm_assign_hits`` and the keyword validation of ``compare``.

Entry errors: every case ends in host code before the entry's first HIP call -- read off csrc/assign.hip: the argument
checks and the ``n == 0`` return precede ``hipStreamIsCapturing``, the first HIP call.  A case that expects success
therefore has ``n == 0``."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from support import assignments as asg

ROOT = Path(__file__).resolve().parent.parent
BADARG, UNSUPPORTED = 10001, 10002


# ------------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("name", asg.NAMES)
def test_definition_is_the_walk_and_the_round_model_agrees(name):
    c = asg.case(name)
    got = asg.answer(name)
    ranks = asg.walk(c)
    assert got.i.tolist() == c.i[ranks].tolist() and got.j.tolist() == c.j[ranks].tolist()
    assert np.array_equal(got.score.view(np.int64), c.score[ranks].view(np.int64))
    matched, history, _ = asg.model(name)
    assert matched == ranks, f"{name}: the round scheme's matches differ from the walk's"
    assert all(b < a for a, b in zip(history, history[1:])), "a round without progress"
    if name in asg.MODEL_ROUNDS:
        assert len(history) == asg.MODEL_ROUNDS[name], (name, history)


def test_every_family_is_listed():
    assert sorted(asg.NAMES) == sorted(asg.cases()) and len(set(asg.NAMES)) == len(asg.NAMES)
    for name in asg.NAMES:
        c = asg.case(name)
        keys = list(zip((-c.score).tolist(), c.i.tolist(), c.j.tolist()))
        assert keys == sorted(keys), f"{name} is not in canonical order"
        if len(c):
            assert 0 <= c.i.min() and c.i.max() < c.left_ids and 0 <= c.j.min() and c.j.max() < c.right_ids
    assert asg.case("gaps_ids_100000").i.max() < 3000 and asg.case(f"gaps_ids_{60 * 41 + 5}").i.max() == 60 * 41 + 4


def test_expected_shapes_of_the_families():
    ties = asg.answer("all_ties_65x130")
    assert ties.i.tolist() == list(range(65)) == ties.j.tolist()
    assert len(asg.answer("perfect_2049")) == 2049 and len(asg.answer("star_1x300")) == 1 == len(asg.answer("star_300x1"))
    assert len(asg.answer("runs_of_64")) == 20  # one winner per run
    twice = asg.answer("every_record_twice")
    assert len(set(zip(twice.i.tolist(), twice.j.tolist()))) == len(twice) > 0
    assert len(asg.answer("empty")) == 0 and asg.answer("one_record").as_tuples() == [(0.25, 3, 2)]


@pytest.mark.parametrize("name", asg.NAMES)
def test_one_to_one_and_maximal(name):
    c, got = asg.case(name), asg.answer(name)
    assert len(set(got.i.tolist())) == len(got) == len(set(got.j.tolist()))
    used_l, used_r = set(got.i.tolist()), set(got.j.tolist())
    assert all(a in used_l or b in used_r for a, b in zip(c.i.tolist(), c.j.tolist())), "a record has both items free"
    assert len(got) <= min(len(c), c.left_ids, c.right_ids)


@pytest.mark.parametrize("name", asg.NAMES)
def test_prefix_property_at_every_distinct_score(name):
    from napkon_string_matching_amd import grid

    c, full = asg.case(name), asg.answer(name)
    scores = sorted(set(c.score.tolist()))
    if len(scores) > 60:  # (every 60th-quantile of many distinct scores, and both ends)
        scores = sorted(set(scores[:: max(1, len(scores) // 60)] + scores[-2:]))
    for t in scores:
        keep = c.score >= t
        got = grid.assign_of_hits(grid.Hits(c.score[keep], c.i[keep], c.j[keep]))
        cut = full.score >= t
        asg.same(got, grid.Hits(full.score[cut], full.i[cut], full.j[cut]), f"{name} at {t!r}")


@pytest.mark.parametrize("name", asg.NAMES)
def test_first_round_matches_are_mutual_bests(name):
    from napkon_string_matching_amd import grid

    c = asg.case(name)
    _, _, first = asg.model(name)
    mutual = grid.best_of_hits(c.hits(), 0.0, mutual=True)
    assert {(int(c.i[r]), int(c.j[r])) for r in first} <= set(zip(mutual.i.tolist(), mutual.j.tolist()))
    assert len(first) > 0 or len(c) == 0


def test_definition_accepts_any_order():
    from napkon_string_matching_amd import grid

    c = asg.case("sparse_257")
    perm = np.random.default_rng(3).permutation(len(c))
    asg.same(grid.assign_of_hits(grid.Hits(c.score[perm], c.i[perm], c.j[perm])), asg.answer("sparse_257"), "shuffled")


def test_route_names():
    from napkon_string_matching_amd import _lib, grid

    assert grid.ASSIGN_ROUTES == {None: 0, "rounds": _lib.ASSIGN_ROUNDS_ONLY, "stream": _lib.ASSIGN_STREAM_ONLY}
    with pytest.raises(ValueError):
        grid.assign_hits(asg.case("one_record").hits(), route="fast")


# ----------------------------------------------------------------------------------------------------------- the C entry
def _call(hits=True, n=1, left_ids=10, right_ids=10, flags=0, out=True, out_count=True):
    """(status, message) of ``nsm_assign_hits`` with host addresses where a device pointer is due: no call here may read or
    write them."""
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    rec, res = _lib.NsmHit(score=7.0, i=1, j=2), _lib.NsmHit(score=-3.0, i=5, j=6)
    count = ctypes.c_ulonglong(41)
    rc = lib.nsm_assign_hits(ctypes.addressof(rec) if hits else None, n, left_ids, right_ids, flags,
                             ctypes.addressof(res) if out else None, ctypes.addressof(count) if out_count else None, None, None)
    assert (rec.score, rec.i, rec.j, res.score, res.i, res.j, count.value) == (7.0, 1, 2, -3.0, 5, 6, 41)
    return rc, (lib.nsm_last_error().decode() if rc else None)


ENTRY_CASES = [
    ("null hits", dict(hits=False), BADARG, "nsm_assign_hits: null hits with n > 0"),
    ("null out", dict(out=False), BADARG, "nsm_assign_hits: null out with n > 0"),
    ("null hits speaks before null out", dict(hits=False, out=False), BADARG, "nsm_assign_hits: null hits with n > 0"),
    ("null out_count", dict(out_count=False), BADARG, "nsm_assign_hits: null out_count"),
    ("null out_count on an empty list", dict(out_count=False, n=0), BADARG, "nsm_assign_hits: null out_count"),
    ("negative left_ids", dict(left_ids=-1), BADARG, "nsm_assign_hits: negative ids bound (left_ids -1, right_ids 10)"),
    ("negative right_ids", dict(right_ids=-7, n=0), BADARG, "nsm_assign_hits: negative ids bound (left_ids 10, right_ids -7)"),
    ("both routes", dict(flags=3), BADARG, "nsm_assign_hits: NSM_ASSIGN_ROUNDS_ONLY and NSM_ASSIGN_STREAM_ONLY exclude each other"),
    ("negative ids speak before the size", dict(left_ids=-1, n=1 << 31), BADARG,
     "nsm_assign_hits: negative ids bound (left_ids -1, right_ids 10)"),
    ("2^31 records", dict(n=1 << 31), UNSUPPORTED, "nsm_assign_hits: 2147483648 records, ranks are 32-bit (at most 2^31 - 1)"),
    ("2^40 records", dict(n=1 << 40), UNSUPPORTED, "nsm_assign_hits: 1099511627776 records, ranks are 32-bit (at most 2^31 - 1)"),
    ("empty list", dict(n=0), 0, None),
    ("empty list, null hits and out", dict(n=0, hits=False, out=False), 0, None),
    ("empty list, no ids", dict(n=0, left_ids=0, right_ids=0, flags=1), 0, None),
]


@pytest.mark.parametrize("label,kw,status,message", ENTRY_CASES, ids=[c[0] for c in ENTRY_CASES])
def test_entry_argument_checks(label, kw, status, message):
    assert _call(**kw) == (status, message)


def test_symbol_header_and_binding():
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    assert _lib.ASSIGN_EXPORTS == ("nsm_assign_hits",) and not set(_lib.ASSIGN_EXPORTS) & set(_lib.EXPORTS)
    fn = _lib.entry("nsm_assign_hits")
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert lib.nsm_abi_version() == 5 == _lib.ABI_VERSION
    declared = lambda path: set(re.findall(r"^\s*(?:int|uint64_t|const char\*)\s+(nsm_\w+)\s*\(", path.read_text(), flags=re.M))
    assert declared(ROOT / "include" / "nsm_hip_assign.h") == {"nsm_assign_hits"}
    assert "nsm_assign_hits" not in declared(ROOT / "include" / "nsm_hip.h")
    assert '#include "nsm_hip.h"' in (ROOT / "include" / "nsm_hip_assign.h").read_text()
    with pytest.raises(_lib.NsmLibraryError):
        _lib.entry("nsm_no_such_entry")


# ------------------------------------------------------------------------------------------------------ compare keywords
def _questionnaire():
    import pandas as pd

    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    rows = [[f"id{k}", f"v{k}", "s", ["c"], ["alpha beta"], ["alpha", "beta"], "p"] for k in range(3)]
    return Questionnaire(pd.DataFrame(rows, columns=["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"]))


@pytest.mark.parametrize("method", ["compare", "gen_comparable"])
def test_compare_refuses_one_to_one_with_a_per_item_query(method):
    q = _questionnaire()
    kw = dict(score_func="fuzzy_match", compare_column="Term", left_name="a", right_name="b")
    call = lambda **extra: getattr(q, method)(q, None, None, **kw, **extra)
    with pytest.raises(ValueError, match="one_to_one and top_k"):
        call(one_to_one=True, top_k=2)
    with pytest.raises(ValueError, match="one_to_one and best_margin"):
        call(one_to_one=True, best_margin=0.0)
    with pytest.raises(ValueError, match="one_to_one must be a bool"):
        call(one_to_one="yes")
    with pytest.raises(ValueError):  # (k is checked first, as before)
        call(one_to_one=True, top_k=0)


def test_cache_key_gains_one_to_one_only_when_set():
    q = _questionnaire()
    kwargs = dict(score_func="fuzzy_match", left_name="a", right_name="b")
    plain = q._hash_compare_args(q, None, None, "Term", 0.1, kwargs)
    assert q._hash_compare_args(q, None, None, "Term", 0.1, kwargs, None, None, False, False) == plain
    assert q._hash_compare_args(q, None, None, "Term", 0.1, kwargs, one_to_one=True) != plain
