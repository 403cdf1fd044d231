"""One-to-one assignment on the GPU (``nsm_assign_hits``, csrc/assign.hip) against the definition
``grid.assign_of_hits``: the same records and the same doubles after the canonical sort, on every family of
tests/support/assignments.py and through each of the three routes (tests/test_cpu_assign.py checks the definition and the
round model those families are judged by).

The C entry is called through ctypes with buffers of exactly the documented sizes; ``stats`` must equal the round model's
figures for ``route="rounds"``, and the default route must be seen to run both stages.  The Python layers are compared
with ``assign_of_hits`` of the hit list the corresponding grid returns."""
import random

import numpy as np
import pandas as pd
import pytest

from support import arena as arena_mod
from support import assignments as asg
from support import probe_tables
from support import threshold_probes as tp

pytestmark = pytest.mark.gpu
ROUTES = {"default": 0, "rounds": 1, "stream": 2}
BADARG = 10001


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _entry(dev, c, flags, count0=0):
    """``nsm_assign_hits`` on the case's records: (status, out tensor with 4 sentinel records behind the documented
    capacity, capacity, counter, stats)."""
    import torch

    from napkon_string_matching_amd import _lib

    fn = _lib.entry("nsm_assign_hits")
    n = len(c)
    recs = torch.from_numpy(asg.records_bytes(c)).to(dev)
    cap = min(n, c.left_ids, c.right_ids)
    out = torch.full((cap + 4, 2), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((1,), count0, dtype=torch.int64, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = fn(recs.data_ptr() if n else 0, n, c.left_ids, c.right_ids, flags, out.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(recs.cpu().numpy().view(np.int64), asg.records_bytes(c).view(np.int64)), "the input was written"
    return rc, out, cap, int(cnt.item()), [int(v) for v in st.tolist()]


# ------------------------------------------------------------------------------------------------------------ C entry
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", asg.NAMES)
def test_entry_equals_the_definition(dev, name, route):
    c, want = asg.case(name), asg.answer(name)
    rc, out, cap, count, stats = _entry(dev, c, ROUTES[route])
    assert rc == 0
    assert count == len(want), f"{name} / {route}: counter {count}, expected {len(want)}; stats {stats}"
    assert (out[cap:] == -7.0).all(), "wrote beyond min(n, left_ids, right_ids) records"
    asg.same(asg.hits_of_records(out[:count].cpu().numpy()), want, f"{name} / {route}")
    assert stats[2] + stats[3] == len(want), stats
    matched, history, _ = asg.model(name)
    if route == "rounds":
        assert stats == [len(history), 0, len(matched), 0], (name, stats)
    if route == "stream":
        assert stats == [0, len(c), 0, len(want)], (name, stats)


def test_default_route_runs_both_stages(dev):
    for name in ("ties5_300x300", "all_ties_65x130"):  # ties: rounds stop paying, the stream stage finishes
        _, _, _, count, stats = _entry(dev, asg.case(name), 0)
        assert stats[0] >= 1 and stats[1] > 0 and stats[3] > 0 and count == len(asg.answer(name)), (name, stats)
    _, _, _, count, stats = _entry(dev, asg.case("distinct_300x300"), 0)  # distinct scores: rounds make the matches
    assert stats[0] >= 1 and stats[2] > 0 and count == len(asg.answer("distinct_300x300")), stats


def test_stats_are_added_to(dev):
    import torch

    from napkon_string_matching_amd import _lib

    c = asg.case("sparse_1025")
    fn = _lib.entry("nsm_assign_hits")
    recs = torch.from_numpy(asg.records_bytes(c)).to(dev)
    out = torch.zeros((len(c), 2), dtype=torch.float64, device=dev)
    st = torch.tensor([100, 200, 300, 400], dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for flags in (1, 2):
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        assert fn(recs.data_ptr(), len(c), c.left_ids, c.right_ids, flags, out.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream) == 0
    # (a call without stats is a call like any other)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    assert fn(recs.data_ptr(), len(c), c.left_ids, c.right_ids, 0, out.data_ptr(), cnt.data_ptr(), 0, stream) == 0
    matched, history, _ = asg.model("sparse_1025")
    assert st.tolist() == [100 + len(history), 200 + len(c), 300 + len(matched), 400 + len(matched)]
    assert int(cnt.item()) == len(matched)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("where,field,value", [("first", "i", "left_ids"), ("last", "j", "right_ids"), ("middle", "i", -1),
                                               ("middle", "j", -5)])
def test_an_id_out_of_range_is_refused(dev, route, where, field, value):
    from napkon_string_matching_amd import _lib

    base = asg.case("sparse_1025")
    r = {"first": 0, "last": len(base) - 1, "middle": 500}[where]
    i, j = base.i.copy(), base.j.copy()
    (i if field == "i" else j)[r] = getattr(base, value) if isinstance(value, str) else value
    bad = asg.Case("bad", base.score, i, j, base.left_ids, base.right_ids)  # (the order is not what is checked here)
    rc, out, _, count, stats = _entry(dev, bad, ROUTES[route], count0=5)
    assert rc == BADARG and "outside" in _lib.load().nsm_last_error().decode()
    assert count == 5 and (out == -7.0).all() and stats == [0, 0, 0, 0]


@pytest.mark.parametrize("route", ROUTES)
def test_guard_bands(dev, route):
    """Everything the entry is handed lies in one arena of random bytes: ``out`` carved at exactly
    min(n, left_ids, right_ids) records, the counter at 8 bytes, the stats at 32.  ``hits`` is byte-identical afterwards,
    no guard byte has changed."""
    import torch

    from napkon_string_matching_amd import _lib

    name = "distinct_300x300"
    c, want = asg.case(name), asg.answer(name)
    cap = min(len(c), c.left_ids, c.right_ids)
    host = asg.records_bytes(c)
    arena = arena_mod.Arena(host.nbytes + cap * 16 + 40 + 8 * (arena_mod.GUARD + arena_mod.ALIGN), dev, seed=11)
    arena.carve("hits", host.nbytes)
    arena.fill("hits", host)
    arena.carve("out", cap * 16)
    arena.carve("out_count", 8)
    arena.zero("out_count")
    arena.carve("stats", 32)
    arena.zero("stats")
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = _lib.entry("nsm_assign_hits")(arena.ptr("hits"), len(c), c.left_ids, c.right_ids, ROUTES[route], arena.ptr("out"),
                                       arena.ptr("out_count"), arena.ptr("stats"), stream)
    torch.cuda.synchronize(dev)
    assert rc == 0
    arena.check(unchanged=["hits"])
    count = int(arena.read("out_count", np.int64)[0])
    assert count == len(want)
    got = arena.read("out", np.float64).reshape(cap, 2)
    asg.same(asg.hits_of_records(got[:count].copy()), want, f"arena / {route}")
    assert np.array_equal(got[count:].view(np.uint8).ravel(), arena.poison("out")[count * 16:]), "records beyond the count were written"
    stats = arena.read("stats", np.int64).tolist()
    assert stats[2] + stats[3] == len(want)


# ------------------------------------------------------------------------------------------------------- Python layers
@pytest.mark.parametrize("route", [None, "rounds", "stream"])
@pytest.mark.parametrize("name", ["sparse_65", "sparse_8193", "all_ties_65x130", "gaps_ids_100000", "empty"])
def test_assign_hits_on_host_lists(dev, name, route):
    from napkon_string_matching_amd import grid

    c = asg.case(name)
    perm = np.random.default_rng(1).permutation(len(c))  # (any order goes in)
    stats = []
    got = grid.assign_hits(grid.Hits(c.score[perm], c.i[perm], c.j[perm]), c.left_ids, c.right_ids, device=dev, route=route,
                           stats=stats)
    asg.same(got, asg.answer(name), f"{name} / {route}")
    assert len(stats) == 4 and stats[2] + stats[3] == len(got)
    asg.same(grid.assign_hits(c.hits(), device=dev, route=route), asg.answer(name), f"{name} / {route}, ids from the list")


GRIDS = ["raw_indel_64", "raw_jaccard_16", "levels_indel_one_word", "levels_jaccard"]


def _grid_calls(g, dev):
    """(grid(thr), assign(thr, route, stats)) of a probe grid through the wrappers of its mode."""
    from napkon_string_matching_amd import grid

    cap = g.pairs
    if g.raw:
        lt, rt = probe_tables.raw_indel_tables(g, dev) if g.kind == "indel" else probe_tables.raw_jaccard_tables(g, dev)
        full, assign = (grid.indel_raw_grid, grid.indel_raw_assign) if g.kind == "indel" else \
            (grid.jaccard_raw_grid, grid.jaccard_raw_assign)
        return (lambda thr: full(lt, rt, thr, capacity=cap),
                lambda thr, route, stats: assign(lt, rt, thr, capacity=cap, route=route, stats=stats))
    tabs = probe_tables.levels_indel_tables(g, dev, False) if g.kind == "indel" else probe_tables.levels_jaccard_tables(g, dev, False)
    full, assign = (grid.indel_levels_grid, grid.indel_levels_assign) if g.kind == "indel" else \
        (grid.jaccard_levels_grid, grid.jaccard_levels_assign)
    return (lambda thr: full(*tabs, thr, category_mode=g.mode, capacity=cap),
            lambda thr, route, stats: assign(*tabs, thr, category_mode=g.mode, capacity=cap, route=route, stats=stats))


@pytest.mark.parametrize("thr", [0.3, 0.6])
@pytest.mark.parametrize("name", GRIDS)
def test_table_assign_equals_the_definition_of_the_grid(dev, name, thr):
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    assert len(g.left) >= 70 and len(g.right) == tp.N_RIGHT
    full, assign = _grid_calls(g, dev)
    hits = full(thr)
    want = grid.assign_of_hits(hits)
    assert 0 < len(want) <= len(g.left) and len(hits) > len(want)
    for route in (None, "rounds", "stream"):
        stats = []
        asg.same(assign(thr, route, stats), want, f"{name} at {thr} / {route}")
        assert stats[2] + stats[3] == len(want), (name, thr, route, stats)
    # a small first buffer: the grid's retry still ends in the same assignment
    if g.raw and g.kind == "indel":
        lt, rt = probe_tables.raw_indel_tables(g, dev)
        asg.same(grid.indel_raw_assign(lt, rt, thr, capacity=8), want, f"{name} at {thr}, grown buffer")


def test_fuzzy_match_assign_with_and_without_a_wide_item(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match

    rng = random.Random(21)
    text = lambda k: " ".join("".join(rng.choice("abcde") for _ in range(rng.randint(2, 6))) for _ in range(k))
    left, right = [text(rng.randint(1, 4)) for _ in range(12)], [text(rng.randint(1, 4)) for _ in range(14)]
    right[5], right[9] = left[2], left[2]  # a tie at the top: (2, 5) is taken, (2, 9) is not
    for wide in (False, True):
        if wide:
            left[3] = "x" * 513  # beyond the fast kernels: the general route, the merged list assigned
        for thr in (0.0, 0.4):
            got = fuzzy_match.assign(left, right, thr, device=dev)
            asg.same(got, grid.assign_of_hits(fuzzy_match.raw_grid(left, right, thr, device=dev)), f"wide {wide} at {thr}")
            assert (2, 5) in set(zip(got.i.tolist(), got.j.tolist())) and 9 not in got.j[got.i == 2]
    assert len(fuzzy_match.assign(left, right, 0.0, device=dev)) == 12
    assert len(fuzzy_match.assign([], right, 0.0, device=dev)) == 0 == len(fuzzy_match.assign(left, [], 0.0, device=dev))


def test_intersection_vs_union_assign_with_and_without_a_wide_item(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import intersection_vs_union

    rng = random.Random(22)
    words = [f"w{q}" for q in range(10)]
    row = lambda: rng.sample(words, rng.randint(1, 4))
    left, right = [row() for _ in range(12)], [row() for _ in range(14)]
    many = [f"x{q}" for q in range(70)]
    for wide in (False, True):
        if wide:
            left[4], right[6] = many[:65], many[3:68] + words[:2]  # 65 distinct tokens and more: the general route
        for thr in (0.0, 0.3):
            got = intersection_vs_union.assign(left, right, thr, device=dev)
            asg.same(got, grid.assign_of_hits(intersection_vs_union.raw_grid(left, right, thr, device=dev)), f"wide {wide} at {thr}")
        if wide:
            assert (4, 6) in set(zip(got.i.tolist(), got.j.tolist()))
    with pytest.raises(ZeroDivisionError):
        intersection_vs_union.assign(["a b", ""], ["a", ""], 0.5, device=dev)


# ------------------------------------------------------------------------------------------------------------ compare
def _frame(rows):
    return pd.DataFrame(rows, columns=["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"])


def _cohort(seed, n, words, zero_at):
    rng = random.Random(seed)
    rows = []
    for k in range(n):
        toks = [rng.choice(words) for _ in range(rng.randint(1, 6))]
        term = [" ".join(toks[q:q + 2]) for q in range(0, len(toks), 2)]
        cat = [f"c{k % 3}"]
        if k == zero_at:  # zero levels; a category of its own, so that it only meets the other side's zero-level item
            term, cat = [], ["none"]
        rows.append([f"{seed}-{k}", f"v{k}", "s", cat, term, toks, "p"])
    return _frame(rows)


def _rows(comparable):
    frame = comparable.dataframe()
    return [(s, a, b) for s, a, b in zip(frame["MatchScore"].tolist(), frame["HapIdentifier"].tolist(), frame["PopIdentifier"].tolist())]


def _reduced(rows):
    """The definition on a frame's rows: identifiers are "<seed>-<position>", positions break ties."""
    from napkon_string_matching_amd import grid

    pos = lambda ident: int(ident.split("-")[1])
    hits = grid.Hits(np.array([r[0] for r in rows], dtype=np.float64), np.array([pos(r[1]) for r in rows], dtype=np.int32),
                     np.array([pos(r[2]) for r in rows], dtype=np.int32))
    taken = grid.assign_of_hits(hits)
    seeds = (rows[0][1].split("-")[0], rows[0][2].split("-")[0])
    return [(s, f"{seeds[0]}-{a}", f"{seeds[1]}-{b}") for s, a, b in taken.as_tuples()]


@pytest.mark.parametrize("score_func", ["intersection_vs_union", "fuzzy_match"])
def test_compare_one_to_one(score_func, tmp_path):
    """``compare(one_to_one=True)`` is ``assign_of_hits`` of the rows of the plain ``compare()``: after categories and
    blacklist, the zero-level pair (score 0) a row like any other; the same when assigned at a cache threshold below
    ``score_threshold`` (the prefix property)."""
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    words = [f"word{q}" for q in range(12)]
    left, right = Questionnaire(_cohort(1, 30, words, 4)), Questionnaire(_cohort(2, 35, words, 7))
    kw = dict(score_func=score_func, compare_column="Term", left_name="hap", right_name="pop", filter_categories=True)
    plain = left.compare(right, None, None, score_threshold=0.0, cached=False, **kw)
    top = plain.dataframe().iloc[0]
    blacklist = {"b": {"hap": [top["HapIdentifier"]], "pop": [top["PopIdentifier"]]}}
    for black in (None, blacklist):
        for thr in (0.0, 0.3):
            rows = _rows(left.compare(right, None, black, score_threshold=thr, cached=False, **kw))
            got = _rows(left.compare(right, None, black, score_threshold=thr, cached=False, one_to_one=True, **kw))
            want = _reduced(rows)
            assert sorted(got) == sorted(want) and 0 < len(want) < len(rows), (score_func, thr, black is not None)
            assert len({a for _, a, _ in got}) == len(got) == len({b for _, _, b in got})
            if black is not None:
                assert (top["HapIdentifier"], top["PopIdentifier"]) not in {(a, b) for _, a, b in got}
            if thr == 0.0:  # (the zero-level pair scores 0 and is the only row of both its items)
                assert (0.0, "1-4", "2-7") in got
    # assigned at cache_threshold 0.1, the rows filtered at 0.3 afterwards
    rows = _rows(left.compare(right, None, blacklist, score_threshold=0.3, cached=False, **kw))
    got = _rows(left.compare(right, None, blacklist, score_threshold=0.3, cache_threshold=0.1, cache_dir=tmp_path,
                             one_to_one=True, **kw))
    assert sorted(got) == sorted(_reduced(rows)) and len(got) > 0
    again = _rows(left.compare(right, None, blacklist, score_threshold=0.3, cache_threshold=0.1, cache_dir=tmp_path,
                               one_to_one=True, **kw))
    assert sorted(again) == sorted(got)  # (read back from its own cache file)
    left.compare(right, None, blacklist, score_threshold=0.3, cache_threshold=0.1, cache_dir=tmp_path, **kw)
    assert len(list(tmp_path.iterdir())) == 2  # (the plain call has a key of its own)


def test_matcher_config_passes_one_to_one(dev):
    """``matching.one_to_one`` of a ``Matcher`` config reaches ``compare`` the way ``top_k`` does."""
    from napkon_string_matching_amd.matcher import Matcher
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    words = [f"word{q}" for q in range(12)]
    cohorts = {"hap": Questionnaire(_cohort(1, 20, words, -1)), "pop": Questionnaire(_cohort(2, 25, words, -1))}
    matching = dict(score_func="fuzzy_match", compare_column="Term", score_threshold=0.2, cached=False)
    want = _reduced(_rows(cohorts["hap"].compare(cohorts["pop"], None, None, left_name="hap", right_name="pop", **matching)))
    matcher = Matcher(None, {"matching": dict(matching, one_to_one=True)}, questionnaires=cohorts)
    matcher.match_questionnaires()
    ((_, result),) = matcher.results.items()
    assert sorted(_rows(result)) == sorted(want) and len(want) > 0
