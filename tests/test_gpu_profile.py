"""Threshold profiles on the GPU (``nsm_*_profile``: the top-k kernels with the tally sink of csrc/score_tally.hpp) against
the definition: the oracle's hit list at ``t[0]``, counted per threshold, and its maxima per left and per right item --
counts equal, best scores bit for bit, ``-1.0`` for an item without a hit.

The probe grids (tests/support/threshold_probes.py) put the ladder exactly on scores shared by many pairs, and one ulp to
either side: a count that is off by a pair, or a comparison with a margin, shows there.  Tables are built as the probe
tests of the threshold grids build them (imported, not copied)."""
import ctypes
import random

import numpy as np
import pandas as pd
import pytest

from support import probe_tables
from support import threshold_probes as tp

pytestmark = pytest.mark.gpu
PRUNE = {"prune": True, "no_prune": False}


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _expect(records, ladder, n_left, n_right):
    """The definition in plain Python, from (score, i, j) records of a grid at or below ``ladder[0]``."""
    kept = [r for r in records if r[0] >= ladder[0]]
    pairs = [sum(1 for r in kept if r[0] >= t) for t in ladder]
    left, right = [-1.0] * n_left, [-1.0] * n_right
    for s, i, j in kept:
        left[i], right[j] = max(left[i], s), max(right[j], s)
    return pairs, left, right


def _assert_profile(prof, records, ladder, n_left, n_right, what):
    pairs, left, right = _expect(records, ladder, n_left, n_right)
    assert prof.pairs.dtype == np.uint64 and prof.pairs.tolist() == pairs, f"{what}: pairs"
    # (tolist() compares the doubles themselves: bit for bit, scores are never NaN or -0.0)
    assert prof.left_best.tolist() == left, f"{what}: left_best"
    assert prof.right_best.tolist() == right, f"{what}: right_best"
    assert prof.matched_left().tolist() == [sum(1 for b in left if b >= t) for t in ladder]
    assert prof.matched_right().tolist() == [sum(1 for b in right if b >= t) for t in ladder]


def _ladders(g):
    t = tp.thresholds_around(tp.probes_of(g))
    return [t[k:k + 64] for k in range(0, len(t), 64)]


# ------------------------------------------------------------------------------------------------------- probe grids
def _profile_call(g, dev):
    """``run(ladder, prune)`` for a probe grid, through the grid-level wrapper of its mode."""
    from napkon_string_matching_amd import grid

    if g.raw and g.kind == "indel":
        lt, rt = probe_tables.raw_indel_tables(g, dev)
        return lambda t, prune: grid.indel_raw_profile(lt, rt, t, prune=prune)
    if g.raw:
        lt, rt = probe_tables.raw_jaccard_tables(g, dev)
        return lambda t, prune: grid.jaccard_raw_profile(lt, rt, t, prune=prune)
    if g.kind == "indel":
        tabs = probe_tables.levels_indel_tables(g, dev, False)
        return lambda t, prune, banned=None: grid.indel_levels_profile(*tabs, t, category_mode=g.mode, prune=prune, banned=banned)
    lt, rt = probe_tables.levels_jaccard_tables(g, dev, False)
    return lambda t, prune, banned=None: grid.jaccard_levels_profile(lt, rt, t, category_mode=g.mode, prune=prune, banned=banned)


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("name", tp.EVERY)
def test_probe_grids(dev, name, route):
    g = tp.grid(name)
    run = _profile_call(g, dev)
    records = tp.all_scores(g)
    for ladder in _ladders(g):
        _assert_profile(run(ladder, PRUNE[route]), records, ladder, len(g.left), len(g.right), f"{name} / {route} from {ladder[0]!r}")


# ------------------------------------------------------------------------------------------------------ small shapes
LADDER_64 = [0.0] + [k / 64 for k in range(1, 64)]


def _small_strings(rng, n):
    return ["".join(rng.choice("abcd") for _ in range(rng.choice((0, 1, 3, 9, 20)))) for _ in range(n)]


@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_small_fuzzy(dev, n, m):
    """Fewer rows than a wave's 8, exactly 8, one more; right sides around one chunk of 64.  At 0.0 every pair is a hit,
    empty strings included."""
    from napkon_string_matching_amd import grid, tables
    from oracle import native

    rng = random.Random(n * 100 + m)
    left, right = _small_strings(rng, n), _small_strings(rng, m)
    left[0] = right[-1] = ""
    units = lambda rows: native.csr([[ord(c) for c in s] for s in rows])
    records = native.indel_raw(units(left), units(right), 0.0, cap=n * m + 1)
    assert len(records) == n * m
    lt, rt = tables.encode_strings(left, right, dev)
    for ladder in ([0.0], LADDER_64, [1.5, 2.0]):
        for prune in (True, False):
            prof = grid.indel_raw_profile(lt, rt, ladder, prune=prune)
            _assert_profile(prof, records, ladder, n, m, f"{n} x {m} T={len(ladder)} prune={prune}")
            if ladder[0] == 0.0:
                assert int(prof.pairs[0]) == n * m
            else:  # a ladder entirely above the best score
                assert not prof.pairs.any() and (prof.left_best == -1.0).all() and (prof.right_best == -1.0).all()


@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_small_jaccard(dev, n, m):
    from napkon_string_matching_amd import grid, tables
    from oracle import native

    rng = random.Random(n * 1000 + m)
    rows = lambda k, low: [rng.sample(range(12), rng.randint(low, 6)) for _ in range(k)]
    left, right = rows(n, 1), rows(m, 0)
    right[0] = []
    records = native.jaccard_raw(native.csr(left), native.csr(right), 0.0, cap=n * m + 1)
    assert len(records) == n * m

    def padded(side):
        ids = np.full((len(side), 16), -1, dtype=np.int32)
        for r, row in enumerate(side):
            ids[r, : len(row)] = row
        return ids

    lt = tables.SetTable.from_padded(padded(left), "left", dev, width=16)
    rt = tables.SetTable.from_padded(padded(right), "right", dev, width=16)
    for ladder in ([0.0], LADDER_64, [1.5, 2.0]):
        for prune in (True, False):
            _assert_profile(grid.jaccard_raw_profile(lt, rt, ladder, prune=prune), records, ladder, n, m,
                            f"{n} x {m} T={len(ladder)} prune={prune}")


@pytest.mark.parametrize("n,m", [(0, 5), (5, 0), (0, 0)])
def test_empty_side(dev, n, m):
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union

    for plugin in (fuzzy_match, intersection_vs_union):
        prof = plugin.profile(["ab cd"] * n, ["ab ef"] * m, [0.0, 0.5], device=dev)
        assert prof.pairs.tolist() == [0, 0] and prof.left_best.tolist() == [-1.0] * n and prof.right_best.tolist() == [-1.0] * m


# ------------------------------------------------------------------------------------------------------------ levels
@pytest.mark.parametrize("name", ["levels_indel_one_word-cat2_lanes", "levels_indel_multi_word_128", "levels_jaccard",
                                  "levels_jaccard-cat2_lanes"])
def test_blacklist_removes_a_rows_best(dev, name):
    """The best pair of every third left item is banned: its ``left_best`` drops to the runner-up and every count loses
    the banned pairs at or above its threshold."""
    g = tp.grid(name)
    run = _profile_call(g, dev)
    records = tp.all_scores(g)
    best = {}
    for s, i, j in records:  # (score descending: the first record of a row is its best)
        best.setdefault(i, (s, j))
    banned = {(i, j) for i, (s, j) in best.items() if i % 3 == 0 and s > 0.0}
    assert len(banned) > 10
    allowed = [r for r in records if (r[1], r[2]) not in banned]
    ban = (np.array([p[0] for p in sorted(banned)]), np.array([p[1] for p in sorted(banned)]))
    ladder = _ladders(g)[0][:20]
    for prune in (True, False):
        prof = run(ladder, prune, ban)
        _assert_profile(prof, allowed, ladder, len(g.left), len(g.right), f"{name} prune={prune}")
    plain = run(ladder, True)
    dropped = [i for i, _ in banned if plain.left_best[i] >= ladder[0] and prof.left_best[i] < plain.left_best[i]]
    assert dropped, "no row's best score moved"


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


@pytest.mark.parametrize("score_func", ["intersection_vs_union", "fuzzy_match"])
def test_compare_profile_with_a_zero_level_item(score_func):
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    words = [f"word{q}" for q in range(12)]
    left, right = Questionnaire(_cohort(1, 30, words, 4)), Questionnaire(_cohort(2, 35, words, 7))
    kw = dict(score_func=score_func, compare_column="Term", left_name="hap", right_name="pop", filter_categories=True)
    ladder = [0.0, 0.1, 0.2, 0.3, 0.5]
    frames = [left.compare(right, None, None, score_threshold=t, cached=False, **kw).dataframe() for t in ladder]
    prof = left.compare_profile(right, ladder, None, None, **kw)
    assert prof.pairs.tolist() == [len(f) for f in frames] and len(frames[0]) > len(frames[1]) > len(frames[-1]) > 0
    assert prof.left_best.shape == (30,) and prof.right_best.shape == (35,)
    assert prof.left_best[4] == 0.0 and prof.right_best[7] == 0.0  # the zero-level pair scores 0: a hit at 0.0 only
    want = frames[0].groupby("HapIdentifier")["MatchScore"].max()
    assert {f"1-{i}": b for i, b in enumerate(prof.left_best.tolist()) if b >= 0.0} == want.to_dict()
    want = frames[0].groupby("PopIdentifier")["MatchScore"].max()
    assert {f"2-{j}": b for j, b in enumerate(prof.right_best.tolist()) if b >= 0.0} == want.to_dict()
    # a blacklist goes to the kernel
    top = frames[1].iloc[0]
    blacklist = {"b": {"hap": [top["HapIdentifier"]], "pop": [top["PopIdentifier"]]}}
    banned = left.compare_profile(right, ladder, None, blacklist, **kw)
    assert banned.pairs.tolist() == [len(left.compare(right, None, blacklist, score_threshold=t, cached=False, **kw)) for t in ladder]
    assert banned.pairs[1] == prof.pairs[1] - 1


# ------------------------------------------------------------------------------------------------------ public faces
def test_fuzzy_match_profile_with_wide_items(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match

    rng = random.Random(11)
    text = lambda n: " ".join("".join(rng.choice("abcde") for _ in range(rng.randint(2, 6))) for _ in range(n))
    left = [text(rng.randint(1, 5)) for _ in range(21)]
    right = [text(rng.randint(1, 5)) for _ in range(70)]
    left[3], right[40] = text(150), text(160)  # more than 512 code units: the general kernel's share
    assert len(left[3]) > 512 and len(right[40]) > 512
    ladder = [0.3, 0.4, 0.5, 0.6, 0.8]
    want = grid.profile_of_hits(fuzzy_match.raw_grid(left, right, ladder[0], device=dev), ladder, len(left), len(right))
    got = fuzzy_match.profile(left, right, ladder, device=dev)
    assert got.pairs.tolist() == want.pairs.tolist() and got.pairs[0] > 0
    assert got.left_best.tolist() == want.left_best.tolist() and got.right_best.tolist() == want.right_best.tolist()
    assert got.left_best[3] >= ladder[0] and got.right_best[40] >= ladder[0]


def test_intersection_vs_union_profile_with_wide_items(dev):
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.compare.score_functions import intersection_vs_union

    rng = random.Random(12)
    words = [f"w{q}" for q in range(40)]
    row = lambda: rng.sample(words, rng.randint(1, 8))
    left, right = [row() for _ in range(21)], [row() for _ in range(70)]
    many = [f"x{q}" for q in range(90)]
    left[5], right[9] = many[:80] + words[:3], many[10:90] + words[:2]  # more than 64 distinct tokens
    ladder = [0.1, 0.2, 1 / 3, 0.5, 1.0]
    want = grid.profile_of_hits(intersection_vs_union.raw_grid(left, right, ladder[0], device=dev), ladder, len(left), len(right))
    got = intersection_vs_union.profile(left, right, ladder, device=dev)
    assert got.pairs.tolist() == want.pairs.tolist() and got.pairs[0] > 0
    assert got.left_best.tolist() == want.left_best.tolist() and got.right_best.tolist() == want.right_best.tolist()
    assert got.left_best[5] > 0.5 and got.right_best[9] > 0.5


# ------------------------------------------------------------------------------------------------------------ errors
def test_empty_vs_empty_jaccard_raises(dev):
    from napkon_string_matching_amd.compare.score_functions import intersection_vs_union

    with pytest.raises(ZeroDivisionError):
        intersection_vs_union.profile(["a b", ""], ["a", ""], [0.1, 0.5], device=dev)
    with pytest.raises(ValueError):  # the ladder is checked first
        intersection_vs_union.profile(["a b", ""], ["a", ""], [0.5, 0.1], device=dev)


def test_c_entries_refuse_bad_arguments(dev):
    import torch

    from napkon_string_matching_amd import _lib, tables

    lib = _lib.load()
    BADARG = 10001
    lt, rt = tables.encode_strings(["abc", "abd"], ["abc", "xyz", ""], dev)
    g = tp.grid("levels_jaccard")
    jl, jr = probe_tables.levels_jaccard_tables(g, dev, False)
    il = probe_tables.levels_indel_tables(tp.grid("levels_indel_one_word"), dev, False)
    pairs = torch.full((64,), 7, dtype=torch.int64, device=dev)
    lb = torch.full((128,), 5.0, dtype=torch.float64, device=dev)
    rb = torch.full((256,), 5.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    arr = lambda values: (ctypes.c_double * max(1, len(values)))(*values)

    def raw(entry, l, r):
        return lambda t, n, p=pairs.data_ptr(), a=lb.data_ptr(), b=rb.data_ptr(): getattr(lib, entry)(
            l.struct(), r.struct(), t, n, _lib.FLAG_PRUNE, p, a, b, 0, stream)

    def levels(entry, tabs):
        return lambda t, n, p=pairs.data_ptr(), a=lb.data_ptr(), b=rb.data_ptr(), bs=0, bj=0: getattr(lib, entry)(
            *[x.struct() for x in tabs], t, n, 0, _lib.FLAG_PRUNE, bs, bj, p, a, b, 0, stream)

    calls = {"nsm_indel_raw_profile": raw("nsm_indel_raw_profile", lt, rt),
             "nsm_jaccard_raw_profile": raw("nsm_jaccard_raw_profile", jl, jr),
             "nsm_indel_levels_profile": levels("nsm_indel_levels_profile", il),
             "nsm_jaccard_levels_profile": levels("nsm_jaccard_levels_profile", (jl, jr))}
    for name, call in calls.items():
        assert call(arr([0.5]), 0) == BADARG, name
        assert call(arr([k / 100 for k in range(65)]), 65) == BADARG, name
        assert call(arr([0.5, 0.4]), 2) == BADARG, name
        assert call(arr([0.5, 0.5]), 2) == BADARG, name
        assert call(arr([0.1, float("nan")]), 2) == BADARG, name
        assert call(None, 1) == BADARG, name
        assert call(arr([0.5]), 1, p=0) == BADARG and call(arr([0.5]), 1, a=0) == BADARG and call(arr([0.5]), 1, b=0) == BADARG, name
        assert b"nsm_" in lib.nsm_last_error()
    # the levels entries' own table checks: half a blacklist
    assert calls["nsm_jaccard_levels_profile"](arr([0.5]), 1, bs=pairs.data_ptr()) == BADARG
    assert calls["nsm_indel_levels_profile"](arr([0.5]), 1, bj=pairs.data_ptr()) == BADARG
    # a stride mismatch of the RAW entry's tables
    wide_l, _ = tables.encode_strings(["a" * 100], ["b"], dev)
    assert lib.nsm_indel_raw_profile(wide_l.struct(), rt.struct(), arr([0.5]), 1, 0, pairs.data_ptr(), lb.data_ptr(), rb.data_ptr(),
                                     0, stream) == BADARG
    torch.cuda.synchronize(dev)
    # ... and nothing was launched: the outputs are untouched
    assert (pairs == 7).all() and (lb == 5.0).all() and (rb == 5.0).all()
    # a good call initialises its outputs itself
    assert calls["nsm_indel_raw_profile"](arr([0.0, 0.9]), 2) == 0
    torch.cuda.synchronize(dev)
    assert pairs[:2].tolist() == [6, 1] and lb[:2].tolist() == [1.0, (1.0 - 2.0 / 6.0) * 100.0 / 100.0] and rb[:3].tolist() == [1.0, 0.0, 0.0]
    assert (pairs[2:] == 7).all() and (lb[2:] == 5.0).all() and (rb[3:] == 5.0).all()


def test_c_entries_with_an_empty_table(dev):
    """The C entries' own handling of a side without rows (the Python faces return before any call): the outputs are
    initialised -- ``pairs`` to 0, the other side's caller ids to -1.0 -- and no sweep runs.  An empty table still needs its
    columns: a null one is NSM_E_BADARG at any row count, as for the top-k entries."""
    import torch

    from napkon_string_matching_amd import _lib, tables

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = (ctypes.c_double * 3)(0.0, 0.5, 1.0)
    st, jt = tables.encode_strings(["abc", "abd"], ["abc", "xyz", ""], dev)
    jl, jr = probe_tables.levels_jaccard_tables(tp.grid("levels_jaccard"), dev, False)
    il, ils, ir, irs = probe_tables.levels_indel_tables(tp.grid("levels_indel_one_word"), dev, False)

    def entries(empty_left):
        """(name, call(pairs, left_best, right_best, stats), rows left, rows right) with one side's row count set to 0."""
        def cut(table, left):
            s = table.struct()  # (a fresh struct per call)
            if left == empty_left:
                s.n = 0
            return s

        a, b = cut(st, True), cut(jt, False)
        yield "nsm_indel_raw_profile", lambda p, l, r, s: lib.nsm_indel_raw_profile(a, b, t, 3, _lib.FLAG_PRUNE, p, l, r, s, stream), a.n, b.n
        c, d = cut(jl, True), cut(jr, False)
        yield "nsm_jaccard_raw_profile", lambda p, l, r, s: lib.nsm_jaccard_raw_profile(c, d, t, 3, _lib.FLAG_PRUNE, p, l, r, s, stream), c.n, d.n
        yield ("nsm_jaccard_levels_profile",
               lambda p, l, r, s: lib.nsm_jaccard_levels_profile(c, d, t, 3, 0, _lib.FLAG_PRUNE, 0, 0, p, l, r, s, stream), c.n, d.n)
        e, f, es, fs = cut(il, True), cut(ir, False), ils.struct(), irs.struct()
        yield ("nsm_indel_levels_profile",
               lambda p, l, r, s: lib.nsm_indel_levels_profile(e, es, f, fs, t, 3, 0, _lib.FLAG_PRUNE, 0, 0, p, l, r, s, stream), e.n, f.n)

    for empty_left in (True, False):
        for name, call, n, m in entries(empty_left):
            assert (n == 0) != (m == 0) and n + m > 0, name
            pairs = torch.full((8,), 7, dtype=torch.int64, device=dev)
            lb = torch.full((n + 4,), 5.0, dtype=torch.float64, device=dev)
            rb = torch.full((m + 4,), 5.0, dtype=torch.float64, device=dev)
            stats = torch.zeros(4, dtype=torch.int64, device=dev)
            assert call(pairs.data_ptr(), lb.data_ptr(), rb.data_ptr(), stats.data_ptr()) == 0, (name, lib.nsm_last_error())
            torch.cuda.synchronize(dev)
            assert pairs.tolist() == [0, 0, 0, 7, 7, 7, 7, 7], name
            assert lb.tolist() == [-1.0] * n + [5.0] * 4 and rb.tolist() == [-1.0] * m + [5.0] * 4, name
            assert stats.tolist() == [0, 0, 0, 0], f"{name}: a sweep ran"
    # no rows and no columns: refused like any null column, before anything is launched
    none = st.struct()
    none.n, none.codes = 0, None
    pairs = torch.full((3,), 7, dtype=torch.int64, device=dev)
    rb = torch.full((3,), 5.0, dtype=torch.float64, device=dev)
    assert lib.nsm_indel_raw_profile(none, jt.struct(), t, 3, 0, pairs.data_ptr(), rb.data_ptr(), rb.data_ptr(), 0, stream) == 10001
    torch.cuda.synchronize(dev)
    assert (pairs == 7).all() and (rb == 5.0).all()
