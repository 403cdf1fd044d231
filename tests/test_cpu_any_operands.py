"""No GPU needed.  Two things around the general kernels (csrc/any_grids.hip):

* the host encoders ``wide._any_strings`` / ``wide._any_sets`` on ``device="cpu"`` against a plain restatement of the
  operand layout, and their caps (refused at cap + 1, accepted at the cap);
* the grids of tests/support/any_operands.py through the oracle alone: tests/test_gpu_any_grids.py is only worth its GPU
  time if these grids have hits and misses where the kernels' edges are, and never ask the oracle for something the
  reference refuses (0 / 0, a zero-level item against one with levels).
"""
import math
import random

import numpy as np
import pytest

from support import any_operands as ao


# ------------------------------------------------------------------------------------------------------- the encoders
def _np(t):
    return t.numpy()


def test_any_strings_layout():
    from napkon_string_matching_amd import wide

    rng = random.Random(3)
    items = [[], ["ab", "", "cab"], ["c"], [], ["bbbb", "a"]]
    items.append(["".join(rng.choice("abc") for _ in range(wide.ANY_LEN))])  # exactly the cap
    lut = {"a": 0, "b": 1, "c": 2}
    strings, keep = wide._any_strings(items, lut, 3, "cpu")
    flat = [s for it in items for s in it]
    assert (strings.n_rows, strings.alphabet, strings.max_len) == (len(flat), 3, wide.ANY_LEN)
    want_offset = [0]
    for s in flat:
        want_offset.append(want_offset[-1] + len(s))
    assert _np(keep["offset"]).tolist() == want_offset and keep["offset"].dtype.itemsize == 8
    assert _np(keep["codes"]).dtype == np.uint16
    assert _np(keep["codes"]).tolist() == [lut[ch] for s in flat for ch in s]
    assert _np(keep["nlev"]).tolist() == [len(it) for it in items]
    first = _np(keep["first"]).tolist()
    for k, it in enumerate(items):  # item k owns rows first[k] .. first[k] + nlev[k]
        assert flat[first[k]: first[k] + len(it)] == list(it)
    assert _np(keep["orig"]).tolist() == list(range(len(items)))
    with pytest.raises(NotImplementedError):
        wide._any_strings([["a" * (wide.ANY_LEN + 1)]], lut, 3, "cpu")
    # nothing but zero-level items: buffers are still addressable
    strings, keep = wide._any_strings([[], []], lut, 1, "cpu")
    assert (strings.n_rows, strings.max_len) == (0, 0) and _np(keep["offset"]).tolist() == [0] and len(keep["codes"]) >= 1


def _first_levels(levels, vocab):
    out = {}
    for lv, level in enumerate(levels):
        for tok in level:
            out.setdefault(vocab[tok], lv)
    return out


def test_any_sets_nested_layout():
    from napkon_string_matching_amd import wide

    items = [[["x", "y"], ["x", "y", "q", "q"], ["q", "x", "y", "a"]], [], [["a"]], [["q", "b"], ["b", "q", "b"]]]
    vocab: dict = {}
    cat = np.array([1, 0, 1 << 63, 5], dtype=np.uint64)
    st, keep = wide._any_sets(items, vocab, 3, "cpu", cat, independent=False)
    assert (st.n, st.max_levels, st.max_ids) == (4, 3, 4) and not st.first
    assert sorted(vocab) == ["a", "b", "q", "x", "y"] and sorted(vocab.values()) == list(range(5))
    offset, ids, lv, plen = (_np(keep[k]) for k in ("offset", "ids", "lv", "plen"))
    assert lv.dtype == np.uint8 and ids.dtype == np.int32 and plen.shape == (4, 3)
    for k, levels in enumerate(items):
        want = _first_levels(levels, vocab)
        row = slice(offset[k], offset[k + 1])
        assert ids[row].tolist() == sorted(want)  # distinct, ascending: the kernel merges two such rows
        assert lv[row].tolist() == [want[v] for v in sorted(want)]
        assert plen[k].tolist() == [len(set(level)) for level in levels] + [0] * (3 - len(levels))
    assert _np(keep["nlev"]).tolist() == [3, 0, 1, 2]
    assert _np(keep["cat"]).view(np.uint64).tolist() == cat.tolist() and _np(keep["cat"])[2] < 0  # (uint64 seen as int64)
    # the other side shares the vocabulary: same token, same id
    st_r, keep_r = wide._any_sets([[["y", "new"]]], vocab, 3, "cpu", None, independent=False)
    assert _np(keep_r["ids"]).tolist() == sorted([vocab["y"], vocab["new"]]) and vocab["new"] == 5 and not st_r.cat


def test_any_sets_independent_layout():
    from napkon_string_matching_amd import wide

    items = [[["x", "y"], ["y", "q", "q"], []], [], [["a"]], [["q", "b"], ["b"]]]
    vocab: dict = {}
    st, keep = wide._any_sets(items, vocab, 3, "cpu", None, independent=True)
    assert st.first and not st.lv and not st.plen and st.max_ids == 2 and st.n == 4
    offset, ids, first, nlev = (_np(keep[k]) for k in ("offset", "ids", "first", "nlev"))
    assert nlev.tolist() == [3, 0, 1, 2] and first.tolist() == [0, 3, 3, 4] and len(offset) == 7
    row = 0
    for levels in items:
        for level in levels:  # one row per level, its distinct ids ascending
            assert ids[offset[row]: offset[row + 1]].tolist() == sorted({vocab[t] for t in level})
            row += 1
    assert row == len(offset) - 1


def test_caps_of_the_encoders(monkeypatch):
    from napkon_string_matching_amd import _lib, grid, wide

    assert (wide.ANY_LEN, wide.ANY_ALPHABET, wide.ANY_IDS) == (4096, 1023, 65535)
    at_cap = [list(range(wide.ANY_IDS))]
    beyond = [list(range(wide.ANY_IDS + 1))]
    for independent in (False, True):
        st, _keep = wide._any_sets([at_cap, [[1]]], {}, 1, "cpu", None, independent=independent)
        assert st.max_ids == wide.ANY_IDS
        with pytest.raises(NotImplementedError):
            wide._any_sets([[[1]], beyond], {}, 1, "cpu", None, independent=independent)
    # the alphabet is counted over both sides by the grid entry itself; everything after the check is stubbed out
    monkeypatch.setattr(_lib, "load", lambda: None)
    monkeypatch.setattr(grid, "run_grid", lambda launch, device, capacity, what: "launched")
    symbols = [chr(ao.BASE + v) for v in range(wide.ANY_ALPHABET + 1)]
    left, right = [["".join(symbols[:500])]], [["".join(symbols[500:wide.ANY_ALPHABET])]]
    assert wide.indel_any_grid(left, right, 0.5, device="cpu") == "launched"
    with pytest.raises(NotImplementedError):
        wide.indel_any_grid(left, [["".join(symbols[500:])]], 0.5, device="cpu")
    assert wide.indel_any_grid([["a" * wide.ANY_LEN]], [["a"]], 0.5, device="cpu") == "launched"
    with pytest.raises(NotImplementedError):
        wide.indel_any_grid([["a"]], [["a" * (wide.ANY_LEN + 1)]], 0.5, device="cpu")


# ------------------------------------------------------------------------------ the grids, through the oracle alone
def _longest(item):
    return max((len(lv) for lv in item), default=0)


@pytest.mark.parametrize("name", sorted(ao.CATALOGUE))
def test_grid_is_not_vacuous(name):
    g = ao.grid(name)
    all_hits = ao.oracle_all(g)  # (a 0 / 0 level pair or a visited zero-level mix would raise here)
    assert all_hits == sorted(all_hits, key=lambda h: (-h[0], h[1], h[2]))
    if g.mode == ao.CAT_NONE:
        assert len(all_hits) == g.pairs
    else:
        assert 0 < len(all_hits) < g.pairs, "the masks must allow some pairs and forbid others"
    for thr in g.mids:
        assert 0 < len(ao.oracle_at(all_hits, thr)) < g.pairs, f"threshold {thr}: both outcomes must occur"
    assert ao.oracle_at(all_hits, ao.ABOVE_ONE) == []
    # cutting the full list is what the oracle itself answers at that threshold
    assert ao.oracle_call(g, g.mids[0]) == ao.oracle_at(all_hits, g.mids[0])
    hits = ao.oracle_at(all_hits, g.mids[-1] if len(g.mids) < 3 else g.mids[1])
    if g.long_strings:
        assert any(_longest(g.left[i]) > 128 for _, i, _j in hits), "no hit whose pattern spans several chunks"
        assert any(_longest(g.right[j]) > 32 for _, _i, j in hits), "no hit whose text spans several carry words"
    if g.mixed_depths:
        assert any(len(g.left[i]) != len(g.right[j]) for _, i, j in hits)
        assert any(max(len(g.left[i]), len(g.right[j])) > 64 for _, i, j in hits)
    if g.kind == "jaccard":
        assert all(any(level for level in it) or not it for it in g.left)


@pytest.mark.parametrize("name", sorted(n for n in ao.CATALOGUE if ao.grid(n).probe))
def test_thresholds_sit_on_scores(name):
    g = ao.grid(name)
    all_hits = ao.oracle_all(g)
    picks = ao.probe_scores(all_hits)
    assert len(picks) >= 3
    lines = []
    for s in picks:
        at = [h for h in all_hits if h[0] == s]
        assert at, "a probed threshold is the score of some pair"
        assert ao.oracle_at(all_hits, math.nextafter(s, 2.0)) == [h for h in all_hits if h[0] > s]
        near = ao.near_neighbours(all_hits, s)
        lines.append(f"{name}: threshold {s!r}: {len(at)} pair(s) at it, "
                     + (f"{near} pair(s) within 1e-9 below" if near else "no neighbour within 1e-9 below in this grid"))
    print("\n".join(lines))  # (pytest -rP or -s shows it)
    thresholds = ao.thresholds(g, all_hits)
    assert thresholds[0] == 0.0 and thresholds.count(ao.ABOVE_ONE) == 1 and all(s in thresholds for s in picks)


def test_some_probed_grid_has_near_neighbours():
    """The slack of the pruning bounds (1e-9) is probed by pairs that close together, not by equality alone."""
    for name in ("fuzzy_depths", "jaccard_depths_deep", "jaccard_depths_64"):
        all_hits = ao.oracle_all(ao.grid(name))
        assert any(ao.near_neighbours(all_hits, s) for s in ao.probe_scores(all_hits)), name


def test_length_and_alphabet_edges_are_present():
    for name in ("fuzzy_length_edges", "fuzzy_length_edges_raw"):
        g = ao.grid(name)
        for side in (g.left, g.right):
            lengths = {len(lv) for it in side for lv in it}
            assert set(ao.PATTERN_EDGES + ao.TEXT_EDGES) <= lengths and 0 in lengths
        assert {4095, 4096} <= {len(lv) for it in g.left for lv in it} and {4095, 4096} <= {len(lv) for it in g.right for lv in it}
        assert (max(len(it) for it in g.left) == 1) == g.raw
        tile = g.right[:64]  # one wave: texts of very different lengths side by side
        assert min(_longest(it) for it in tile) <= 32 and max(_longest(it) for it in tile) >= 4095
    for alphabet in (1, 255, 256, 1023):
        g = ao.grid(f"fuzzy_alphabet_{alphabet}")
        assert len({v for side in (g.left, g.right) for it in side for lv in it for v in lv}) == alphabet


def test_depth_grids_mix_depths_in_one_tile():
    from napkon_string_matching_amd import wide

    for name, depths in (("fuzzy_depths", ao.DEPTHS), ("jaccard_depths_deep", ao.DEPTHS),
                         ("jaccard_depths_64", tuple(d for d in ao.DEPTHS if d <= 64))):
        g = ao.grid(name)
        assert set(depths) <= {len(it) for it in g.right[:64]} and set(depths) <= {len(it) for it in g.left}
        pairs = {(len(g.left[i]), len(g.right[j])) for i in range(len(g.left)) for j in range(len(g.right))}
        assert (1, max(depths)) in pairs and (max(depths), 1) in pairs
        if g.kind == "jaccard":
            assert all(wide._nested(it) for it in g.left + g.right)
            assert (max(len(it) for it in g.left + g.right) > wide.FAST_LEVELS) == (g.layout == "independent")


def test_nested_jaccard_grid_has_every_entry_level_pair():
    from napkon_string_matching_amd import wide

    g = ao.grid("jaccard_nested")
    assert all(wide._nested(it) for it in g.left + g.right) and max(len(it) for it in g.left + g.right) == 64
    assert {(p, q) for p in ao.ENTRY_LEVELS for q in ao.ENTRY_LEVELS} <= ao.entry_level_pairs(g)
    sizes_l = [len(set(it[-1])) for it in g.left]
    sizes_r = [len(set(it[-1])) for it in g.right]
    assert min(s for s in sizes_l if s >= 65) == 65 and max(sizes_l) == 3000 and min(sizes_r) <= 3 and max(sizes_r) >= 2990
    assert any(len(lv) != len(set(lv)) for it in g.left + g.right for lv in it), "a token repeated inside a level"


def test_independent_jaccard_grid_is_irregular():
    from napkon_string_matching_amd import wide

    g = ao.grid("jaccard_independent")
    assert any(not wide._nested(it) for it in g.left) and any(not wide._nested(it) for it in g.right)
    assert all(lv for it in g.left for lv in it), "left levels are never empty: no step can be empty on both sides"
    assert any(not lv for it in g.right for lv in it[1:] or it)
    assert max(len(it) for it in g.left + g.right) > 64
    widths = {len(set(lv)) for it in g.left + g.right for lv in it}
    assert max(widths) >= 65 and min(widths - {0}) == 1


def test_geometry_grids():
    for kind in ("indel", "jaccard"):
        assert [len(ao.grid(f"tails_{kind}_{n}").right) for n in ao.RIGHT_TAILS] == [1, 63, 64, 65, 129]
        g = ao.grid(f"many_rows_{kind}")
        rows = ao.rows_per_chunk(len(g.left), len(g.right))
        assert rows >= 2 and len(g.left) % rows != 0
        # the last block's single row has a hit, and so has a row that is not the first of its block
        hits = ao.oracle_at(ao.oracle_all(g), g.mids[0])
        assert any(i == len(g.left) - 1 for _, i, _j in hits) and any(i % rows for _, i, _j in hits)
    assert ao.rows_per_chunk(99, 150) == 1  # (what every grid of tests/test_gpu_wide.py has)


def test_masked_grids_use_bit_63_and_pair_empty_masks():
    top = np.uint64(1) << np.uint64(63)
    for name in ao.CATALOGUE:
        g = ao.grid(name)
        if g.mode == ao.CAT_NONE:
            continue
        assert (g.cat_l & top).any() and (g.cat_r & top).any(), name
        pairs = {(i, j) for _, i, j in ao.oracle_all(g)}
        both_empty = {(i, j) for i in np.flatnonzero(g.cat_l == 0) for j in np.flatnonzero(g.cat_r == 0)}
        if name.startswith("categories_"):
            assert both_empty, name
            assert (both_empty <= pairs) if g.mode == ao.CAT_INTERSECT_OR_BOTH_EMPTY else not (both_empty & pairs), name
            only_top = {(i, j) for i in range(len(g.left)) for j in range(len(g.right))
                        if g.cat_l[i] & g.cat_r[j] == top}
            assert only_top and only_top <= pairs, name
        else:  # zero-level items and items with levels never meet
            assert any(not it for it in g.left) and any(not it for it in g.right)
            assert all(bool(g.left[i]) == bool(g.right[j]) for i, j in pairs), name
            assert any(not g.left[i] for i, _j in pairs) and any(g.left[i] for i, _j in pairs)


@pytest.mark.parametrize("name", sorted(ao.ZERO_ONLY))
def test_zero_level_grids(name):
    g = ao.grid(name)
    all_hits = ao.oracle_all(g)
    assert all_hits and all(h[0] == 0.0 for h in all_hits)
    assert (len(all_hits) == g.pairs) == (g.mode == ao.CAT_NONE)
    assert ao.oracle_call(g, 5e-324) == []


def test_cap_pair_scores():
    left, right, want = ao.jaccard_cap_pair()
    assert len(left) == 1 and len(right) == 2 and len(set(left[0][-1])) == 65535 and len(set(right[1][-1])) == 65534
    assert want[0] == (0.875, 0, 0) and want[1][1:] == (0, 1)
    sizes = [(30000, 29999), (50000, 49999), (65535, 65534)]
    score = (sizes[1][1] / sizes[1][0]) * 0.5 + (sizes[2][1] / sizes[2][0]) * 0.25 + (sizes[2][1] / sizes[2][0]) * 0.125
    assert want[1][0] == score
