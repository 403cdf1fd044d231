"""The guard-band arena of tests/support/arena.py on ``device="cpu"``, and the premises of
tests/test_gpu_memory_contract.py from the oracle alone (no GPU).

The GPU file only pins the extents of include/nsm_hip*.h if (1) the arena reports a stray byte wherever it lands outside a
region, and says where, and (2) its cases are worth running: more oracle hits than every "too small" capacity, caller ids
with gaps, top-k rows of every fill -- for the entries of nsm_hip.h by the oracle, for the nsm_set_* / nsm_edit_* entries
under every measure and metric by the definitions.
"""
import numpy as np
import pytest
import torch

from support import any_operands as ao
from support import arena as ar
from support import memory_cases as mc
from support import threshold_probes as tp

SIZES = (("a", 16, torch.float64, (1, 2)), ("b", 8, torch.int64, None), ("c", 1000, torch.uint8, None),
         ("d", 4 * 37, torch.int32, (37,)), ("last", 16 * 65, torch.float64, (65, 2)))


def _arena(seed=3):
    a = ar.Arena(64 * 1024, "cpu", seed)
    views = {name: a.carve(name, nbytes, dtype, shape) for name, nbytes, dtype, shape in SIZES}
    return a, views


def _nearest(a, offset):
    """(distance, side, name) of the region edge nearest to a byte outside every region, computed apart from Arena._where."""
    best = None
    for name, (start, end) in a.regions.items():
        assert not start <= offset < end
        cand = (start - offset, "before the start of", name) if offset < start else (offset - end + 1, "behind the end of", name)
        if best is None or cand[0] < best[0]:
            best = cand
    return best


def test_carve_gives_exact_aligned_views_with_guards():
    a, views = _arena()
    assert not (a.host == 0).any()  # the poison has no zero byte: "left as it was" differs from "zeroed"
    assert not (a.host == a.host[0]).all()
    edges = sorted(a.regions.values())
    for (name, nbytes, dtype, shape), v in zip(SIZES, views.values()):
        start, end = a.regions[name]
        assert end - start == nbytes == v.numel() * v.element_size() and v.dtype == dtype
        assert v.data_ptr() == a.ptr(name) == a.base + start and a.ptr(name) % ar.ALIGN == 0
        assert shape is None or tuple(v.shape) == shape
        assert v.contiguous().view(torch.uint8).numpy().tobytes() == a.host[start:end].tobytes()  # the view IS the poison
    assert edges[0][0] >= ar.GUARD and a.nbytes - edges[-1][1] >= ar.GUARD
    for (_, end), (start, _) in zip(edges, edges[1:]):
        assert start - end >= ar.GUARD
    a.check()
    for name in a.regions:
        a.unchanged(name)
    with pytest.raises(ValueError):
        a.carve("a", 8)
    with pytest.raises(ValueError):
        a.carve("odd", 12, torch.float64)
    with pytest.raises(ValueError):
        ar.Arena(3 * ar.GUARD, "cpu", 1).carve("big", 2 * ar.GUARD)  # no room for the guard behind it


@pytest.mark.parametrize("name", [s[0] for s in SIZES])
@pytest.mark.parametrize("where", ["just before", "just behind", "4095 behind"])
def test_a_stray_byte_outside_a_region_is_reported(name, where):
    a, _ = _arena()
    start, end = a.regions[name]
    offset = {"just before": start - 1, "just behind": end, "4095 behind": end + 4094}[where]
    a.buf[offset] ^= 0x5A
    dist, side, near = _nearest(a, offset)
    if where != "4095 behind":
        assert (dist, near) == (1, name)
    elif name == "last":
        assert (dist, side, near) == (4095, "behind the end of", "last")
    with pytest.raises(ar.ArenaError) as err:
        a.check()
    text = str(err.value)
    assert f"arena offsets {offset} .. {offset}" in text and f"first {dist} byte(s) {side} {near!r}" in text, text
    for region in a.regions:  # (no region itself changed)
        a.unchanged(region)


def test_a_run_of_stray_bytes_reports_both_ends():
    a, _ = _arena()
    end = a.regions["c"][1]
    a.buf[end: end + 16] = 0
    with pytest.raises(ar.ArenaError) as err:
        a.check()
    assert f"16 byte(s) changed, arena offsets {end} .. {end + 15}: first 1 byte(s) behind the end of 'c', last 16 byte(s) " \
           f"behind the end of 'c'" in str(err.value)


def test_a_write_inside_a_region_is_for_unchanged_to_see():
    a, views = _arena()
    views["d"][5] += 1
    a.check()
    with pytest.raises(ar.ArenaError) as err:
        a.unchanged("d")
    assert "byte 20 of 'd'" in str(err.value)
    a.unchanged("c")
    # fill and zero move the host copy along: what they wrote is the new "as it was"
    a.fill("b", np.array([7], dtype=np.int64))
    a.unchanged("b")
    assert views["b"].tolist() == [7] and a.poison("b", np.int64).tolist() == [7]
    a.zero("b")
    a.unchanged("b")
    assert views["b"].tolist() == [0]
    with pytest.raises(ValueError):
        a.fill("b", np.zeros(3, dtype=np.int64))
    a.check()


def test_rehome_keeps_dtypes_shapes_and_contents():
    import ctypes

    from napkon_string_matching_amd import _lib, tables

    g = tp.grid("levels_jaccard-cat1_partition")
    vocabulary = tables.Vocabulary()
    st = tables.SetTable.from_levels(g.right, "right", "cpu", vocabulary, width=g.size, categories=g.cat_r, category_mode=g.mode,
                                     partition=True)
    lt, rt = tables.encode_strings(["abc", "", "abd" * 20], ["abc", "xyz"], "cpu")
    items = [["ab", "ab cd"], ["x"], ["ab", "ab ef", "ab ef gh"]]
    li, ls, _, _ = tables.encode_level_strings(items, items, "cpu", np.array([1, 2, 3], np.uint64), np.array([1, 2, 3], np.uint64),
                                               _lib.CAT_INTERSECT, partition=True)
    keep = dict(codes=torch.arange(10, dtype=torch.int16), offset=torch.tensor([0, 4, 10]), note="not a tensor")
    anys = _lib.NsmAnyStrings(keep["codes"].data_ptr(), keep["offset"].data_ptr(), 2, 77, 6)
    a = ar.Arena(ar.table_bytes(st, lt, lt, li, ls, (anys, keep)) + 2 * ar.GUARD, "cpu", 9)
    for k, table in enumerate((st, lt, li, ls)):
        moved = ar.rehome(table, a, f"t{k}")
        assert type(moved) is type(table)
        before, after = ar._tensors_of(table), ar._tensors_of(moved)
        assert list(before) == list(after) and len(before) >= 4
        for col in before:
            assert after[col].dtype == before[col].dtype and after[col].shape == before[col].shape, col
            assert torch.equal(after[col], before[col]), col
            start, end = a.regions[f"t{k}.{col}"]
            assert end - start == before[col].numel() * before[col].element_size()
            assert after[col].numel() == 0 or after[col].data_ptr() == a.base + start
        assert (moved.n, getattr(moved, "width", None), getattr(moved, "stride", None)) == \
               (table.n, getattr(table, "width", None), getattr(table, "stride", None))
        assert ctypes.sizeof(moved.struct()) == ctypes.sizeof(table.struct())
    assert st.seg is not None and li.seg is not None and lt.hist16 is not None  # (the optional columns were there to move)
    moved, kept = ar.rehome((anys, keep), a, "any")
    assert (moved.codes, moved.offset) == (a.ptr("any.codes"), a.ptr("any.offset")) and (moved.n_rows, moved.alphabet, moved.max_len) == (2, 77, 6)
    assert torch.equal(kept["codes"], keep["codes"]) and kept["note"] == "not a tensor" and anys.codes == keep["codes"].data_ptr()
    a.check()
    for name in a.regions:
        a.unchanged(name)
    auto = ar.rehome(lt, a)
    assert torch.equal(auto.codes, lt.codes) and "StrTable0.codes" in a.regions
    assert ar.input_names(a, "t0", "any") == [n for n in a.regions if n.startswith(("t0.", "any."))]


# ------------------------------------------------------------------------------------------- premises of the GPU cases
@pytest.mark.parametrize("name", tp.EVERY)
def test_threshold_grids_overflow_every_small_capacity(name):
    thr, want = mc.hit_case(name)
    assert len(want) > max(mc.SMALL_CAPACITIES) + 1 and len(set(want)) == len(want)
    assert mc.capacities(len(want)) == sorted(set(mc.capacities(len(want))))  # eight different sizes
    assert want == tp.oracle_call(tp.grid(name), thr)


@pytest.mark.parametrize("name", mc.ANY_GRIDS)
def test_any_grids_overflow_every_small_capacity(name):
    thr, want = mc.any_case(name)
    assert len(want) > max(mc.SMALL_CAPACITIES) + 1 and want == ao.oracle_call(ao.grid(name), thr)


@pytest.mark.parametrize("entry", mc.FLOOR_GRIDS)
def test_floor_grids_overflow_every_small_capacity(entry):
    g = tp.grid(mc.FLOOR_GRIDS[entry])
    thr, lf, rf, want = mc.floor_case(g.name)
    at_thr = tp.expectation(tp.all_scores(g), thr)
    assert max(mc.SMALL_CAPACITIES) + 1 < len(want) < len(at_thr)  # the floors admit some pairs and refuse others
    assert np.isnan(lf).any() and not any(i == mc.caller_id(3) for _, i, _ in want)  # (item 3: a NaN floor admits nothing)
    assert g.partition is False


@pytest.mark.parametrize("entry", mc.PROFILE_GRIDS)
def test_profile_case_has_gaps_and_items_without_a_hit(entry):
    g = tp.grid(mc.PROFILE_GRIDS[entry])
    ladder, pairs, left, right = mc.profile_case(g.name)
    assert len(ladder) == 3 and ladder == sorted(ladder) and pairs[0] > pairs[1] > pairs[2] > 0
    for ids, n in ((left, len(g.left)), (right, len(g.right))):
        assert sorted(ids) == [3 * k + 2 for k in range(n)]  # gaps: ids 0, 1, 3, 4, 6 .. name no item
        assert any(v == -1.0 for v in ids.values()) and any(v > 0 for v in ids.values())
    assert pairs[0] == len(tp.oracle_call(g, ladder[0]))


@pytest.mark.parametrize("entry", mc.TOP_K_GRIDS)
def test_top_k_case_has_rows_of_every_fill(entry):
    g = tp.grid(mc.TOP_K_GRIDS[entry])
    case = mc.top_k_case(g.name)
    assert case is not None, "no probe threshold leaves empty, short and long rows"
    thr, allowed, banned = case
    count = mc.row_counts(allowed, len(g.left))
    assert 0 in count and any(0 < c < 3 for c in count) and any(c > 3 for c in count)
    assert max(mc.TOP_K) > len(g.right) and (banned is not None) == (not g.raw)
    if banned:
        assert len(allowed) < len(tp.expectation(tp.all_scores(g), thr))  # the blacklist removes hits


@pytest.mark.parametrize("entry", mc.PAIRS_GRIDS)
def test_pair_lists_hold_duplicates_and_ids_without_a_row(entry):
    g = tp.grid(mc.PAIRS_GRIDS[entry])
    assert g.mode == tp.CAT_NONE
    for n_pairs in mc.PAIR_COUNTS:
        pairs = mc.pair_list(g, n_pairs)
        scores = mc.pair_scores(g, pairs)
        assert len(pairs) == n_pairs == len(scores)
        if n_pairs >= 63:
            assert len(set(pairs)) < n_pairs                                                   # duplicates
            assert any(not (0 <= i < len(g.left) and 0 <= j < len(g.right)) for i, j in pairs)  # ids outside the maps
            assert any(i in mc.UNMAPPED_LEFT or j in mc.UNMAPPED_RIGHT for i, j in pairs)       # ids whose row is -1
            assert sum(s >= 0 for s in scores) > n_pairs // 2 and any(s == -1.0 for s in scores)


# ------------------------------------------------------------------------- premises of the additive headers' cases
def test_codes_are_the_headers():
    from napkon_string_matching_amd import _lib

    assert {v: mc.CODE[v] for v in mc.MEASURES} == {v: c for v, c in _lib.MEASURES.items() if c} and len(mc.MEASURES) == 3
    assert {v: mc.CODE[v] for v in mc.METRICS} == {v: c for v, c in _lib.METRICS.items() if c} and len(mc.METRICS) == 2
    every = mc.additive(list(mc.FLOOR_GRIDS) + list(mc.TOP_K_GRIDS) + list(mc.PROFILE_GRIDS) + list(mc.PAIRS_GRIDS))
    assert {e for e, _, _ in every} == set(_lib.MEASURE_EXPORTS) | set(_lib.EDIT_EXPORTS) and len({e for e, _, _ in every}) == 18
    assert all(e.startswith("nsm_set_") == (v in mc.MEASURES) for e, _, v in every)


def test_both_distances_in_one_pass_are_the_two_row_programme():
    import random

    from support import edit_distance as ed

    rng = random.Random(7)
    for alphabet in ("ab", "abcdefgh"):
        for _ in range(12):
            a = "".join(rng.choice(alphabet) for _ in range(rng.choice((0, 1, 5, 9, 17))))
            rights = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 21))) for _ in range(9)] + ["", a, a + a]
            d, w = ed.both_many(a, rights)
            assert d == [ed.distance(a, b) for b in rights] and w == [ed.within(a, b) for b in rights], (a, rights)
    assert ed.both_many([1, 2, 3], [(1, 2, 3, 4), (), (9, 1, 2, 3, 9)]) == ([1, 3, 2], [0, 3, 0])  # (code units as ints)
    # the yardstick of a levels grid is compare_terms with that definition: two pairs by hand from the two-row programme
    g = tp.grid("levels_indel_one_word-cat2_lanes")
    by_pair = {(i, j): s for s, i, j in mc.edit_scores(g, "edit_within")}
    from oracle.compare import compare_terms

    for (i, j) in list(by_pair)[:: max(1, len(by_pair) // 5)][:5]:
        f = lambda a, b: ed.score("edit_within", len(a), len(b), ed.within(tp.text(a), tp.text(b)))
        assert by_pair[i, j] == compare_terms(g.left[i], g.right[j], f)


@pytest.mark.parametrize("entry,sibling,variant", mc.additive(mc.FLOOR_GRIDS))
def test_additive_floor_grids_overflow_every_small_capacity(entry, sibling, variant):
    name = mc.FLOOR_GRIDS[sibling]
    g = mc.view(name, variant)
    thr, lf, rf, want = mc.floor_case(name, variant)
    at_thr = tp.expectation(mc.scores(g, variant), thr)
    assert max(mc.SMALL_CAPACITIES) + 1 < len(want) < len(at_thr) < g.pairs  # more than 65 hits, fewer than all pairs
    assert len(set(want)) == len(want) and mc.capacities(len(want)) == sorted(set(mc.capacities(len(want))))
    assert np.isnan(lf).any() and not any(i == mc.caller_id(3) for _, i, _ in want)  # (item 3: a NaN floor admits nothing)
    assert len(lf) == mc.caller_id(len(g.left) - 1) + 1 and len(rf) == mc.caller_id(len(g.right) - 1) + 1
    assert g.partition is False and (variant != "smaller" or not g.raw or all(g.right))


@pytest.mark.parametrize("entry,sibling,variant", mc.additive(mc.TOP_K_GRIDS))
def test_additive_top_k_cases_have_rows_of_every_fill(entry, sibling, variant):
    name = mc.grid_name(mc.TOP_K_GRIDS, sibling, variant)
    g = mc.view(name, variant)
    case = mc.top_k_case(name, variant)
    assert case is not None, "no probe threshold leaves empty, short and long rows"
    thr, allowed, banned = case
    count = mc.row_counts(allowed, len(g.left))
    assert 0 in count and any(0 < c < 3 for c in count) and any(c > 3 for c in count)
    assert max(mc.TOP_K) > len(g.right) and (banned is not None) == (not g.raw)
    at_thr = tp.expectation(mc.scores(g, variant), thr)
    assert len(allowed) < g.pairs and (not banned or len(allowed) < len(at_thr))  # the blacklist removes hits
    if variant == "smaller" and g.raw:  # why this variant has a grid of its own
        for other in ("raw_jaccard_16", "raw_jaccard_32"):
            assert mc.top_k_case(other, variant) is None


@pytest.mark.parametrize("entry,sibling,variant", mc.additive(mc.PROFILE_GRIDS))
def test_additive_profile_cases_have_gaps(entry, sibling, variant):
    name = mc.grid_name(mc.PROFILE_GRIDS, sibling, variant)
    g = mc.view(name, variant)
    ladder, pairs, left, right = mc.profile_case(name, variant)
    assert len(ladder) == 3 and ladder == sorted(ladder) and g.pairs > pairs[0] > pairs[1] > pairs[2] > 0
    for ids, n in ((left, len(g.left)), (right, len(g.right))):
        assert sorted(ids) == [3 * k + 2 for k in range(n)] and any(v > 0 for v in ids.values())
    assert any(v == -1.0 for v in left.values()) or any(v == -1.0 for v in right.values())  # items without a hit
    assert pairs[0] == len(tp.expectation(mc.scores(g, variant), ladder[0]))


@pytest.mark.parametrize("entry,sibling,variant", mc.additive(mc.PAIRS_GRIDS))
def test_additive_pair_lists_score_most_pairs(entry, sibling, variant):
    g = tp.grid(mc.PAIRS_GRIDS[sibling])
    for n_pairs in mc.PAIR_COUNTS[1:]:
        pairs = mc.pair_list(g, n_pairs)
        scores = mc.pair_scores(g, pairs, variant)
        assert len(scores) == n_pairs and sum(s >= 0 for s in scores) > n_pairs // 2 and any(s == -1.0 for s in scores)
        assert all(s == -1.0 for s, (i, j) in zip(scores, pairs) if i in mc.UNMAPPED_LEFT or not 0 <= j < len(g.right))
    if variant == "smaller" and g.raw:  # an empty right row: the measure divides by zero, the entry writes -1.0
        empty = [j for j, row in enumerate(g.right) if not row and j not in mc.UNMAPPED_RIGHT]
        listed = {p for n in mc.PAIR_COUNTS for p in mc.pair_list(g, n)}
        assert any(j in empty and 0 <= i < len(g.left) and i not in mc.UNMAPPED_LEFT for i, j in listed)


def test_support_case_is_small_and_peels():
    from napkon_string_matching_amd import grid
    from support import edge_support as es

    lists, nodes, min_score = mc.support_case()
    sizes = [len(hits) for hits, _, _ in lists]
    assert 0 in sizes and len(lists) == 5 and 150 < sum(sizes) <= 320
    counting, one = grid.truss_of_hits(lists, nodes, 0, min_score)
    peeled, rounds = grid.truss_of_hits(lists, nodes, 1, min_score)
    assert one == 1 and rounds >= 2
    flat = np.concatenate(peeled)
    assert (flat == -1).any() and (flat == -2).any() and (flat >= 1).any() and (np.concatenate(counting) == 0).any()
    records, distinct = es.edge_counts(lists, nodes, min_score)
    assert distinct < records < sum(sizes)  # duplicates; records that are no edge
    assert any(np.isnan(hits.score).any() for hits, _, _ in lists)
    for side in ("i", "j", "negative"):
        bad = mc.support_case_with_bad_id(lists, nodes, side)
        hits, lb, rb = bad[-1]
        out = (hits.i < 0) | (hits.i >= nodes - lb) | (hits.j < 0) | (hits.j >= nodes - rb)
        assert out.sum() == 1 and hits.score[out][0] < min_score and mc.support_records(hits).shape == (len(hits), 2)


def test_sort_records_are_distinct_and_tie_on_scores():
    for n, cap in mc.SORT_SIZES:
        rec = mc.sort_records(cap, 5, 1000)
        assert rec.shape == (cap, 2) and cap > n
        ij = rec.view(np.int32).reshape(-1, 4)[:, 2:]
        assert len({(a, b) for a, b in ij.tolist()}) == cap and len(set(rec[:, 0].tolist())) <= 50
        want = mc.sorted_records(rec[:n])
        keys = list(zip((-want[:, 0]).tolist(), *want.view(np.int32).reshape(-1, 4)[:, 2:].T.tolist()))
        assert keys == sorted(keys)
