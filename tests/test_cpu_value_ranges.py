"""The inputs of tests/test_gpu_value_ranges.py through the oracle and plain Python alone (no GPU): can they see what they
are for?

* Part A.  The levels Jaccard kernels compare ids modulo 2^26 (include/nsm_hip.h: ``NSM_LEVELS_ID_LIMIT``).  A Python model
  of that compare must answer differently from the oracle on the IMAGES grids at every threshold the GPU file uses, with
  every planted alias pair among the differences: the inputs can see the defect, and the model records what a library
  without the id limit answers.  The Python encoders refuse such tables on the host path, with the words of the builder.
* Part B.  At strides 256 and 512 the grids hold hits that a histogram whose counts WRAP would prune, and none that the
  saturating column prunes: the L1 form of the bound stays valid under clipping.  Pure runs check the oracle against the
  closed form.
* Part C.  The numpy encoders against the per-row restatement of the header, on the inputs they accept.
"""
import numpy as np
import pytest

from support import threshold_probes as tp
from support import value_ranges as vr

A_GRIDS = vr.JACCARD_RAW + vr.JACCARD_RAW_SMALL + vr.LEVELS_LOW + vr.LEVELS_SMALL + vr.LEVELS_IMAGES


# ----------------------------------------------------------------------------------------------------------- Part A
def test_id_pools():
    assert all(0 <= v < vr.P26 for v in vr.LOW) and len(set(vr.LOW)) == len(vr.LOW)
    assert len({vr.residue(v) for v in vr.LOW}) == len(vr.LOW)  # nothing inside LOW is congruent: LOW tables are exact
    assert all(vr.P26 <= v <= vr.INT32_MAX and vr.residue(v) in vr.LOW for v in vr.IMAGES) and vr.INT32_MAX in vr.IMAGES
    assert all(v < vr.GLOBAL_INDEX_LIMIT for v in vr.SMALL) and len(vr.SMALL) >= 64
    assert 64 * (max(vr.SMALL_LEVELS) + 1) <= 1 << 23 and len(vr.SMALL_LEVELS) >= 64  # (tables.MAX_INDEX_VOCAB keys)
    # the two largest allowed ids shift to the bit patterns of the padding
    shifted = lambda v: (v << 6) & 0xFFFFFFFF
    assert shifted(vr.P26 - 1) == shifted(-1) and shifted(vr.P26 - 2) == shifted(-2)
    # the arithmetic of the issue: true Jaccard 0.0, the shifted compare says 1.0
    a, b = [5, 63, 1 << 16], [5 + vr.P26, 63 + 2 * vr.P26, (1 << 16) + 31 * vr.P26]
    assert vr.jaccard(a, b) == 0.0 and vr.jaccard([shifted(v) for v in a], [shifted(v) for v in b]) == 1.0


@pytest.mark.parametrize("name", A_GRIDS)
def test_set_scorer_equals_the_oracle(name):
    """The oracle on the raw integers against the ten-line ``set`` scorer: same pairs, same order, same doubles; the shapes
    and the hits the GPU file counts on."""
    g = vr.grid(name)
    assert (len(g.left), len(g.right)) == (vr.N_LEFT, vr.N_RIGHT)
    rows = [r if g.raw else r[-1] for r in g.left + g.right]
    assert all(1 <= len(r) <= g.size and len(set(r)) == len(r) for r in rows) and max(map(len, rows)) > g.size // 2
    if not g.raw:
        assert {len(it) for it in g.left} == {1, 2, 3, 4} == {len(it) for it in g.right}
        assert all(set(a) <= set(b) and a == b[: len(a)] for it in g.left + g.right for a, b in zip(it, it[1:]))
    want = tp.all_scores(g)
    assert want == vr.set_scores(g)
    for thr in vr.JACCARD_THRESHOLDS:
        hits = tp.expectation(want, thr)
        # a levels score is below 1.0 (its weights sum to 1 - 2^-steps): the one empty list
        assert (len(hits) == 0) == (thr == 1.0 and not g.raw), (name, thr)
        assert hits == tp.oracle_call(g, thr) if thr in (0.3, 1.0) else True


@pytest.mark.parametrize("name", vr.JACCARD_RAW + vr.LEVELS_IMAGES)
def test_alias_pairs(name):
    g = vr.grid(name)
    alias = vr.alias_pairs(g)
    assert len(alias) >= 20
    scores = {(i, j): s for s, i, j in vr.set_scores(g)} if g.cat_l is None else None
    for i, j in alias:
        a, b = (g.left[i], g.right[j]) if g.raw else (g.left[i][-1], g.right[j][-1])
        assert not set(a) & set(b) and {vr.residue(v) for v in a} == {vr.residue(v) for v in b}
        assert scores is None or scores[(i, j)] == 0.0
    if g.raw:
        sizes = {len(g.left[i]) for i, _ in alias}
        assert {1, len(vr.CLASSES)} <= sizes and any(vr.INT32_MAX in g.right[j] or vr.INT32_MAX in g.left[i] for i, j in alias)


@pytest.mark.parametrize("name", vr.LEVELS_IMAGES)
def test_shifted_compare_model_differs_on_the_images_grids(name):
    """What a library without the id limit answers on these inputs: every alias pair scored as if its ids were equal."""
    g = vr.grid(name)
    true, model = tp.all_scores(g), vr.shifted_compare_scores(g)
    model_score = {(i, j): s for s, i, j in model}
    alias = vr.alias_pairs(g)
    every_level = [p for p in alias if model_score[p] == vr.levels_score(g.left[p[0]], g.left[p[0]], vr.jaccard)]
    last_only = [p for p in alias if p not in every_level]
    assert len(every_level) >= 8 and len(last_only) >= 8 and all(0.0 < model_score[p] for p in alias)
    assert {len(g.left[i]) for i, _ in every_level} == {1, 2, 3, 4}
    for i, j in last_only:  # before the last level the two items share nothing, even modulo 2^26
        assert len(g.left[i]) >= 3
        assert all(not {vr.residue(v) for v in a} & {vr.residue(v) for v in b} for a, b in zip(g.left[i][:-1], g.right[j][:-1]))
    seen = set()
    for thr in vr.JACCARD_THRESHOLDS:
        a, b = set(tp.expectation(true, thr)), set(tp.expectation(model, thr))
        if thr == 1.0:  # no levels score reaches 1.0 (the weights sum to 1 - 2^-steps): both lists are empty there
            assert not a and not b
            continue
        assert a != b, f"{name}: the shifted compare answers the oracle's list at {thr!r}"
        wrong = {(i, j) for _, i, j in a ^ b}
        assert all(p in wrong for p in alias if model_score[p] >= thr)  # an alias pair: 0.0 in truth, a hit in the model
        seen |= wrong
    assert set(alias) <= seen


def _nested(g, side, device="cpu", **kw):
    from napkon_string_matching_amd import tables

    items, cat = (g.left, g.cat_l) if side == "left" else (g.right, g.cat_r)
    ids, plen, nlev = vr.nested_arrays(items, g.size)
    return tables.SetTable.from_nested_arrays(ids, plen, nlev, side, device, categories=cat, width=g.size,
                                              category_mode=g.mode, partition=g.partition, **kw)


def test_host_encoder_refuses_level_ids_at_the_limit():
    from napkon_string_matching_amd import tables

    assert tables.LEVELS_ID_LIMIT == vr.LEVELS_ID_LIMIT
    for name in vr.LEVELS_IMAGES:
        for side in ("left", "right"):
            with pytest.raises(ValueError, match=r"2\^26 \(NSM_LEVELS_ID_LIMIT\)"):
                _nested(vr.grid(name), side)
    one = lambda v: tables.SetTable.from_nested_arrays(np.array([[7, v]], np.int32), np.array([[1, 2]], np.uint8), np.array([2]),
                                                        "right", "cpu", width=16)
    with pytest.raises(ValueError, match=r"2\^26"):
        one(vr.LEVELS_ID_LIMIT)
    assert one(vr.LEVELS_ID_LIMIT - 1).ids[0, :2].tolist() == [7, vr.LEVELS_ID_LIMIT - 1]
    # RAW tables compare whole ids: any int32 >= 0
    raw = tables.SetTable.from_padded(np.array([[vr.INT32_MAX, 5, vr.P26]], np.int32), "right", "cpu", width=16)
    assert raw.ids[0, :4].tolist() == [5, vr.P26, vr.INT32_MAX, -2] and raw.post is None
    t = _nested(vr.grid(vr.LEVELS_LOW[0]), "right")
    assert int(t.ids.max()) == vr.P26 - 1 and t.post is None  # (2^26 keys: no global index by default)


def test_host_encoder_refuses_a_global_index_beyond_its_keys():
    from napkon_string_matching_amd import tables

    ids = np.array([[3, vr.GLOBAL_INDEX_LIMIT, -1]], np.int32)
    with pytest.raises(ValueError, match=r"2\^25"):
        tables.SetTable.from_padded(ids, "right", "cpu", width=16, index=True)
    assert tables.SetTable.from_padded(ids, "right", "cpu", width=16).post is None  # index=None: left out
    with pytest.raises(ValueError, match=r"2\^25"):
        tables.SetTable.from_nested_arrays(ids, np.array([[1, 2]], np.uint8), np.array([2]), "right", "cpu", width=16, index=True)
    small = tables.SetTable.from_padded(np.array([[3, 1 << 16, -1]], np.int32), "right", "cpu", width=16, index=True)
    assert small.post is not None and small.vocab == (1 << 16) + 1


# ----------------------------------------------------------------------------------------------------------- Part B
@pytest.mark.parametrize("name", vr.RAW_STRINGS)
def test_low_entropy_strings(name):
    """Shapes; pure runs against the closed form LCS = min(m, n); every threshold has hits; the saturating histogram never
    prunes a hit; at strides >= 256 at least 30 hits sit where a wrapping histogram prunes."""
    g = vr.grid(name)
    alphabet = vr.alphabet_of(g)
    a = vr.SYMBOLS[alphabet][0]
    assert len(g.left) == vr.STR_LEFT and len(g.right) == vr.STR_RIGHT
    assert all(len(s) <= g.size and all(u < alphabet for u in s) for s in g.left + g.right)
    assert max(map(len, g.left)) == g.size == max(map(len, g.right)) and [] in g.left and [] in g.right
    want = tp.all_scores(g)
    assert len(want) == g.pairs
    runs = 0
    for s, i, j in want:
        x, y = g.left[i], g.right[j]
        if x and y and set(x) == {a} == set(y):
            assert s == vr.indel_ratio(len(x), len(y), min(len(x), len(y))), (name, len(x), len(y))
            runs += 1
        assert vr.histogram_bound(x, y, lambda v: min(v, 255)) >= s  # clipping only weakens the bound
    assert runs >= 40
    for thr in vr.INDEL_THRESHOLDS:
        assert len(tp.expectation(want, thr)) > 0
    # runs of m and 2 m units: 2/3 in exact arithmetic, within an ulp of it through the documented formula
    thirds = [s for s, i, j in want if g.left[i] and len(g.right[j]) == 2 * len(g.left[i]) and set(g.left[i] + g.right[j]) == {a}]
    assert thirds and all(abs(s - 2 / 3) <= 2.3e-16 for s in thirds)
    ties = tp.RowRanks(want).kth_tie(3)
    assert ties is not None and ties > 0.0
    if g.size >= 256:
        assert sum(vr.saturated(s) for s in g.left) >= 4 and sum(vr.saturated(s) for s in g.right) >= 4
        assert len(vr.wrap_witnesses(g, want)) >= 30
    else:
        assert not any(vr.saturated(s) for s in g.left + g.right)
        if g.size == 64:  # the thermometer codes' extremes: a bucket of 64, a 16-bucket sum fed by two 32-buckets
            d = vr.SYMBOLS[alphabet][3]
            assert any(max(vr.bucket_counts(s)) == 64 for s in g.left) and any(a in s and d in s for s in g.left)


@pytest.mark.parametrize("name", vr.RAW_SATURATED)
def test_a_right_tile_that_only_a_valid_bound_keeps(name):
    """The last right tile holds the runs a^248 .. a^255 and nothing else (every other right row is longer).  Some left row
    has all eight as hits at 0.75 while a bound over wrapped counts prunes all eight: the kernel's wave-wide vote has no
    lane left to save the row.  The clipped bound prunes none of them."""
    g = vr.grid(name)
    assert len(g.left) == vr.STR_LEFT and len(g.right) == vr.STR_RIGHT
    tail = [j for j, s in enumerate(g.right) if len(s) in vr.TAIL_RUNS]
    assert len(tail) == 8 and all(len(s) >= 256 for j, s in enumerate(g.right) if j not in tail)
    want = tp.all_scores(g)
    score = {(i, j): s for s, i, j in want}
    for thr in vr.INDEL_THRESHOLDS:
        assert len(tp.expectation(want, thr)) > 0
    lost_rows = 0
    for i, x in enumerate(g.left):
        if all(score[(i, j)] >= 0.75 for j in tail):
            assert all(vr.histogram_bound(x, g.right[j], lambda v: min(v, 255)) >= score[(i, j)] for j in tail)
            lost_rows += all(vr.histogram_bound(x, g.right[j], lambda v: v % 256) < 0.75 for j in tail)
    assert lost_rows >= 2


@pytest.mark.parametrize("name", vr.LEVELS_STRINGS)
def test_low_entropy_level_strings(name):
    g = vr.grid(name)
    assert len(g.left) == 24 and len(g.right) == 70 and {len(it) for it in g.left + g.right} == {1, 2, 3}
    assert max(len(lv) for it in g.left + g.right for lv in it) == g.size
    want = tp.all_scores(g)
    assert len(want) == g.pairs
    for thr in vr.INDEL_THRESHOLDS:  # a levels score is below 1.0
        assert (len(tp.expectation(want, thr)) == 0) == (thr == 1.0)
    # hits whose step-1 strings a wrapping histogram would prune, and none that the saturating column prunes
    assert len(vr.levels_wrap_witnesses(g, want)) >= 8
    for s, i, j in want:
        x, y = (it[min(1, len(it) - 1)] for it in (g.left[i], g.right[j]))
        rest = 1.0 - 0.5 ** max(len(g.left[i]), len(g.right[j])) - 0.5
        assert vr.histogram_bound(x, y, lambda v: min(v, 255)) / 2 + rest >= s


# ----------------------------------------------------------------------------------------------------------- Part C
def _same_columns(table, model, names):
    for col in names:
        got = getattr(table, col).numpy()
        want = model[col]
        if got.dtype != want.dtype:  # torch has no unsigned 32 / 64 bit columns
            got = got.view(want.dtype).reshape(want.shape)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), col


@pytest.mark.parametrize("width", [16, 32, 64])
@pytest.mark.parametrize("width_in", [4, 16, 40, 100])
def test_numpy_set_encoder_against_the_model(width_in, width):
    from napkon_string_matching_amd import tables

    for side in (0, 1):
        case = vr.set_builder_case(width_in, width, levels=False, repeats=False, seed=side)
        model = vr.set_table_model(case["rows"], width, side, orig=case["orig"])
        t = tables.SetTable.from_padded(np.array(case["rows"], np.int32), ("left", "right")[side], "cpu", width=width,
                                        orig=np.array(case["orig"], np.int32), index=False)
        _same_columns(t, model, ("ids", "cnt", "sig", "sig2", "orig", "size_start"))
        case = vr.set_builder_case(width_in, width, levels=True, holes=False, seed=side)
        model = vr.set_table_model(case["rows"], width, side, case["nlev"], case["plen"], case["cat"], case["orig"])
        t = tables.SetTable.from_nested_arrays(np.array(case["rows"], np.int32), np.array(case["plen"], np.uint8),
                                               np.array(case["nlev"], np.int32), ("left", "right")[side], "cpu",
                                               categories=np.array(case["cat"], np.uint64), width=width, category_mode=1,
                                               partition=False, orig=np.array(case["orig"], np.int32), index=False)
        _same_columns(t, model, ("ids", "cnt", "sig", "sig2", "orig", "size_start", "nlev", "plen", "cat", "filt"))


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("stride,alphabet", [(64, 40), (128, 7), (256, 255), (512, 2)])
def test_numpy_str_encoder_against_the_model(stride, alphabet, sort):
    from napkon_string_matching_amd import tables

    case = vr.str_builder_case(stride, alphabet)
    model = vr.str_table_model(case["codes"], case["lengths"], alphabet, sort, case["orig"])
    assert stride < 256 or (model["hist"] == 255).any()
    t = tables.StrTable.from_codes(np.array(case["codes"], np.uint8), np.array(case["lengths"], np.int32), alphabet, "cpu",
                                   orig=np.array(case["orig"], np.int32), sort=sort)
    _same_columns(t, model, ("codes", "len", "orig", "hist") + (("len_start",) if sort else ()) +
                  (("hist16",) if sort and stride == 64 else ()))
    assert (t.len_start is None) == (not sort)


def test_models_on_rows_worked_by_hand():
    """The restatement itself, on rows small enough to check by eye against include/nsm_hip.h."""
    m = vr.set_table_model([[-7, 9, 9, -1, 2], [vr.INT32_MIN, -2, -1, -1, -1], [4, 1, 3, 2, 0]], 16, 1, orig=[10, 11, vr.INT32_MAX])
    assert m["ids"][:, :6].tolist() == [[0, 1, 2, 3, 4, -2], [2, 9, -2, -2, -2, -2], [-2] * 6]
    assert m["cnt"].tolist() == [5, 2, 0] and m["orig"].tolist() == [vr.INT32_MAX, 10, 11]
    assert m["size_start"].tolist() == [0] * 12 + [1] * 3 + [2, 2, 3] and m["sig"][2] == 0
    m = vr.set_table_model([[5, -1, 6, 7]], 16, 0, nlev=[2], plen=[[1, 3, 200, 0]], cat=[6])
    assert m["ids"][0, :4].tolist() == [5, 6, 7, -1] and m["plen"].tolist() == [[1, 3, 3, 3]]
    assert m["filt"][0, 2:5].tolist() == [6, 0, 3 | 3 << 8 | 2 << 16] and m["filt"][0, 7] == 0
    assert int(m["filt"][0, 0]) | int(m["filt"][0, 1]) << 32 == int(m["sig"][0]) == vr.signature_model([5, 6, 7], 0x9E3779B1)
    s = vr.str_table_model([[1] * 300 + [33] * 200 + [9] * 12, [2, 2, 7, 7] + [0] * 508], [500, 2], 40, True)
    assert s["len"].tolist() == [500, 2] and s["hist"][0, 1] == 255 and s["hist16"][0, 1] == 255 and s["hist"][1, 2] == 2
    assert s["codes"][1].tolist() == [2, 2] + [40] * 510 and s["len_start"][[0, 12, 13, 510, 511, 513]].tolist() == [0, 0, 1, 1, 2, 2]


# ----------------------------------------------------------------------------------------------------------- Part D
def test_edit_seam_alphabets_and_lds_arithmetic():
    """``pm_stride`` at the seam alphabets, and the dynamic LDS of the RAW Levenshtein sweep restated from ``kTopG``,
    ``pm_stride`` and the words of a row: exactly 64 KB at stride 256 over 255 symbols (the launcher asks only ABOVE it),
    96 KB and 128 KB on the two stride-512 grids."""
    import re
    from pathlib import Path

    assert [vr.pm_stride(a) for a in (40, 63, 64, 127, 128, 191, 192, 255)] == [64, 64, 128, 128, 192, 192, 256, 256]
    for alphabet in vr.SEAM_ALPHABETS + (255,):
        a, b, c, d = vr.SYMBOLS[alphabet]
        assert (a, b, c, d) == (alphabet - 1, alphabet - 33, alphabet - 2, alphabet - 17) and min(a, b, c, d) >= 0
        assert a & 31 == b & 31 and a & 31 != c & 31 and a & 15 == d & 15 and a & 31 != d & 31
        assert alphabet < vr.pm_stride(alphabet)  # the pad code has a mask of its own
        assert (a > 63) == (alphabet > 64)  # from 65 symbols on the highest code lies past the first 64 masks
    # A tripwire, no proof: the two literal texts below are how the source spells kTopG and pm_stride today.  A reformat of
    # the source trips it without harm (update the text here); it exists so that a CHANGE of either makes someone look at
    # vr.TOP_G / vr.pm_stride, which restate them.
    csrc = Path(__file__).resolve().parents[1] / "napkon-string-matching_amd" / "csrc"
    assert int(re.search(r"kTopG\s*=\s*(\d+)", (csrc / "top_k_raw_kernels.hpp").read_text()).group(1)) == vr.TOP_G
    assert "(left->alphabet + 1) + 63) / 64 * 64" in (csrc / "edit_raw.hip").read_text()
    lds = {name: vr.edit_lds_bytes(vr.edit_grid(name).size, vr.alphabet_of(vr.edit_grid(name))) for name in vr.EDIT_RAW}
    assert lds["value_edit_str_256_255"] == 64 * 1024 and lds["value_edit_str_512_128"] == 96 * 1024
    assert lds["value_edit_str_512_255"] == 128 * 1024 and [n for n, v in lds.items() if v > 64 * 1024] == vr.EDIT_RAW_W8
    assert sorted({vr.pm_stride(vr.alphabet_of(vr.edit_grid(n))) for n in vr.EDIT_RAW}) == [64, 128, 192, 256]


def test_edit_launch_table_has_twelve_instantiations():
    """query x prune x metric -> instantiation: sixteen launches, twelve distinct kernels (an unpruned sweep is the same
    under both metrics); the tests of tests/test_gpu_edit_ranges.py run every one, on every grid."""
    assert len(vr.EDIT_LAUNCHES) == 16 and len(set(vr.EDIT_LAUNCHES.values())) == 12
    assert {inst[3] for inst in vr.EDIT_LAUNCHES.values()} == {"TopLists<false>", "TopLists<true>", "ScoreTally", "FloorGate"}
    per_sink = {}
    for (query, prune, metric), (words, pruned, hist, sink) in vr.EDIT_LAUNCHES.items():
        assert words == 8 and pruned == prune and hist == (prune and metric == "edit")
        per_sink.setdefault(sink, set()).add((pruned, hist))
    assert all(v == {(False, False), (True, True), (True, False)} for v in per_sink.values())
    ran = {(q, prune, m) for queries in vr.EDIT_QUERIES.values() for q in queries for prune in (True, False) for m in vr.EDIT_METRICS}
    assert ran == set(vr.EDIT_LAUNCHES)


@pytest.mark.parametrize("name", vr.EDIT_RAW)
def test_edit_raw_grids_hold_their_seams(name):
    from support import edit_distance as ed

    g = vr.edit_grid(name)
    alphabet = vr.alphabet_of(g)
    a, b, c, _ = vr.SYMBOLS[alphabet]
    units = {u for side in (g.left, g.right) for s in side for u in s}
    assert {a, b, c} <= units and max(units) == a == alphabet - 1
    assert (len(g.left), len(g.right)) == ((32, 72) if g.size <= 128 else vr.EDIT_CUT)
    assert g.size <= 128 or (len(g.left) % vr.TOP_G != 0 and -(-len(g.left) // vr.TOP_G) == 3)  # three groups, the last ragged
    for side in (g.left, g.right):
        lengths = {len(s) for s in side}
        assert lengths >= {n for n in vr.EDIT_LENGTH_SEAMS if n <= g.size and (g.size >= 256 or n <= 1)}, (name, sorted(lengths))
    runs = lambda side: {len(s) for s in side if s and set(s) == {a}}
    doubles = [(m, 2 * m) for m in runs(g.left) if 2 * m in runs(g.left) and m in runs(g.right) and 2 * m in runs(g.right)]
    assert doubles, "no run of m units beside one of 2 m units on both sides"
    for metric in vr.EDIT_METRICS:
        full = vr.edit_records(g, metric)
        by_pair = {(i, j): s for s, i, j in full}
        assert len(full) == g.pairs
        bases = vr.edit_thresholds(full)
        assert bases[0] == 0.5 and bases[2] == 1.0
        for t in bases:  # a pair exactly on it, pairs below it
            assert any(h[0] == t for h in full) and full[-1][0] < t
        m, m2 = doubles[0]
        index = lambda side, n: next(k for k, s in enumerate(side) if s == [a] * n)
        short_long, long_short = by_pair[index(g.left, m), index(g.right, m2)], by_pair[index(g.left, m2), index(g.right, m)]
        assert (short_long, long_short) == ((0.5, 0.5) if metric == "edit" else (1.0, 0.5))
        # the stacked pass against the two-row programme on a few short pairs of the grid
        for i, j in list(by_pair)[:: max(1, len(by_pair) // 7)]:
            x, y = g.left[i], g.right[j]
            if len(x) * len(y) <= 64 * 64:
                dist = (ed.distance if metric == "edit" else ed.within)(tp.text(x), tp.text(y))
                assert by_pair[i, j] == ed.score(metric, len(x), len(y), dist)


@pytest.mark.parametrize("name", vr.EDIT_LEVELS)
def test_edit_levels_grids_hold_the_highest_symbol(name):
    g = vr.edit_grid(name)
    assert vr.alphabet_of(g) == 255 and (len(g.left), len(g.right)) == vr.EDIT_LEVELS_ITEMS
    assert {len(it) for it in g.left} == {1, 2, 3} == {len(it) for it in g.right}
    assert any(lv and set(lv) == {254} for it in g.right for lv in it)  # a level of nothing but the code alphabet - 1
    assert g.size // 2 < max(len(lv) for it in g.left + g.right for lv in it) <= g.size
    for metric in vr.EDIT_METRICS:
        plain, both_empty = vr.edit_records(g, metric, 0), vr.edit_records(g, metric, 2)
        assert len(plain) == g.pairs and 0 < len(both_empty) < g.pairs and set(both_empty) <= set(plain)
        cl, cr = vr.edit_categories(g, 2)
        assert any(int(cl[i]) == 0 == int(cr[j]) for _, i, j in both_empty)  # a pair of two items without a category
        for full in (plain, both_empty):
            for t in vr.edit_thresholds(full):
                assert any(h[0] == t for h in full) and full[-1][0] < t < full[0][0]
