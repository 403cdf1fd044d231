"""Do the seam corpora of tests/support/lcs_seams.py hold what they claim?  The oracle alone; nothing here needs a GPU.

* every pair with an LCS by construction scores ``indel_score(la, lb, that LCS)`` in the C oracle, bit for bit -- RAW grids
  and all four levels layouts: the oracle and the arithmetic are pinned to each other independently of any kernel;
* the cases of a stride reach EVERY instantiation of every loop (the host model of the dispatch in the support module), each
  padded loop with its smallest and its largest pattern: a later edit that drops a seam fails here, not nowhere;
* every case holds, per EARLY cadence, a pair whose score is a probe threshold and for which LCS so far + text units left
  equals ``need`` at a check point of that cadence (a plain model of the recurrence, right string as text as in the
  multi-word kernels);
* the size caps: at most 8 left and 64 + 37 right strings per case.
"""
import pytest

from support import lcs_abandon
from support import lcs_seams as ls
from support import threshold_probes as tp


def _cases(stride):
    return [ls.raw_case(stride, p, a) for p, a in ls.cases(stride)]


def test_case_grid():
    assert ls.pattern_lengths(64) == [1, 2, 3, 4, 5, 31, 32, 33, 63, 64]
    for stride in ls.STRIDES:
        lengths = ls.pattern_lengths(stride)
        assert {1, 2, 3, 4, 5} <= set(lengths) and max(lengths) == stride
        assert {32 * m + d for m in range(1, stride // 32 + 1) for d in (-1, 0, 1) if 32 * m + d <= stride} <= set(lengths)
        assert {64 * w + d for w in range(1, stride // 64 + 1) for d in (-1, 0, 1) if 64 * w + d <= stride} <= set(lengths)
        assert len(ls.CASE_IDS[stride]) == len(set(ls.CASE_IDS[stride])) == len(lengths) + 1


@pytest.mark.parametrize("stride", ls.STRIDES)
def test_sizes_lengths_and_alphabets(stride):
    for g in _cases(stride):
        assert 1 <= len(g.left) <= ls.MAX_LEFT and 1 <= len(g.right) <= ls.MAX_RIGHT
        assert all(len(s) == g.pattern for s in g.left), "one pattern length per case"
        assert max(len(s) for s in g.right) == stride, "the longest right string forces the stride"
        symbols = {u for s in g.left + g.right for u in s}
        assert len(symbols) == 255 if g.alpha else len(symbols) <= 8 + 8 + len(ls.seam_positions(g.pattern))
        # texts of every residue mod 4 (the last dword) and texts on both sides of the pattern's length
        lengths = {len(s) for s in g.right}
        assert {t % 4 for t in lengths} == {0, 1, 2, 3}
        assert min(lengths) < g.pattern and (g.pattern == stride or max(lengths) > g.pattern)
        late_letters = set(ls.LATE)
        holders = [j for j, s in enumerate(g.right) if late_letters & set(s)]  # one row holds the last-lane pattern's letters
        assert holders == [g.late[-1][1]] and g.late[-1][0] == 6 and len(g.left) == 7
        for layout in ls.LAYOUTS:
            lv = ls.levels_case(stride, g.pattern, g.alpha, layout)
            assert len({u for it in lv.left + lv.right for s in it for u in s}) <= 255
            assert [it[-1] for it in lv.left] == g.left or g.alpha
            assert all(len(it[-1]) == g.pattern for it in lv.left)


@pytest.mark.parametrize("stride", ls.STRIDES)
def test_closed_forms_are_the_oracles_scores(stride):
    for g in _cases(stride):
        at = {(i, j): s for s, i, j in tp.all_scores(g)}
        assert len(at) == g.pairs
        families = {g.source[j] for (_, j) in g.closed}
        assert families == set(range(7)), f"{g.name}: families with a closed form"
        for (i, j), lcs in g.closed.items():
            want = ls.indel_score(g.pattern, len(g.right[j]), lcs)
            assert at[(i, j)] == want, f"{g.name} pair {(i, j)}: oracle {at[(i, j)]!r}, closed form LCS {lcs} gives {want!r}"
        for i in range(len(g.left) - 1):  # self pairs
            assert g.closed[(i, i)] == g.pattern and at[(i, i)] == 1.0


@pytest.mark.parametrize("layout", ls.LAYOUTS)
@pytest.mark.parametrize("stride", ls.STRIDES)
def test_closed_forms_in_the_levels_layouts(stride, layout):
    for p, alpha in ls.cases(stride):
        g = ls.levels_case(stride, p, alpha, layout)
        at = {(i, j): s for s, i, j in tp.all_scores(g)}
        assert len(at) == g.pairs
        for (i, j), lcs in g.closed.items():
            want = ls.level_score(g, i, j, lcs)
            assert at[(i, j)] == want, f"{g.name} pair {(i, j)}: oracle {at[(i, j)]!r}, closed form {want!r}"
        if layout == "step2_sparse":  # a handful of right items per key (the last-lane pattern has its one row)
            for i in range(len(g.left)):
                assert (2 if i < 6 else 1) <= sum(1 for it in g.right if it[1] == g.left[i][1]) <= 40


def _lcs_of_prefixes(pat, text):
    """[LCS(pat, text[:c]) for c = 0 .. len(text)]: the bit-parallel recurrence on Python integers, one text unit a step."""
    masks = {}
    for k, u in enumerate(pat):
        masks[u] = masks.get(u, 0) | (1 << k)
    full = (1 << len(pat)) - 1
    v, out = full, [0]
    for u in text:
        x = v & masks.get(u, 0)
        v = ((v + x) | (v & ~x)) & full
        out.append(len(pat) - bin(v).count("1"))
    return out


def test_every_instantiation_is_reached():
    for stride in ls.STRIDES:
        K = stride // 64
        r = ls.reached(stride)
        # wide_lcs: every W <= K with its first and its last pattern length; the padded loops with both word counts
        want = set()
        for W in (1, 2, 3, 4, 6, 8):
            if W > K:
                continue
            for w in {6: (5, 6), 8: (7, 8)}.get(W, (W,)) if K == 8 else (W,):  # (patterns of 5 words run in the 6-word loop, ...)
                want |= {(K, W, 64 * (w - 1) + 1), (K, W, 64 * w)}
        assert want <= r["wide_lcs"], f"stride {stride}: wide_lcs misses {sorted(want - r['wide_lcs'])}"
        assert {W for _, W, _ in r["wide_lcs"]} == {W for W in (1, 2, 3, 4, 6, 8) if W <= K}
        assert {W for _, W, _ in r["wide_lcs2"]} == {W for W in (1, 2) if W <= K}
        assert K == 1 or {(K, 2, 65), (K, 2, 128), (K, 1, 64)} <= r["wide_lcs2"]
        # tile_lcs1: every L the dispatch can choose for this K, each with the smallest and the largest pattern it serves
        serves = {2: (1, 64), 3: (65, 96), 4: (97, 128), 5: (129, 160), 6: (161, 192), 8: (193, 256), 12: (257, 384), 16: (385, 512)}
        chosen = {1: (2,), 2: (2, 3, 4), 4: (2, 3, 4, 5, 6, 8), 8: (2, 3, 4, 5, 6, 8, 12, 16)}[K]
        assert {L for _, L, _ in r["tile_lcs1"]} == set(chosen)
        for L in chosen:
            lo, hi = serves[L]
            assert {(K, L, lo), (K, L, hi)} <= r["tile_lcs1"], f"stride {stride}: tile_lcs1<{K}, {L}> lacks {lo} or {hi}"
            if L in (8, 12, 16):  # padded loops: a pattern of the smallest and of the largest limb count, and the seams between
                assert {(K, L, lo + 31), (K, L, lo + 32), (K, L, hi - 32), (K, L, hi - 31)} <= r["tile_lcs1"]
        assert (K, 2, 32) in r["tile_lcs1"] and (K, 2, 33) in r["tile_lcs1"]
        # tile_lcs2: 2, 3, 4 limbs (a one-word stride has two)
        assert {L for L, _ in r["tile_lcs2"]} == ({2} if K == 1 else {2, 3, 4})
        assert K == 1 or {(2, 64), (3, 65), (3, 96), (4, 97), (4, 128)} <= r["tile_lcs2"]
        assert K <= 2 or any(not ls.tile_two_patterns(p, p) for p, _ in ls.cases(stride)), "the 2 x 64 cut-over to one pattern per pass"
        assert K <= 2 or {129} <= {p for p, _ in ls.cases(stride)}
        # RAW top-k: W = K, texts of every residue mod 16
        assert r["raw_top_k"] == {(K, q) for q in range(16)}
        if stride == 64:  # the finish kernel: both sweeps in both role orders
            assert r["finish"] == {(s, o) for s in ("narrow", "wide") for o in ("left_is_pattern", "right_is_pattern")}
    # the model itself at the seams the mutations aim at
    assert [ls.wide_words(8, p) for p in (64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512)] == \
        [1, 2, 2, 3, 3, 4, 4, 6, 6, 6, 6, 8, 8, 8, 8]
    assert [ls.tile1_limbs(8, p) for p in (32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256, 257, 384, 385, 512)] == \
        [2, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 8, 8, 8, 8, 12, 12, 16, 16]
    assert [ls.tile1_limbs(2, p) for p in (64, 65, 96, 97, 128)] == [2, 3, 3, 4, 4]
    assert ls.finish_sweep(32, 40) == ("narrow", "left_is_pattern") and ls.finish_sweep(40, 33) == ("wide", "right_is_pattern")


@pytest.mark.parametrize("stride", ls.STRIDES)
def test_late_matches_sit_on_the_stop_rule(stride):
    """Per case and cadence: a late-match pair whose score is a probe threshold; at that threshold ``need`` is its LCS, and
    LCS so far + units left == need at a check point of the cadence (never below it before: the pair must not be stopped)."""
    for g in _cases(stride):
        at = {(i, j): s for s, i, j in tp.all_scores(g)}
        probes = set(ls.probe_scores(g))
        assert len(g.late) <= 4 < ls.PROBE_CAP <= 8 and len(probes) <= ls.PROBE_CAP
        assert at[(0, 0)] in probes, "the self / run score"
        found = set()
        for i, j, m in g.late:
            pat, text = g.left[i], g.right[j]
            assert at[(i, j)] in probes, f"{g.name}: late pair {(i, j)} is not a probe"
            need = lcs_abandon.need_of(at[(i, j)], len(pat) + len(text))
            assert need == m == lcs_abandon.lcs_bits(pat, text) and set(text[: len(text) - m]) == {ls.JUNK}
            so_far = _lcs_of_prefixes(pat, text)
            for cadence in ls.CADENCES:
                for c in range(cadence, len(text), cadence):  # check points strictly inside the text
                    reach = so_far[c] + len(text) - c
                    assert reach >= need
                    if reach == need:
                        found.add(cadence)
        assert found == set(ls.CADENCES), f"{g.name}: cadences with reach == need at a check point: {sorted(found)}"
        # the same rows, the same LCS and the same lengths in every levels layout: their scores are probes there too
        for layout in ls.LAYOUTS:
            lv = ls.levels_case(stride, g.pattern, g.alpha, layout)
            lat = {(i, j): s for s, i, j in tp.all_scores(lv)}
            assert {lat[(i, j)] for i, j, _ in lv.late} <= set(ls.probe_scores(lv))
            assert len(ls.thresholds(lv)) <= 2 + 3 * ls.PROBE_CAP
