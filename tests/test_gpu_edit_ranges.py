"""The Levenshtein kernels at their alphabet and LDS seams, every query against the definitions: same pairs, same order,
same doubles.

tests/test_gpu_edit_distance.py draws every string from 36 symbols, so the match-mask stride ``pm_stride`` of
csrc/edit_raw.hip and csrc/edit_levels.hip -- the alphabet and its pad code rounded up to a multiple of 64 -- was always
64 there.  Here (tests/support/value_ranges.py, Part D; tests/test_cpu_value_ranges.py checks the premises without a GPU):

* RAW grids at stride 64 over alphabets of 63, 64, 127, 128, 191 and 192 symbols (``pm_stride`` 64, 128, 128, 192, 192,
  256), whose strings use the highest legal code ``alphabet - 1`` (above 63: past the first 64 masks, where a clamp of the
  symbol to the wrong bound folds it onto another symbol), its neighbour, and a symbol of the same histogram bucket;
* strides 128 and 256 over 255 symbols -- at stride 256 the sweep's match masks fill exactly 64 KB of LDS, the far side of
  the launcher's comparison -- and stride 512 over 128 and 255 symbols: 96 KB and 128 KB, which the launcher has to ask
  for, once per instantiation of the kernel.  ``vr.EDIT_LAUNCHES`` maps query x prune x metric to the instantiation; every
  one of the twelve at eight words is launched by the tests below on both stride-512 grids;
* levels grids over 255 symbols at strides 256 and 512 (csrc/edit_levels.hip indexes its masks by the code unit as it is).

The yardstick is the two-row dynamic programme of tests/support/edit_distance.py, d and w of a pair from one pass; for the
levels grids the oracle's ``compare_terms`` with that definition as score_func.  Cached per process.
"""
import numpy as np
import pytest

from support import best_matches as bm
from support import probe_tables
from support import threshold_probes as tp
from support import value_ranges as vr

pytestmark = pytest.mark.gpu
CASES = [(n, m) for n in vr.EDIT_RAW for m in vr.EDIT_METRICS]
LEVELS_CASES = [(n, m, mode) for n in vr.EDIT_LEVELS for m in vr.EDIT_METRICS for mode in (0, 2)]


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _case(name, metric, dev):
    """(grid, left table, right table, every pair's record, the base thresholds)."""
    from napkon_string_matching_amd import tables

    g = vr.edit_grid(name)

    def make():
        alphabet = vr.alphabet_of(g)
        lt = tables.StrTable.from_codes(*vr.codes_of(g.left, g.size), alphabet, dev)
        rt = tables.StrTable.from_codes(*vr.codes_of(g.right, g.size), alphabet, dev)
        assert lt.stride == rt.stride == g.size and lt.alphabet == rt.alphabet == alphabet
        assert lt.hist is not None and rt.hist is not None  # (with them NSM_FLAG_PRUNE under "edit" is the histogram variant)
        assert int(lt.codes.max()) == alphabet  # the pad code; the highest symbol is alphabet - 1
        return lt, rt

    lt, rt = probe_tables.cached(g.name, make)
    full = vr.edit_records(g, metric)
    assert len(full) == g.pairs
    lds = vr.TOP_G * vr.pm_stride(lt.alphabet) * (lt.stride // 64) * 8
    assert lds == vr.edit_lds_bytes(g.size, vr.alphabet_of(g)) and (lds > 64 * 1024) == (name in vr.EDIT_RAW_W8)
    return g, lt, rt, full, vr.edit_thresholds(full)


def _launches(queries, metric):
    """The instantiations a test launches: its queries, pruned and unpruned, under its metric -- all in the table."""
    keys = [(q, prune, metric) for q in queries for prune in (True, False)]
    assert all(k in vr.EDIT_LAUNCHES for k in keys)
    return keys


def _same(got, want, what):
    assert got == want, f"{what}: {probe_tables.first_difference(got, want)}"


@pytest.mark.parametrize("name,metric", CASES)
def test_threshold_grid(dev, name, metric):
    """The floor grid without floors, at thresholds that each have a pair exactly on them and at their two neighbours."""
    from napkon_string_matching_amd import grid

    g, lt, rt, full, bases = _case(name, metric, dev)
    for _, prune, _ in _launches(vr.EDIT_QUERIES["threshold_grid"], metric):
        for thr in vr.around(bases):
            got = grid.indel_raw_grid(lt, rt, thr, prune=prune, metric=metric).as_tuples()
            _same(got, tp.expectation(full, thr), f"{name} {metric} prune={prune} at {thr!r}")


@pytest.mark.parametrize("name,metric", CASES)
def test_top_k(dev, name, metric):
    from napkon_string_matching_amd import grid

    g, lt, rt, full, bases = _case(name, metric, dev)
    groups = tp.groups_of(g)
    for query, prune, _ in _launches(vr.EDIT_QUERIES["top_k"], metric):
        grp = groups if query == "top_k_grouped" else None
        ranks = tp.RowRanks(full, None if grp is None else grp.tolist())
        for k in (1, 3):
            for thr in (0.0, bases[0], bases[1]):
                got = grid.indel_raw_top_k(lt, rt, k, thr, prune=prune, groups=grp, metric=metric).as_tuples()
                _same(got, ranks.cut(thr, k), f"{name} {metric} {query} prune={prune} k={k} at {thr!r}")


@pytest.mark.parametrize("name,metric", CASES)
def test_profile_and_best(dev, name, metric):
    from napkon_string_matching_amd import grid

    g, lt, rt, full, bases = _case(name, metric, dev)
    ladder = vr.around(bases)
    kept = tp.expectation(full, ladder[0])
    lb, rb = bm.bests(kept)
    hits = bm.to_hits(tp.expectation(full, 0.0))
    for _, prune, _ in _launches(vr.EDIT_QUERIES["profile_and_best"][:1], metric):
        prof = grid.indel_raw_profile(lt, rt, ladder, prune=prune, metric=metric)
        assert prof.pairs.tolist() == [len(tp.expectation(kept, t)) for t in ladder], f"{name} {metric} prune={prune}: pairs"
        assert prof.left_best.tolist() == [lb.get(i, -1.0) for i in range(len(g.left))], f"{name} {metric} prune={prune}: left_best"
        assert prof.right_best.tolist() == [rb.get(j, -1.0) for j in range(len(g.right))], f"{name} {metric} prune={prune}: right_best"
        for mutual in (False, True):
            want = grid.best_of_hits(hits, 0.0, mutual, len(g.left), len(g.right)).as_tuples()
            got = grid.indel_raw_best(lt, rt, 0.0, 0.0, mutual=mutual, prune=prune, metric=metric).as_tuples()
            _same(got, want, f"{name} {metric} best mutual={mutual} prune={prune}")
            assert len(want) >= (1 if mutual else len(g.left))


@pytest.mark.parametrize("name,metric", CASES)
def test_floor_grid(dev, name, metric):
    """Floors on every item's best score (its ties survive): one side, the other, both."""
    from napkon_string_matching_amd import grid

    g, lt, rt, full, bases = _case(name, metric, dev)
    lb, rb = bm.bests(full)
    left = np.array([lb[i] for i in range(len(g.left))])
    right = np.array([rb[j] for j in range(len(g.right))])
    for _, prune, _ in _launches(vr.EDIT_QUERIES["floor_grid"], metric):
        for thr in (0.0, bases[0]):
            kept = tp.expectation(full, thr)
            for lf, rf in ((left, None), (None, right), (left, right)):
                got = grid.indel_raw_floor_grid(lt, rt, thr, lf, rf, prune=prune, metric=metric).as_tuples()
                want = bm.floors_plain(kept, lf, rf)
                assert len(want) > 0
                _same(got, want, f"{name} {metric} floors prune={prune} at {thr!r}")


@pytest.mark.parametrize("name,metric", CASES)
def test_listed_pairs(dev, name, metric):
    """Every pair of the grid (csrc/edit_pairs.hip: a wave per pair, no LDS masks)."""
    from napkon_string_matching_amd import grid

    g, lt, rt, full, _ = _case(name, metric, dev)
    by_pair = {(i, j): s for s, i, j in full}
    listed = sorted(by_pair, key=lambda p: (p[1] * 7 + p[0]) % 101)  # (an order of its own)
    i, j = np.array([p[0] for p in listed]), np.array([p[1] for p in listed])
    got = grid.indel_raw_pairs(lt, rt, i, j, metric=metric)
    want = np.array([by_pair[p] for p in listed])
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), f"{name} {metric}: {len(bad)} scores differ, first {listed[bad[0]]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


# ============================================================================================================== levels
def _levels_case(name, metric, mode, dev):
    from napkon_string_matching_amd import tables

    g = vr.edit_grid(name)
    alphabet = vr.alphabet_of(g)
    cl, cr = vr.edit_categories(g, mode)

    def make():
        tabs = tables.encode_level_codes(vr.level_codes_of(g.left, g.size), vr.level_codes_of(g.right, g.size), alphabet, dev,
                                         cl, cr, mode, partition=False)
        assert tabs[1].stride == tabs[3].stride == g.size and tabs[1].alphabet == alphabet == 255
        return tabs

    return g, probe_tables.cached((g.name, mode), make), vr.edit_records(g, metric, mode)


@pytest.mark.parametrize("name,metric,mode", LEVELS_CASES)
def test_levels_queries(dev, name, metric, mode):
    """``nsm_edit_levels_top_k``, ``_profile`` and ``_floor_grid`` over 255 symbols, without categories and under the "both
    empty" category mode; ``nsm_edit_levels_pairs`` (which knows no predicate) once per grid."""
    from napkon_string_matching_amd import grid

    g, tabs, full = _levels_case(name, metric, mode, dev)
    assert 0 < len(full) and (mode == 0) == (len(full) == g.pairs)
    bases = vr.edit_thresholds(full)
    ladder = vr.around(bases)
    ranks = tp.RowRanks(full)
    lb, rb = bm.bests(full)
    left = np.array([lb.get(i, 0.0) for i in range(len(g.left))])
    right = np.array([rb.get(j, 0.0) for j in range(len(g.right))])
    for prune in (True, False):
        what = f"{name} {metric} mode {mode} prune={prune}"
        for k in (1, 3):
            for thr in (0.0,) + tuple(bases):
                got = grid.indel_levels_top_k(*tabs, k, thr, category_mode=mode, prune=prune, metric=metric).as_tuples()
                _same(got, ranks.cut(thr, k), f"{what} top-k k={k} at {thr!r}")
        kept = tp.expectation(full, ladder[0])
        klb, krb = bm.bests(kept)
        prof = grid.indel_levels_profile(*tabs, ladder, category_mode=mode, prune=prune, metric=metric)
        assert prof.pairs.tolist() == [len(tp.expectation(kept, t)) for t in ladder], f"{what}: pairs"
        assert prof.left_best.tolist() == [klb.get(i, -1.0) for i in range(len(g.left))], f"{what}: left_best"
        assert prof.right_best.tolist() == [krb.get(j, -1.0) for j in range(len(g.right))], f"{what}: right_best"
        for thr in ladder:
            for lf, rf in ((None, None), (left, right)):
                got = grid.indel_levels_floor_grid(*tabs, thr, lf, rf, category_mode=mode, prune=prune, metric=metric).as_tuples()
                _same(got, bm.floors_plain(tp.expectation(full, thr), lf, rf), f"{what} floors at {thr!r}")
    if mode == 0:
        by_pair = {(i, j): s for s, i, j in full}
        listed = sorted(by_pair, key=lambda p: (p[1] * 5 + p[0]) % 97)
        got = grid.indel_levels_pairs(*tabs, np.array([p[0] for p in listed]), np.array([p[1] for p in listed]), metric=metric)
        want = np.array([by_pair[p] for p in listed])
        bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
        assert not len(bad), f"{name} {metric}: {len(bad)} scores differ, first {listed[bad[0]]}: {got[bad[0]]!r} != {want[bad[0]]!r}"
