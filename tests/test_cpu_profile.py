"""Threshold profiles without a GPU: ``grid.profile_of_hits`` (the definition every kernel is checked against) on the
oracle's score lists, merging, the validation of a ladder, and the C ABI's four ``nsm_*_profile`` entries."""
import re
from pathlib import Path

import numpy as np
import pytest

from support import threshold_probes as tp

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("nsm_indel_raw_profile", "nsm_jaccard_raw_profile", "nsm_indel_levels_profile", "nsm_jaccard_levels_profile")


def _hits(records):
    from napkon_string_matching_amd import grid

    return grid.Hits(np.array([r[0] for r in records], dtype=np.float64), np.array([r[1] for r in records], dtype=np.int32),
                     np.array([r[2] for r in records], dtype=np.int32))


def _ladders(g):
    t = tp.thresholds_around(tp.probes_of(g))
    return [t[k:k + 64] for k in range(0, len(t), 64)]


@pytest.mark.parametrize("make,size", [(tp.raw_indel, 64), (tp.raw_jaccard, 16)])
def test_profile_of_hits_is_the_plain_count(make, size):
    from napkon_string_matching_amd import grid

    g = make(size)
    records = tp.all_scores(g)
    assert len(records) > 1000
    for ladder in _ladders(g) + [[0.0], [0.0, 0.25, 0.5, 1.0], [1.5, 2.0]]:
        prof = grid.profile_of_hits(_hits(records), ladder, len(g.left), len(g.right))
        kept = [r for r in records if r[0] >= ladder[0]]
        assert prof.pairs.dtype == np.uint64 and prof.pairs.tolist() == [sum(1 for r in kept if r[0] >= t) for t in ladder]
        left = [max((r[0] for r in kept if r[1] == i), default=-1.0) for i in range(len(g.left))]
        right = [max((r[0] for r in kept if r[2] == j), default=-1.0) for j in range(len(g.right))]
        assert prof.left_best.tolist() == left and prof.right_best.tolist() == right
        assert prof.matched_left().tolist() == [sum(1 for b in left if b >= t) for t in ladder]
        assert prof.matched_right().tolist() == [sum(1 for b in right if b >= t) for t in ladder]


def test_merging_two_halves_gives_the_whole():
    from napkon_string_matching_amd import grid

    g = tp.raw_indel(64)
    records = tp.all_scores(g)
    ladder = _ladders(g)[0]
    n, m = len(g.left), len(g.right)
    whole = grid.profile_of_hits(_hits(records), ladder, n, m)
    cut = m // 3
    parts = []
    for cols in (np.arange(cut), np.arange(cut, m)):  # two column blocks, each indexed from 0 as a sub-grid is
        lo = int(cols[0])
        part = [(s, i, j - lo) for s, i, j in records if lo <= j < lo + len(cols)]
        parts.append((grid.profile_of_hits(_hits(part), ladder, n, len(cols)), np.arange(n), cols))
    merged = grid.merge_profiles(parts, ladder, n, m)
    assert merged.pairs.tolist() == whole.pairs.tolist()
    assert merged.left_best.tolist() == whole.left_best.tolist() and merged.right_best.tolist() == whole.right_best.tolist()


@pytest.mark.parametrize("bad", [[], [k / 100 for k in range(65)], [0.5, 0.4], [0.3, 0.3], [0.1, float("nan")], [float("nan")]],
                         ids=["empty", "65", "descending", "equal", "nan_last", "nan_only"])
def test_ladder_validation(bad):
    from napkon_string_matching_amd import grid

    with pytest.raises(ValueError):
        grid.check_thresholds(bad)
    with pytest.raises(ValueError):
        grid.profile_of_hits(_hits([(0.5, 0, 0)]), bad, 1, 1)


def test_ladder_of_64_is_accepted():
    from napkon_string_matching_amd import grid

    t = grid.check_thresholds(k / 64 for k in range(64))
    assert t.dtype == np.float64 and len(t) == 64


def test_header_declares_and_lib_binds_the_entries():
    from napkon_string_matching_amd import _lib

    header = (ROOT / "include" / "nsm_hip.h").read_text()
    for name in ENTRIES:
        decl = re.search(rf"\bint {name}\(([^;]*)\);", header)
        assert decl, name
        args = decl.group(1)
        assert "const double* thresholds" in args and "int32_t n_thresholds" in args
        assert "uint64_t* pairs" in args and "double* left_best" in args and "double* right_best" in args
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5
