"""The two general kernels of csrc/any_grids.hip (``nsm_indel_any_grid``, ``nsm_jaccard_any_grid``) called directly
through their thin encoders (``wide.indel_any_grid``, ``wide.jaccard_any_grid``), against the C oracle: the identical
list of (score, i, j), scores bit for bit, no tolerance.  The grids come from tests/support/any_operands.py and aim at the
kernels' own edges: pattern lengths at the 128-unit chunk seams and text lengths at the 32-position carry words, the
4096-unit / 1023-symbol / 65535-id caps, depths from 1 to 300 in one wave, both layouts of the Jaccard operand, blocks
that walk several left rows, right-side tails, 64-bit category masks, zero-level items, and thresholds put exactly on
a pair's score (and one ulp above it).  tests/test_cpu_any_operands.py checks, with the oracle alone, that these grids
have hits and misses where this file needs them.
"""
import math

import numpy as np
import pytest

from support import any_operands as ao

pytestmark = pytest.mark.gpu


def _kernel(g, thr, capacity=None):
    from napkon_string_matching_amd import wide

    left, right = ao.kernel_operands(g)
    fn = wide.indel_any_grid if g.kind == "indel" else wide.jaccard_any_grid
    return fn(left, right, thr, g.cat_l, g.cat_r, g.mode, raw=g.raw, capacity=capacity).as_tuples()


def _chosen_layout(g):
    """The rule of wide.jaccard_any_grid, on this grid's inputs."""
    from napkon_string_matching_amd import wide

    deepest = max(max((len(it) for it in g.left), default=1), max((len(it) for it in g.right), default=1), 1)
    nested = all(wide._nested(it) for items in (g.left, g.right) for it in items)
    return "independent" if deepest > wide.FAST_LEVELS or not nested else "nested"


def _first_difference(got, want):
    extra, missing = sorted(set(got) - set(want))[:4], sorted(set(want) - set(got))[:4]
    return f"got {len(got)} hits, oracle {len(want)}; only in got {extra}; only in oracle {missing}"


def _check(g):
    if g.kind == "jaccard":
        assert _chosen_layout(g) == g.layout, f"{g.name}: built for the {g.layout} layout"
    all_hits = ao.oracle_all(g)
    seen = {}
    for thr in ao.thresholds(g, all_hits):
        want = ao.oracle_at(all_hits, thr)
        # (threshold 0.0: every allowed pair is a hit; the small buffer overflows and run_grid launches a second time)
        got = seen[thr] = _kernel(g, thr, capacity=7 if thr == 0.0 else None)
        assert got == want, f"{g.name} at threshold {thr!r}: {_first_difference(got, want)}"
    if g.probe:  # (implied by the equalities above; spelled out, since it is what these thresholds are for)
        for s in ao.probe_scores(all_hits):
            at = {(i, j) for score, i, j in all_hits if score == s}
            assert at, s
            here = {(i, j) for _, i, j in seen[s]}
            above = {(i, j) for _, i, j in seen[math.nextafter(s, 2.0)]}
            assert at <= here and not at & above, f"{g.name}: pairs scoring exactly {s!r}: {sorted(at - here)[:4]} lost at it, " \
                                                   f"{sorted(at & above)[:4]} kept one ulp above"


FUZZY = ["fuzzy_length_edges", "fuzzy_length_edges_raw", "fuzzy_alphabet_1", "fuzzy_alphabet_255", "fuzzy_alphabet_256",
         "fuzzy_alphabet_1023", "fuzzy_depths"]
JACCARD = ["jaccard_depths_deep", "jaccard_depths_64", "jaccard_nested", "jaccard_independent", "jaccard_raw_wide"]
GEOMETRY = [f"tails_{k}_{n}" for k in ("indel", "jaccard") for n in ao.RIGHT_TAILS]
MASKED = [n for n in ao.CATALOGUE if n.startswith(("categories_", "zero_levels_apart_"))]


def test_lists_cover_the_catalogue():
    assert sorted(FUZZY + JACCARD + GEOMETRY + MASKED + ["many_rows_indel", "many_rows_jaccard"]) == sorted(ao.CATALOGUE)


@pytest.mark.parametrize("name", FUZZY)
def test_fuzzy_kernel_matches_oracle(name):
    """Length edges of the chunked LCS (levels and RAW), alphabets of exactly 1 / 255 / 256 / 1023 code units, depths
    1 .. 300 in one wave; thresholds at exact scores where the grid asks for them."""
    _check(ao.grid(name))


@pytest.mark.parametrize("name", JACCARD)
def test_jaccard_kernel_matches_oracle(name):
    """Both layouts (asserted): ids entering at different levels on the two sides, 64 levels exactly, wide against
    small items, repeated tokens, levels that are not nested, levels empty on the right, more than 64 levels."""
    _check(ao.grid(name))


@pytest.mark.parametrize("name", GEOMETRY)
def test_right_side_tails(name):
    _check(ao.grid(name))


@pytest.mark.parametrize("kind", ["indel", "jaccard"])
def test_blocks_that_walk_several_rows(kind):
    g = ao.grid(f"many_rows_{kind}")
    rows = ao.rows_per_chunk(len(g.left), len(g.right))
    assert rows >= 2 and len(g.left) % rows != 0, "every block must walk several left rows, the last block fewer"
    _check(g)


@pytest.mark.parametrize("name", MASKED)
def test_category_masks_and_zero_level_items(name):
    g = ao.grid(name)
    top = np.uint64(1) << np.uint64(63)
    assert (g.cat_l & top).any() and (g.cat_r & top).any()
    _check(g)


@pytest.mark.parametrize("name", sorted(ao.ZERO_ONLY))
def test_grid_of_zero_level_items(name):
    """Every allowed pair scores 0.0: all of them at threshold 0.0, none at the smallest positive threshold."""
    g = ao.grid(name)
    all_hits = ao.oracle_all(g)
    assert all_hits and all(h[0] == 0.0 for h in all_hits)
    assert (len(all_hits) == g.pairs) == (g.mode == ao.CAT_NONE)
    assert _kernel(g, 0.0, capacity=7) == all_hits
    for thr in (5e-324, 1e-300, 0.5, ao.ABOVE_ONE):
        assert _kernel(g, thr) == []


def test_jaccard_independent_layout_raw(monkeypatch):
    """RAW quotient in the independent layout.  wide.jaccard_any_grid never picks it for single-level items (they are
    always nested), the C entry accepts it: the layout rule is overridden for this call."""
    from napkon_string_matching_amd import wide

    g = ao.grid("jaccard_raw_wide")
    monkeypatch.setattr(wide, "_nested", lambda levels: False)
    all_hits = ao.oracle_all(g)
    for thr in ao.thresholds(g, all_hits):
        assert _kernel(g, thr, capacity=7 if thr == 0.0 else None) == ao.oracle_at(all_hits, thr), thr


def test_jaccard_item_at_the_id_cap():
    """65535 ids in one item: a cell of the kernel's 16-bit histogram of first common steps holds up to 65535."""
    from napkon_string_matching_amd import wide

    left, right, want = ao.jaccard_cap_pair()
    assert max(len(set(lv)) for lv in left[0]) == wide.ANY_IDS
    assert wide.jaccard_any_grid(left, right, 0.0).as_tuples() == want
    best = want[0][0]
    assert best == 0.875 and want[1][0] < best
    assert wide.jaccard_any_grid(left, right, best).as_tuples() == want[:1]
    assert wide.jaccard_any_grid(left, right, want[1][0]).as_tuples() == want
    assert wide.jaccard_any_grid(left, right, math.nextafter(best, 2.0)).as_tuples() == []


def test_caps_are_refused_before_any_launch(monkeypatch):
    from napkon_string_matching_amd import grid, wide

    def no_launch(*args, **kwargs):
        raise AssertionError("a grid beyond the caps reached the launcher")

    monkeypatch.setattr(grid, "run_grid", no_launch)
    symbols = [chr(ao.BASE + v) for v in range(wide.ANY_ALPHABET + 1)]
    with pytest.raises(NotImplementedError):
        wide.indel_any_grid([["".join(symbols[:600])]], [["".join(symbols[600:])]], 0.5)
    with pytest.raises(NotImplementedError):
        wide.indel_any_grid([["ab" * 2048 + "a"]], [["ab"]], 0.5)
    with pytest.raises(NotImplementedError):
        wide.indel_any_grid([["ab"]], [["b"], ["a" * (wide.ANY_LEN + 1)]], 0.5)
    too_many = [list(range(wide.ANY_IDS + 1))]
    with pytest.raises(NotImplementedError):
        wide.jaccard_any_grid([too_many], [[[1]]], 0.5)
    with pytest.raises(NotImplementedError):  # the independent layout has the cap per level
        wide.jaccard_any_grid([[[1], [2]]], [[[3]] + too_many], 0.5)
