"""Every fast-path grid and top-k kernel with the threshold put exactly on oracle scores, and one ulp to either side.

A pair is a hit iff ``score >= threshold``, and almost every fast path decides from a bound derived from the threshold
whether to compute the score at all: the smallest step-1 LCS of the scan / park / split / tile kernels (float, with a margin
of 2e-3 of an LCS unit), the ``score + rest + 1e-6 >= threshold`` early exits, ``ceil(2 thr m (1 - 1e-9))`` of the Jaccard
kernels, the length and histogram floors of the top-k kernels, the launchers' integer tables and the prefix lengths of the
global index.  The rule all of them must keep: a bound may skip a pair only when the pair is strictly below the threshold,
and every float bound carries a margin above its own rounding.

The grids (tests/support/threshold_probes.py; tests/test_cpu_threshold_probes.py checks them with the oracle alone) hold
scores shared by hundreds of pairs, distinct scores a few ulps apart, and tight families whose bounds are met with equality.
For every grid, route and threshold the kernel's list must equal the oracle's list cut at the threshold: same pairs, same
order, scores bit for bit.  Then the property itself: the pairs scoring exactly ``s`` are all present at ``s`` and one ulp
below it, and none of them one ulp above.

At most 40 probes x 3 thresholds per route, every tight-family score and every ulp twin among them.  The per-tile index of
the RAW Jaccard grid exists for widths 16 and 32 only, so width 64 has no "index_tile" route.
"""
import numpy as np
import pytest

from support import threshold_probes as tp
from support import probe_tables
from support.probe_checks import check as _check, check_top_k as _check_top_k

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------------------- RAW Indel
RAW_INDEL_ROUTES = {64: {"two_stage": dict(two_stage=True), "one_stage": dict(two_stage=False), "no_prune": dict(prune=False)},
                    128: {"prune": dict(prune=True), "no_prune": dict(prune=False)}}
RAW_INDEL_CASES = [(n, r) for n in tp.RAW_INDEL for r in RAW_INDEL_ROUTES[64 if n.endswith("_64") else 128]]


@pytest.mark.parametrize("name,route", RAW_INDEL_CASES)
def test_indel_raw_grid(dev, name, route):
    """The launcher's tables of smallest LCS per length sum (``lcsmin``), the 16- and 32-bucket histogram filters and the
    in-scan early exit of the multi-word LCS; strings that fill the row on both sides (la + lb = 2 * stride)."""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    lt, rt = probe_tables.raw_indel_tables(g, dev)
    kw = RAW_INDEL_ROUTES[64 if g.size == 64 else 128][route]
    _check(g, route, lambda thr: grid.indel_raw_grid(lt, rt, thr, capacity=g.pairs + 1, **kw).as_tuples())


# ------------------------------------------------------------------------------------------------------- RAW Jaccard
RAW_JACCARD_ROUTES = {"prune": dict(prune=True, index=False), "no_prune": dict(prune=False, index=False),
                      "index_global": dict(index=True), "index_tile": dict(index="tile"), "index_auto": dict(index=None)}
RAW_JACCARD_CASES = [(n, r) for n in tp.RAW_JACCARD for r in RAW_JACCARD_ROUTES if not (r == "index_tile" and n.endswith("_64"))]


@pytest.mark.parametrize("name,route", RAW_JACCARD_CASES)
def test_jaccard_raw_grid(dev, name, route):
    """``ceil`` of the smallest intersection, the signature bound, the prefix lengths of the global index (on a right table
    that carries its postings) and the per-tile index; 1/2, 1/3, 2/3 shared by hundreds of pairs, subset pairs."""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    lt, rt = probe_tables.raw_jaccard_tables(g, dev)
    kw = RAW_JACCARD_ROUTES[route]
    _check(g, route, lambda thr: grid.jaccard_raw_grid(lt, rt, thr, capacity=g.pairs + 1, **kw).as_tuples())


# ---------------------------------------------------------------------------------------------------- levels Jaccard
LEVELS_JACCARD_ROUTES = {f"{'prune' if prune else 'no_prune'}-index_{label}": dict(prune=prune, index=index)
                         for prune in (True, False)
                         for label, index in (("auto", None), ("never", False), ("global", True), ("tile", "tile"))}


@pytest.mark.parametrize("route", LEVELS_JACCARD_ROUTES)
@pytest.mark.parametrize("name", tp.LEVELS_JACCARD)
def test_jaccard_levels_grid(dev, name, route):
    """The size bound ``ceil(2 thr m (1 - 1e-9))`` of the filter kernel and of the global index, per category variant."""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    lt, rt = probe_tables.levels_jaccard_tables(g, dev, g.partition)
    kw = LEVELS_JACCARD_ROUTES[route]
    _check(g, route, lambda thr: grid.jaccard_levels_grid(lt, rt, thr, category_mode=g.mode, capacity=g.pairs + 1, **kw).as_tuples())


# ------------------------------------------------------------------------------------------------------ levels Indel
def _forced(flag_name):
    """``NSM_FLAG_SPLIT`` / ``NSM_FLAG_TILE`` through the C entry, with the workspace the library asks for; on the split
    route the overflow word must stay 0: the split path itself produced the hits.  (Expected survivors: every pair -- the low
    thresholds keep them all alive, and the queue is to hold them.)"""
    def run(tabs, g, thr):
        import torch

        from napkon_string_matching_amd import _lib, grid

        li, ls, ri, rs = tabs
        lib = _lib.load()
        dev = li.first.device
        flags = _lib.FLAG_PRUNE | getattr(_lib, flag_name)
        mode = int(li.category_mode if li.category_mode is not None else g.mode)
        asked = int(lib.nsm_indel_levels_workspace_bytes(li.struct(), ls.struct(), ri.struct(), rs.struct(), thr, flags, float(g.pairs)))
        assert (asked >= 1024) if flag_name == "FLAG_SPLIT" else asked >= 0
        ws = torch.zeros(asked // 8, dtype=torch.int64, device=dev) if asked else None
        buf = grid.HitBuffer(g.pairs + 1, dev)
        buf.reset()
        _lib.check(lib.nsm_indel_levels_grid(li.struct(), ls.struct(), ri.struct(), rs.struct(), thr, mode, flags,
                                             buf.records.data_ptr(), buf.capacity, buf.count.data_ptr(),
                                             ws.data_ptr() if ws is not None else 0, asked, float(g.pairs),
                                             torch.cuda.current_stream(dev).cuda_stream), "nsm_indel_levels_grid")
        n = int(buf.count.item())  # synchronises the stream
        if flag_name == "FLAG_SPLIT":
            assert int(ws[1].item()) & 0xFFFFFFFF == 0, f"{g.name} at threshold {thr!r}: the survivor queue overflowed"
        return grid.sort_hits_device(buf, n).as_tuples()

    return run


def _through_grid(**kw):
    def run(tabs, g, thr):
        from napkon_string_matching_amd import grid

        return grid.indel_levels_grid(*tabs, thr, category_mode=g.mode, capacity=g.pairs + 1, **kw).as_tuples()

    return run


ONE_WORD_ROUTES = {"default": _through_grid(), "park": _through_grid(park=True), "wave_wide": _through_grid(wave_wide=True),
                   "no_prune": _through_grid(prune=False), "no_workspace": _through_grid(workspace=0),
                   "forced_split": _forced("FLAG_SPLIT"), "forced_tile": _forced("FLAG_TILE")}
MULTI_WORD_ROUTES = {"shared_tile": _through_grid(), "park": _through_grid(park=True), "wave_wide": _through_grid(wave_wide=True)}


@pytest.mark.parametrize("route", ONE_WORD_ROUTES)
@pytest.mark.parametrize("name", tp.ONE_WORD)
def test_indel_levels_grid_one_word(dev, name, route):
    """The smallest step-1 LCS (``needf``, 2e-3 of margin) of the scan, park, split and tile kernels and their
    ``score + rest + 1e-6`` early exits, on tight families (every bound of steps >= 2 met with equality) and anagram pairs
    (histogram bound 1.0, ratio below it), on both sides of the routing thresholds 0.55 and 0.7."""
    import torch

    from napkon_string_matching_amd import _lib

    g = tp.grid(name)
    tabs = probe_tables.levels_indel_tables(g, dev, g.partition)
    try:
        _check(g, route, lambda thr: ONE_WORD_ROUTES[route](tabs, g, thr))
    finally:
        if route in ("default", "forced_split"):  # the side stream and events of the split path
            torch.cuda.synchronize(dev)
            assert _lib.load().nsm_release(torch.cuda.current_stream(dev).cuda_stream) == 0


@pytest.mark.parametrize("route", MULTI_WORD_ROUTES)
@pytest.mark.parametrize("name", tp.MULTI_WORD)
def test_indel_levels_grid_multi_word(dev, name, route):
    """The same bound in the shared-tile, park and wave-wide kernels at strides 128, 256 and 512; a tight family whose step-1
    strings fill the row (n1 = 2 * stride, 1024 at stride 512: the largest float rounding of ``needf``)."""
    g = tp.grid(name)
    tabs = probe_tables.levels_indel_tables(g, dev, g.partition)
    _check(g, route, lambda thr: MULTI_WORD_ROUTES[route](tabs, g, thr))


# -------------------------------------------------------------------------------------------------------------- top-k
PRUNE = {"prune": True, "no_prune": False}


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("name", tp.RAW_INDEL)
def test_indel_raw_top_k(dev, name, route, grouped):
    """The length and histogram floors ``ceil(eff (la + lb) / 2) - 1`` with ``eff = max(threshold, floor)``."""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    lt, rt = probe_tables.raw_indel_tables(g, dev)
    groups = tp.groups_of(g) if grouped else None
    _check_top_k(g, f"top_k-{route}-{'grouped' if grouped else 'plain'}",
                 lambda k, thr: grid.indel_raw_top_k(lt, rt, k, thr, prune=PRUNE[route], groups=groups).as_tuples(), groups)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("name", tp.RAW_JACCARD)
def test_jaccard_raw_top_k(dev, name, route, grouped):
    """The size floor ``floor(eff (a + b) / (1 + eff)) - 1`` and the signature bound."""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    lt, rt = probe_tables.raw_jaccard_tables(g, dev)
    groups = tp.groups_of(g) if grouped else None
    _check_top_k(g, f"top_k-{route}-{'grouped' if grouped else 'plain'}",
                 lambda k, thr: grid.jaccard_raw_top_k(lt, rt, k, thr, prune=PRUNE[route], groups=groups).as_tuples(), groups)


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("name", tp.ONE_WORD + tp.MULTI_WORD)
def test_indel_levels_top_k(dev, name, route):
    """The ``+ 1e-9`` early exits of the levels top-k kernel (tables without a partition, as the kernel asks)."""
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    tabs = probe_tables.levels_indel_tables(g, dev, False)
    _check_top_k(g, f"top_k-{route}",
                 lambda k, thr: grid.indel_levels_top_k(*tabs, k, thr, category_mode=g.mode, prune=PRUNE[route]).as_tuples())


@pytest.mark.parametrize("route", PRUNE)
@pytest.mark.parametrize("name", tp.LEVELS_JACCARD)
def test_jaccard_levels_top_k(dev, name, route):
    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    lt, rt = probe_tables.levels_jaccard_tables(g, dev, False)
    _check_top_k(g, f"top_k-{route}",
                 lambda k, thr: grid.jaccard_levels_top_k(lt, rt, k, thr, category_mode=g.mode, prune=PRUNE[route]).as_tuples())
