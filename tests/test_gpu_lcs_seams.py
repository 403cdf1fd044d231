"""Every Indel entry and route on the seam corpora of tests/support/lcs_seams.py: one case = one (stride, pattern length), all
left strings of that length, so that every bit-parallel LCS loop runs the instantiation the case names (the host model in
the support module; tests/test_cpu_lcs_seams.py asserts that the cases reach every one) on runs whose carries ripple
through every word, on matches that sit in the top word or limb only, on markers at the limb and word seams, on texts of
every length modulo 4 and 16, and on late-match rows that sit exactly on the EARLY stop rules.

For each call the kernel's list must equal the oracle's list cut at the threshold: same pairs, same order, scores bit for
bit.  Thresholds per case: 0.0, 1.0 and at most 5 oracle scores (the late-match pairs', then the self pairs') with one ulp
to either side.  The expectation never depends on which loop ran.
"""
import random

import numpy as np
import pytest

from support import best_matches as bm
from support import lcs_seams as ls
from support import probe_tables
from support import threshold_probes as tp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _case(stride, cid):
    p, alpha = ls.cases(stride)[ls.CASE_IDS[stride].index(cid)]
    return p, alpha


def _same(g, route, thr, got, want):
    assert got == want, f"{g.name} / {route} at threshold {thr!r}: {probe_tables.first_difference(got, want)}"


def _check_grid(g, route, run):
    """``run(thr)`` -> the kernel's (score, i, j) list."""
    all_hits = tp.all_scores(g)
    for thr in ls.thresholds(g):
        _same(g, route, thr, run(thr), tp.expectation(all_hits, thr))


def _check_top_k(g, route, run, every_ulp=True):
    """``run(k, thr)``: per left item the first k of the oracle's list cut at the threshold, (score descending, j ascending).
    ``every_ulp`` = False (the routes without pruning, whose kernels score every pair whatever the threshold, the slowest
    calls of this file): 0.0, 1.0 and the probe scores themselves."""
    ranks = tp.RowRanks(tp.all_scores(g))
    for k in (1, 3, len(g.right)):
        for thr in ls.thresholds(g) if every_ulp else sorted({0.0, 1.0} | set(ls.probe_scores(g))):
            _same(g, f"{route} k={k}", thr, run(k, thr), ranks.cut(thr, k))


def _check_profile(g, route, run):
    """``pairs[k]`` = the length of the oracle's list at t[k]; the bests are its maxima per item, -1.0 without a hit.  The
    whole ladder (the bests go by 0.0) and the ladder from its first positive threshold on."""
    ladder = ls.thresholds(g)
    for t in (ladder, ladder[1:]):
        kept = tp.expectation(tp.all_scores(g), t[0])
        lb, rb = bm.bests(kept)
        prof = run(t)
        assert prof.pairs.tolist() == [len(tp.expectation(kept, x)) for x in t], f"{g.name} / {route} from {t[0]!r}: pairs"
        assert prof.left_best.tolist() == [lb.get(i, -1.0) for i in range(len(g.left))], f"{g.name} / {route} from {t[0]!r}: left_best"
        assert prof.right_best.tolist() == [rb.get(j, -1.0) for j in range(len(g.right))], f"{g.name} / {route} from {t[0]!r}: right_best"


def _check_floor_grid(g, route, run):
    """Floors = every item's best score (its ties survive): one side, the other, both and none at 0.0; both sides with the
    threshold on every probe score and at 1.0."""
    lb, rb = bm.bests(tp.all_scores(g))
    left = np.array([lb.get(i, 0.0) for i in range(len(g.left))])
    right = np.array([rb.get(j, 0.0) for j in range(len(g.right))])
    for thr in [0.0, 1.0] + ls.probe_scores(g):
        kept = tp.expectation(tp.all_scores(g), thr)
        for lf, rf in ((left, right),) + (((left, None), (None, right), (None, None)) if thr == 0.0 else ()):
            _same(g, f"{route} floors", thr, run(thr, lf, rf), bm.floors_plain(kept, lf, rf))


def _check_pairs(g, run):
    """All N x M pairs of the grid, in an order of its own, some twice: scores bit for bit."""
    from napkon_string_matching_amd import grid

    rng = random.Random(len(g.name))
    listed = [(i, j) for i in range(len(g.left)) for j in range(len(g.right))]
    listed += rng.sample(listed, 50)
    rng.shuffle(listed)
    i, j = np.array([p[0] for p in listed]), np.array([p[1] for p in listed])
    want = grid.lookup_pairs(tp.all_scores(g), i, j)
    got = run(i, j)
    assert (want >= 0.0).all() and got.dtype == np.float64
    bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
    assert not len(bad), f"{g.name}: {len(bad)} scores differ, first {listed[bad[0]]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


# ---------------------------------------------------------------------------------------------------------------- RAW
def _raw_routes(stride):
    from napkon_string_matching_amd import grid

    def grid_route(prune):
        return lambda g, lt, rt: _check_grid(g, f"grid prune={prune}", lambda thr: grid.indel_raw_grid(
            lt, rt, thr, capacity=g.pairs + 1, prune=prune).as_tuples())

    def top_k(prune):
        return lambda g, lt, rt: _check_top_k(g, f"top_k prune={prune}", lambda k, thr: grid.indel_raw_top_k(
            lt, rt, k, thr, prune=prune).as_tuples(), every_ulp=prune)

    def profile(prune):
        return lambda g, lt, rt: _check_profile(g, f"profile prune={prune}", lambda t: grid.indel_raw_profile(lt, rt, t, prune=prune))

    def floors(prune):
        return lambda g, lt, rt: _check_floor_grid(g, f"floor_grid prune={prune}", lambda thr, lf, rf: grid.indel_raw_floor_grid(
            lt, rt, thr, lf, rf, prune=prune, capacity=g.pairs + 1).as_tuples())

    routes = {}
    if stride > 64:  # (the stride-64 grid routes have tests/support/lcs_abandon.py)
        routes.update({"grid-prune": grid_route(True), "grid-no_prune": grid_route(False)})
    routes.update({"top_k-prune": top_k(True), "top_k-no_prune": top_k(False), "profile-prune": profile(True),
                   "profile-no_prune": profile(False), "floor_grid-prune": floors(True), "floor_grid-no_prune": floors(False),
                   "pairs": lambda g, lt, rt: _check_pairs(g, lambda i, j: grid.indel_raw_pairs(lt, rt, i, j))})
    return routes


RAW_ROUTE_NAMES = {s: (["grid-prune", "grid-no_prune"] if s > 64 else []) +
                   ["top_k-prune", "top_k-no_prune", "profile-prune", "profile-no_prune", "floor_grid-prune", "floor_grid-no_prune", "pairs"]
                   for s in ls.STRIDES}
RAW_PARAMS = [pytest.param(s, c, r, id=f"{c}-{r}") for s in ls.STRIDES for c in ls.CASE_IDS[s] for r in RAW_ROUTE_NAMES[s]]


@pytest.mark.parametrize("stride,case,route", RAW_PARAMS)
def test_raw(dev, stride, case, route):
    """``wide_lcs<K, EARLY>`` (grid), the inline W-word loop of the top-k kernels (top-k, profile, floor grid) and the pairs
    kernel on the RAW strings of the case."""
    g = ls.raw_case(stride, *_case(stride, case))
    lt, rt = probe_tables.raw_indel_tables(g, dev)
    _raw_routes(stride)[route](g, lt, rt)


# ------------------------------------------------------------------------------------------------------------- levels
def _forced(flag_name):
    """``NSM_FLAG_SPLIT`` / ``NSM_FLAG_TILE`` through the C entry, with the workspace the library asks for when every pair
    is expected to survive; on the split route the overflow word must stay 0: the split path itself produced the hits."""
    # (a copy of the helper in tests/test_gpu_threshold_probes.py, without categories)
    def run(tabs, g, thr):
        import torch

        from napkon_string_matching_amd import _lib, grid

        li, ls_, ri, rs = tabs
        lib = _lib.load()
        device = li.first.device
        flags = _lib.FLAG_PRUNE | getattr(_lib, flag_name)
        asked = int(lib.nsm_indel_levels_workspace_bytes(li.struct(), ls_.struct(), ri.struct(), rs.struct(), thr, flags, float(g.pairs)))
        # (the scan kernel of the split path holds two 64-entry mask tables: with more than 63 symbols the library asks for no
        # workspace and the same call runs the single-kernel path -- the 255-symbol case; same comparison either way)
        split = flag_name == "FLAG_SPLIT" and ls_.alphabet + 1 <= 64
        assert (asked >= 1024) if split else (asked == 0 or flag_name == "FLAG_TILE")
        ws = torch.zeros(asked // 8, dtype=torch.int64, device=device) if asked else None
        buf = grid.HitBuffer(g.pairs + 1, device)
        buf.reset()
        _lib.check(lib.nsm_indel_levels_grid(li.struct(), ls_.struct(), ri.struct(), rs.struct(), thr, 0, flags,
                                             buf.records.data_ptr(), buf.capacity, buf.count.data_ptr(),
                                             ws.data_ptr() if ws is not None else 0, asked, float(g.pairs),
                                             torch.cuda.current_stream(device).cuda_stream), "nsm_indel_levels_grid")
        n = int(buf.count.item())  # synchronises the stream
        if split:
            assert int(ws[1].item()) & 0xFFFFFFFF == 0, f"{g.name} at threshold {thr!r}: the survivor queue overflowed"
        return grid.sort_hits_device(buf, n).as_tuples()

    return run


def _through_grid(**kw):
    def run(tabs, g, thr):
        from napkon_string_matching_amd import grid

        return grid.indel_levels_grid(*tabs, thr, capacity=g.pairs + 1, **kw).as_tuples()

    return run


GRID_ROUTES = {"default": _through_grid(), "park": _through_grid(park=True), "wave_wide": _through_grid(wave_wide=True),
               "no_prune": _through_grid(prune=False), "no_workspace": _through_grid(workspace=0),
               "forced_split": _forced("FLAG_SPLIT"), "forced_tile": _forced("FLAG_TILE")}
ONE_WORD_ONLY = ("no_prune", "no_workspace", "forced_split", "forced_tile")
OTHER_ROUTES = ("top_k-prune", "top_k-no_prune", "profile", "floor_grid", "pairs")
LEVELS_PARAMS = [pytest.param(s, c, r, id=f"{c}-{r}") for s in ls.STRIDES for c in ls.CASE_IDS[s]
                 for r in list(GRID_ROUTES) + list(OTHER_ROUTES) if s == 64 or r not in ONE_WORD_ONLY]


@pytest.mark.parametrize("stride,case,route", LEVELS_PARAMS)
def test_levels(dev, stride, case, route):
    """The same strings as level strings, in the four layouts of ``lcs_seams.levels_case`` (one after the other: a failure
    names the layout with the grid): the shared-tile kernel (default route of the multi-word strides:
    ``tile_lcs2_any<K, EARLY>`` at step 1, ``tile_lcs1_any`` / ``tile_lcs2_any`` wave-wide, the dense pass, the generic
    full-limb pass of deep items), the park kernel (``wide_lcs`` / ``wide_lcs2``), the wave-wide kernel, the levels top-k
    kernels (top-k, profile, floor grid) and the pairs kernel; at stride 64 also the split path (scan -> queue ->
    ``lane_lcs`` of the finish kernel) and the one-word tile kernel, forced through the C entry."""
    import torch

    from napkon_string_matching_amd import _lib, grid

    try:
        for layout in ls.LAYOUTS:
            g = ls.levels_case(stride, *_case(stride, case), layout)
            tabs = probe_tables.levels_indel_tables(g, dev, False)
            if route in GRID_ROUTES:
                _check_grid(g, route, lambda thr: GRID_ROUTES[route](tabs, g, thr))
            elif route.startswith("top_k"):
                prune = route == "top_k-prune"
                _check_top_k(g, route, lambda k, thr: grid.indel_levels_top_k(*tabs, k, thr, prune=prune).as_tuples(), every_ulp=prune)
            elif route == "profile":
                for prune in (True, False):
                    _check_profile(g, f"profile prune={prune}", lambda t: grid.indel_levels_profile(*tabs, t, prune=prune))
            elif route == "floor_grid":
                for prune in (True, False):
                    _check_floor_grid(g, f"floor_grid prune={prune}", lambda thr, lf, rf: grid.indel_levels_floor_grid(
                        *tabs, thr, lf, rf, prune=prune, capacity=g.pairs + 1).as_tuples())
            else:
                _check_pairs(g, lambda i, j: grid.indel_levels_pairs(*tabs, i, j))
    finally:
        if stride == 64 and route in ("default", "forced_split"):  # the side stream and events of the split path
            torch.cuda.synchronize(dev)
            assert _lib.load().nsm_release(torch.cuda.current_stream(dev).cuda_stream) == 0
