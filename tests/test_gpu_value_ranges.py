"""Column values at the edges of their ranges, every entry against the oracle: same pairs, same order, same doubles.

The other GPU files feed the kernels dense token ids (a ``Vocabulary`` renumbers them from 0) and strings drawn at random
from alphabets of 4 .. 200 symbols.  Here (tests/support/value_ranges.py; tests/test_cpu_value_ranges.py checks the premises
without a GPU):

* Part A -- token ids over the whole int32 range.  RAW tables take any id >= 0; levels tables ids below 2^26
  (``NSM_LEVELS_ID_LIMIT``), the two that shift to the bit patterns of the padding included, and the builder and both
  encoder paths refuse anything beyond, as they refuse a global inverted index for ids from 2^25 on.
* Part B -- runs, blocks and periodic strings over two or three symbols: histogram buckets at and beyond the ``uint8``
  ceiling, exact ties across rows and length classes, scores on 2/3.
* Part C -- ``nsm_build_set_table`` / ``nsm_build_str_table`` through ctypes on every clause of their comments (ids in any
  slots, assorted negative values, ``width_in`` != width, garbage past the last level and past the length), every column
  byte for byte against the per-row restatement of the header.

No case skips or shrinks itself; an expected list is empty only where the CPU file shows it (a levels score never reaches
1.0: its weights sum to 1 - 2^-steps).
"""
import ctypes

import numpy as np
import pytest

from support import best_matches as bm
from support import probe_tables
from support import threshold_probes as tp
from support import value_ranges as vr
from test_gpu_threshold_probes import LEVELS_JACCARD_ROUTES, RAW_INDEL_ROUTES, RAW_JACCARD_ROUTES

pytestmark = pytest.mark.gpu
PRUNE = {"prune": True, "no_prune": False}
BADARG = 10001


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ tables
def _raw_jaccard_tables(g, dev, index=None):
    from napkon_string_matching_amd import tables

    def make():
        lt = tables.SetTable.from_padded(vr.padded(g.left, g.size), "left", dev, width=g.size)
        rt = tables.SetTable.from_padded(vr.padded(g.right, g.size), "right", dev, width=g.size, index=index)
        assert lt.width == rt.width == g.size and lt.post is None
        return lt, rt

    return probe_tables.cached((g.name, "index", index), make)


def _nested_table(g, side, dev, partition, **kw):
    from napkon_string_matching_amd import tables

    items, cat = (g.left, g.cat_l) if side == "left" else (g.right, g.cat_r)
    ids, plen, nlev = vr.nested_arrays(items, g.size)
    return tables.SetTable.from_nested_arrays(ids, plen, nlev, side, dev, categories=cat, width=g.size, category_mode=g.mode,
                                              partition=partition, **kw)


def _levels_jaccard_tables(g, dev, partition):
    def make():
        lt, rt = _nested_table(g, "left", dev, partition), _nested_table(g, "right", dev, partition)
        assert (lt.seg is not None) == partition and lt.width == rt.width == g.size
        return lt, rt

    return probe_tables.cached((g.name, partition), make)


def _raw_string_tables(g, dev):
    from napkon_string_matching_amd import tables

    def make():
        alphabet = vr.alphabet_of(g)
        lt = tables.StrTable.from_codes(*vr.codes_of(g.left, g.size), alphabet, dev)
        rt = tables.StrTable.from_codes(*vr.codes_of(g.right, g.size), alphabet, dev)
        assert lt.stride == rt.stride == g.size and (g.size != 64 or (lt.hist16 is not None and rt.hist16 is not None))
        return lt, rt

    return probe_tables.cached(g.name, make)


def _levels_string_tables(g, dev):
    from napkon_string_matching_amd import tables

    def make():
        tabs = tables.encode_level_codes(vr.level_codes_of(g.left, g.size), vr.level_codes_of(g.right, g.size), 40, dev)
        assert tabs[1].stride == tabs[3].stride == g.size
        return tabs

    return probe_tables.cached(g.name, make)


# ------------------------------------------------------------------------------------------------------------ checks
def _cut(g, thr):
    """The oracle's list at ``thr``; empty only where no score can reach the threshold (levels grids at 1.0)."""
    want = tp.expectation(tp.all_scores(g), thr)
    assert (len(want) == 0) == (thr == 1.0 and not g.raw), f"{g.name}: expected list at {thr!r}"
    return want


def _check_grid(g, thresholds, route, run):
    for thr in thresholds:
        want, got = _cut(g, thr), run(thr)
        assert got == want, f"{g.name} / {route} at threshold {thr!r}: {probe_tables.first_difference(got, want)}"


def _check_top_k(g, thresholds, ks, route, run, groups=None):
    ranks = tp.RowRanks(tp.all_scores(g), None if groups is None else groups.tolist())
    for k in ks:
        for thr in thresholds:
            want, got = ranks.cut(thr, k), run(k, thr)
            assert (len(want) == 0) == (len(_cut(g, thr)) == 0)
            assert got == want, f"{g.name} / {route} k={k} at threshold {thr!r}: {probe_tables.first_difference(got, want)}"


def _check_profile(g, thresholds, route, run):
    """``pairs[k]`` = the length of the oracle's list at t[k]; the bests are its maxima per item, -1.0 without a hit."""
    ladder = sorted(thresholds)
    for t0 in range(len(ladder)):  # every suffix of the ladder: each threshold is once the one the bests go by
        t = ladder[t0:]
        kept = _cut(g, t[0])
        lb, rb = bm.bests(kept)
        prof = run(t)
        assert prof.pairs.tolist() == [len(tp.expectation(kept, x)) for x in t], f"{g.name} / {route} from {t[0]!r}: pairs"
        assert prof.left_best.tolist() == [lb.get(i, -1.0) for i in range(len(g.left))], f"{g.name} / {route} from {t[0]!r}: left_best"
        assert prof.right_best.tolist() == [rb.get(j, -1.0) for j in range(len(g.right))], f"{g.name} / {route} from {t[0]!r}: right_best"


def _check_floor_grid(g, thresholds, route, run):
    """Floors on every item's best score (its ties survive), one side, the other, both; and no floors at all."""
    lb, rb = bm.bests(tp.all_scores(g))
    left = np.array([lb.get(i, 0.0) for i in range(len(g.left))])
    right = np.array([rb.get(j, 0.0) for j in range(len(g.right))])
    for thr in thresholds:
        kept = _cut(g, thr)
        for lf, rf in ((None, None), (left, None), (None, right), (left, right)):
            want, got = bm.floors_plain(kept, lf, rf), run(thr, lf, rf)
            assert (lf is None and rf is None) or len(want) > 0 or not kept
            assert got == want, f"{g.name} / {route} floors at {thr!r}: {probe_tables.first_difference(got, want)}"


def _check_pairs(g, run):
    """Every pair of the grid, in an order of its own, some twice."""
    import random

    from napkon_string_matching_amd import grid

    assert g.cat_l is None  # (the pairs entries know no category predicate)
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


def _groups(g):
    return tp.groups_of(g)


# =========================================================================================================== Part A
RAW_JACCARD_CASES = [(n, r) for n in vr.JACCARD_RAW for r in ("prune", "no_prune", "index_tile") if not (r == "index_tile" and n.endswith("_64"))]


@pytest.mark.parametrize("name,route", RAW_JACCARD_CASES)
def test_jaccard_raw_grid_any_int32_id(dev, name, route):
    """Ids from LOW and IMAGES, 2^31 - 1 among them: a RAW kernel compares whole ids, so an alias pair scores 0."""
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    lt, rt = _raw_jaccard_tables(g, dev)
    assert rt.post is None  # (2^31 keys: the default leaves the global index out)
    kw = RAW_JACCARD_ROUTES[route]
    _check_grid(g, vr.JACCARD_THRESHOLDS, route, lambda thr: grid.jaccard_raw_grid(lt, rt, thr, capacity=g.pairs + 1, **kw).as_tuples())
    got = {(i, j) for _, i, j in grid.jaccard_raw_grid(lt, rt, 5e-324, capacity=g.pairs + 1, **kw).as_tuples()}
    assert not got & set(vr.alias_pairs(g)), "an alias pair shares no id"


@pytest.mark.parametrize("name", vr.JACCARD_RAW)
def test_jaccard_raw_queries_any_int32_id(dev, name):
    """Top-k (plain and grouped, prune on and off, k = 1, 3, n_right), profile, floor grid and pairs on the same tables."""
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    lt, rt = _raw_jaccard_tables(g, dev)
    groups = _groups(g)
    for route, prune in PRUNE.items():
        for grp in (None, groups):
            _check_top_k(g, vr.JACCARD_THRESHOLDS, (1, 3, len(g.right)), f"top_k-{route}-{'plain' if grp is None else 'grouped'}",
                         lambda k, thr: grid.jaccard_raw_top_k(lt, rt, k, thr, prune=prune, groups=grp).as_tuples(), grp)
        _check_profile(g, vr.JACCARD_THRESHOLDS, f"profile-{route}", lambda t: grid.jaccard_raw_profile(lt, rt, t, prune=prune))
        _check_floor_grid(g, vr.JACCARD_THRESHOLDS, f"floor_grid-{route}",
                          lambda thr, lf, rf: grid.jaccard_raw_floor_grid(lt, rt, thr, lf, rf, prune=prune, capacity=g.pairs).as_tuples())
    _check_pairs(g, lambda i, j: grid.jaccard_raw_pairs(lt, rt, i, j))


@pytest.mark.parametrize("route", ["index_global", "index_auto"])
@pytest.mark.parametrize("name", vr.JACCARD_RAW_SMALL)
def test_jaccard_raw_global_index_below_its_limit(dev, name, route):
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    lt, rt = _raw_jaccard_tables(g, dev)
    assert rt.post is not None and rt.vocab == max(vr.SMALL) + 1
    kw = RAW_JACCARD_ROUTES[route]
    _check_grid(g, vr.JACCARD_THRESHOLDS, route, lambda thr: grid.jaccard_raw_grid(lt, rt, thr, capacity=g.pairs + 1, **kw).as_tuples())


def test_global_index_is_refused_from_2_pow_25_on(dev):
    """Both encoder paths refuse ``index=True`` with the same ``ValueError``; ``index=None`` leaves the index out and the grid
    stays exact; the largest id the index takes builds it."""
    from napkon_string_matching_amd import grid, tables

    left = np.array([[3, vr.GLOBAL_INDEX_LIMIT, 9], [3, -1, -1], [vr.GLOBAL_INDEX_LIMIT - 1, 3, -1]], np.int32)
    right = np.array([[vr.GLOBAL_INDEX_LIMIT, 3, -1], [9, -1, -1], [vr.GLOBAL_INDEX_LIMIT - 1, -1, -1]], np.int32)
    messages = []
    for device in ("cpu", dev):
        with pytest.raises(ValueError, match=r"below 2\^25") as err:
            tables.SetTable.from_padded(right, "right", device, width=16, index=True)
        messages.append(str(err.value))
    assert messages[0] == messages[1]
    lt = tables.SetTable.from_padded(left, "left", dev, width=16)
    rt = tables.SetTable.from_padded(right, "right", dev, width=16)
    assert rt.post is None
    want = [(s, i, j) for s, i, j in vr.set_scores(tp.ProbeGrid("tiny", "jaccard", True, [[v for v in r if v >= 0] for r in left],
                                                                [[v for v in r if v >= 0] for r in right])) if s >= 0.3]
    assert len(want) >= 3
    for kw in RAW_JACCARD_ROUTES.values():
        assert grid.jaccard_raw_grid(lt, rt, 0.3, **kw).as_tuples() == want
    below = np.where(right == vr.GLOBAL_INDEX_LIMIT, 11, right)
    rt = tables.SetTable.from_padded(below, "right", dev, width=16, index=True)
    assert rt.post is not None and rt.vocab == vr.GLOBAL_INDEX_LIMIT
    want = [(s, i, j) for s, i, j in vr.set_scores(tp.ProbeGrid("tiny", "jaccard", True, [[v for v in r if v >= 0] for r in left],
                                                                [[v for v in r if v >= 0] for r in below])) if s >= 0.3]
    assert len(want) >= 3 and grid.jaccard_raw_grid(lt, rt, 0.3, index=True).as_tuples() == want


@pytest.mark.parametrize("route", LEVELS_JACCARD_ROUTES)
@pytest.mark.parametrize("name", vr.LEVELS_LOW + vr.LEVELS_SMALL)
def test_jaccard_levels_grid_ids_below_the_limit(dev, name, route):
    """Every id a levels table may hold, 2^26 - 1 and 2^26 - 2 (the bit patterns of the left and the right padding once
    shifted) in many rows and alone in some.  The LOW tables are beyond a global index (2^26 keys: forcing "an index" takes
    the per-tile one), the SMALL tables carry it."""
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    lt, rt = _levels_jaccard_tables(g, dev, g.partition)
    assert (rt.post is not None) == (name in vr.LEVELS_SMALL)
    kw = LEVELS_JACCARD_ROUTES[route]
    _check_grid(g, vr.JACCARD_THRESHOLDS, route,
                lambda thr: grid.jaccard_levels_grid(lt, rt, thr, category_mode=g.mode, capacity=g.pairs + 1, **kw).as_tuples())


@pytest.mark.parametrize("name", vr.LEVELS_LOW + vr.LEVELS_SMALL)
def test_jaccard_levels_queries_ids_below_the_limit(dev, name):
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    lt, rt = _levels_jaccard_tables(g, dev, False)
    for route, prune in PRUNE.items():
        _check_top_k(g, vr.JACCARD_THRESHOLDS, (1, 3, len(g.right)), f"top_k-{route}",
                     lambda k, thr: grid.jaccard_levels_top_k(lt, rt, k, thr, category_mode=g.mode, prune=prune).as_tuples())
        _check_profile(g, vr.JACCARD_THRESHOLDS[:3], f"profile-{route}",
                       lambda t: grid.jaccard_levels_profile(lt, rt, t, category_mode=g.mode, prune=prune))
        _check_floor_grid(g, vr.JACCARD_THRESHOLDS, f"floor_grid-{route}",
                          lambda thr, lf, rf: grid.jaccard_levels_floor_grid(lt, rt, thr, lf, rf, category_mode=g.mode, prune=prune,
                                                                             capacity=g.pairs).as_tuples())
    prof = grid.jaccard_levels_profile(lt, rt, [1.0], category_mode=g.mode)  # (nothing reaches 1.0)
    assert prof.pairs.tolist() == [0] and (prof.left_best == -1.0).all() and (prof.right_best == -1.0).all()
    if g.cat_l is None:
        _check_pairs(g, lambda i, j: grid.jaccard_levels_pairs(lt, rt, i, j))


# ------------------------------------------------------------------------------------------------- the builders' C ABI
def _build_set(dev, rows, width, side, nlev=None, plen=None, cat=None, orig=None):
    """``nsm_build_set_table`` through ctypes on caller-allocated, poisoned columns: (status, message, rows built, columns)."""
    import torch

    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    n, width_in = len(rows), len(rows[0])
    up = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(np.array(a, dtype=dtype))).to(dev)
    new = lambda shape, dtype: torch.full(shape, 0x5A, dtype=dtype, device=dev)
    levels = nlev is not None
    max_levels = len(plen[0]) if levels else 0
    cols = dict(ids=new((n, width), torch.int32), cnt=new((n,), torch.int32), sig=new((n,), torch.int64), sig2=new((n,), torch.int64),
                orig=new((n,), torch.int32), size_start=new((width + 2,), torch.int32))
    if levels:
        cols.update(nlev=new((n,), torch.int32), plen=new((n, max_levels), torch.uint8), filt=new((n, 8), torch.int32))
        if cat is not None:
            cols["cat"] = new((n,), torch.int64)
    ptr = lambda name: cols[name].data_ptr() if name in cols else None
    st = _lib.NsmSetTable(ptr("ids"), ptr("cnt"), ptr("sig"), ptr("sig2"), ptr("orig"), ptr("size_start"), ptr("nlev"), ptr("plen"),
                          ptr("cat"), ptr("filt"), None, None, n, width, max_levels)
    ins = [up(rows, np.int32), up(nlev, np.int32) if levels else None, up(plen, np.uint8) if levels else None,
           torch.from_numpy(np.array(cat, dtype=np.uint64).view(np.int64)).to(dev) if cat is not None else None,
           up(orig, np.int32) if orig is not None else None]
    p = [None if t is None else t.data_ptr() for t in ins]
    rc = lib.nsm_build_set_table(p[0], n, width_in, side, p[1], p[2], p[3], p[4], _lib.CAT_INTERSECT if cat is not None else 0, 0,
                                 ctypes.byref(st), torch.cuda.current_stream(dev).cuda_stream)
    return rc, (lib.nsm_last_error().decode() if rc else None), st.n, {k: v.cpu().numpy() for k, v in cols.items()}


def _build_str(dev, codes, lengths, alphabet, sort, orig=None):
    import torch

    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    n, stride = len(codes), len(codes[0])
    new = lambda shape, dtype: torch.full(shape, 0x5A, dtype=dtype, device=dev)
    cols = dict(codes=new((n, stride), torch.uint8), len=new((n,), torch.int32), orig=new((n,), torch.int32),
                hist=new((n, 32), torch.uint8), hist16=new((n, 16), torch.uint8))
    if sort:
        cols["len_start"] = new((stride + 2,), torch.int32)
    st = _lib.NsmStrTable(cols["codes"].data_ptr(), cols["len"].data_ptr(), cols["orig"].data_ptr(),
                          cols["len_start"].data_ptr() if sort else None, cols["hist"].data_ptr(), n, stride, alphabet,
                          cols["hist16"].data_ptr())
    ins = [torch.from_numpy(np.array(codes, np.uint8)).to(dev), torch.from_numpy(np.array(lengths, np.int32)).to(dev),
           None if orig is None else torch.from_numpy(np.array(orig, np.int32)).to(dev)]
    rc = lib.nsm_build_str_table(ins[0].data_ptr(), ins[1].data_ptr(), None if orig is None else ins[2].data_ptr(), n,
                                 _lib.BUILD_SORT if sort else 0, ctypes.byref(st), torch.cuda.current_stream(dev).cuda_stream)
    return rc, (lib.nsm_last_error().decode() if rc else None), st.n, {k: v.cpu().numpy() for k, v in cols.items()}


def _same_columns(got, model, what):
    assert set(got) == set(model), what
    for col, want in model.items():
        have = got[col].view(want.dtype).reshape(want.shape)  # (torch has no unsigned 32 / 64 bit columns)
        assert have.tobytes() == want.tobytes(), f"{what}: column {col} differs in rows {np.flatnonzero((have != want).reshape(len(want), -1).any(axis=1))[:5]}"


def test_builder_refuses_level_ids_from_the_limit_on(dev):
    """``NSM_E_BADARG`` and a message that names the limit, for one id at 2^26 in 300 rows as for a table of images; the id
    below it builds; RAW rows stay unrestricted."""
    case = vr.set_builder_case(16, 16, levels=True)
    rc, _, n, cols = _build_set(dev, case["rows"], 16, 0, case["nlev"], case["plen"])
    assert rc == 0 and n == vr.BUILDER_ROWS and int(cols["ids"].max()) == vr.LEVELS_ID_LIMIT - 1
    rows = [list(r) for r in case["rows"]]
    at = next(k for k, r in enumerate(rows) if vr.LEVELS_ID_LIMIT - 1 in r)
    rows[at][rows[at].index(vr.LEVELS_ID_LIMIT - 1)] = vr.LEVELS_ID_LIMIT
    rc, message, _, _ = _build_set(dev, rows, 16, 0, case["nlev"], case["plen"])
    assert rc == BADARG and "2^26 (NSM_LEVELS_ID_LIMIT)" in message
    g = vr.grid(vr.LEVELS_IMAGES[0])
    for side, items in enumerate((g.left, g.right)):
        ids, plen, nlev = vr.nested_arrays(items, 16)
        rc, message, _, _ = _build_set(dev, ids.tolist(), 16, side, nlev.tolist(), plen.tolist())
        assert rc == BADARG and "2^26 (NSM_LEVELS_ID_LIMIT)" in message
        rc, _, n, cols = _build_set(dev, ids.tolist(), 16, side)  # the same rows as a RAW table
        assert rc == 0 and n == len(items)
    rc, _, _, cols = _build_set(dev, [[vr.INT32_MAX, -1, vr.P26, 5]], 16, 1)
    assert rc == 0 and cols["ids"][0, :4].tolist() == [5, vr.P26, vr.INT32_MAX, -2]


def test_encoders_refuse_level_ids_from_the_limit_on(dev):
    """The host path and the device path raise the same ``ValueError``, with the builder's words."""
    from napkon_string_matching_amd import tables

    messages = set()
    for name in (vr.LEVELS_IMAGES[0], vr.LEVELS_IMAGES[-1]):
        for device in ("cpu", dev):
            for side in ("left", "right"):
                with pytest.raises(ValueError, match=r"2\^26 \(NSM_LEVELS_ID_LIMIT\)") as err:
                    _nested_table(vr.grid(name), side, device, False)
                messages.add(str(err.value))
    assert len(messages) == 1
    rc, message, _, _ = _build_set(dev, [[vr.LEVELS_ID_LIMIT]], 16, 0, [1], [[1]])
    assert rc == BADARG and messages.pop() in message
    one = lambda v: tables.SetTable.from_nested_arrays(np.array([[7, v]], np.int32), np.array([[1, 2]], np.uint8), np.array([2]),
                                                        "right", dev, width=16)
    assert one(vr.LEVELS_ID_LIMIT - 1).ids[0, :3].tolist() == [7, vr.LEVELS_ID_LIMIT - 1, -2]
    with pytest.raises(ValueError):
        one(vr.LEVELS_ID_LIMIT)
    raw = tables.SetTable.from_padded(np.array([[vr.INT32_MAX, 5, vr.P26]], np.int32), "right", dev, width=16)
    assert raw.ids[0, :4].tolist() == [5, vr.P26, vr.INT32_MAX, -2]


# =========================================================================================================== Part B
RAW_STRING_CASES = [(n, r) for n in vr.RAW_STRINGS for r in RAW_INDEL_ROUTES[64 if "_str_64_" in n else 128]]


@pytest.mark.parametrize("name,route", RAW_STRING_CASES)
def test_indel_raw_grid_low_entropy(dev, name, route):
    """Stride 64: the thermometer codes' extremes (a bucket of 64, two symbols in one 16-bucket) through the two-stage,
    one-stage and unpruned routes.  Wider strides: the histogram bound over saturated counts."""
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    lt, rt = _raw_string_tables(g, dev)
    if g.size >= 256:
        assert int(lt.hist.max()) == 255 == int(rt.hist.max())
    kw = RAW_INDEL_ROUTES[64 if g.size == 64 else 128][route]
    _check_grid(g, vr.INDEL_THRESHOLDS, route, lambda thr: grid.indel_raw_grid(lt, rt, thr, capacity=g.pairs + 1, **kw).as_tuples())


@pytest.mark.parametrize("route", RAW_INDEL_ROUTES[128])
@pytest.mark.parametrize("name", vr.RAW_SATURATED)
def test_indel_raw_grid_saturated_tile(dev, name, route):
    """The wide RAW kernel skips a left row only when the histogram bound fails in every lane of a right tile; the last
    tile here holds nothing but near-copies of the left rows whose bucket count is 256 (saturated to 255 in the column)."""
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    lt, rt = _raw_string_tables(g, dev)
    assert int(lt.hist.max()) == 255
    kw = RAW_INDEL_ROUTES[128][route]
    _check_grid(g, vr.INDEL_THRESHOLDS, route, lambda thr: grid.indel_raw_grid(lt, rt, thr, capacity=g.pairs + 1, **kw).as_tuples())


@pytest.mark.parametrize("name", vr.RAW_STRINGS)
def test_indel_raw_queries_low_entropy(dev, name):
    """Runs of equal length are exact ties across rows and length classes: the rank cut of the top-k lists has to break them
    by j.  Top-k and grouped top-k (prune on and off, k = 1, 3, 64), profile, floor grid, pairs."""
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    lt, rt = _raw_string_tables(g, dev)
    groups = _groups(g)
    for route, prune in PRUNE.items():
        for grp in (None, groups):
            _check_top_k(g, vr.INDEL_THRESHOLDS, (1, 3, 64), f"top_k-{route}-{'plain' if grp is None else 'grouped'}",
                         lambda k, thr: grid.indel_raw_top_k(lt, rt, k, thr, prune=prune, groups=grp).as_tuples(), grp)
        _check_profile(g, vr.INDEL_THRESHOLDS, f"profile-{route}", lambda t: grid.indel_raw_profile(lt, rt, t, prune=prune))
        _check_floor_grid(g, vr.INDEL_THRESHOLDS, f"floor_grid-{route}",
                          lambda thr, lf, rf: grid.indel_raw_floor_grid(lt, rt, thr, lf, rf, prune=prune, capacity=g.pairs).as_tuples())
    _check_pairs(g, lambda i, j: grid.indel_raw_pairs(lt, rt, i, j))


LEVELS_STRING_ROUTES = {"default": {}, "park": dict(park=True), "wave_wide": dict(wave_wide=True), "no_prune": dict(prune=False)}


@pytest.mark.parametrize("route", LEVELS_STRING_ROUTES)
@pytest.mark.parametrize("name", vr.LEVELS_STRINGS)
def test_indel_levels_grid_low_entropy(dev, name, route):
    """The tile, park and finish kernels use the L1 histogram bound at strides 256 and 512 without a guard: valid under
    saturation, and pinned here on step-1 strings whose buckets pass 255."""
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    tabs = _levels_string_tables(g, dev)
    kw = LEVELS_STRING_ROUTES[route]
    _check_grid(g, vr.INDEL_THRESHOLDS, route, lambda thr: grid.indel_levels_grid(*tabs, thr, capacity=g.pairs + 1, **kw).as_tuples())


@pytest.mark.parametrize("name", vr.LEVELS_STRINGS)
def test_indel_levels_queries_low_entropy(dev, name):
    from napkon_string_matching_amd import grid

    g = vr.grid(name)
    tabs = _levels_string_tables(g, dev)
    for route, prune in PRUNE.items():
        _check_top_k(g, vr.INDEL_THRESHOLDS, (1, 3, 64), f"top_k-{route}",
                     lambda k, thr: grid.indel_levels_top_k(*tabs, k, thr, prune=prune).as_tuples())
        _check_profile(g, vr.INDEL_THRESHOLDS[:4], f"profile-{route}", lambda t: grid.indel_levels_profile(*tabs, t, prune=prune))
        _check_floor_grid(g, vr.INDEL_THRESHOLDS, f"floor_grid-{route}",
                          lambda thr, lf, rf: grid.indel_levels_floor_grid(*tabs, thr, lf, rf, prune=prune, capacity=g.pairs).as_tuples())
    _check_pairs(g, lambda i, j: grid.indel_levels_pairs(*tabs, i, j))


# =========================================================================================================== Part C
MAX_LEVELS_OF = {4: 1, 16: 4, 40: 7, 100: 5}


@pytest.mark.parametrize("width", [16, 32, 64])
@pytest.mark.parametrize("width_in", [4, 16, 40, 100])
def test_set_builder_input_clauses(dev, width_in, width):
    """Ids in any slots between -1, -2, -7 and INT32_MIN, ``width_in`` narrower and wider than the table, RAW rows with
    repeated ids, ``plen`` with garbage past the last level, ``orig`` NULL and given (INT32_MAX among its values)."""
    for side in (0, 1):
        case = vr.set_builder_case(width_in, width, levels=False, seed=side)
        orig = case["orig"] if side == 0 else None
        rc, message, n, cols = _build_set(dev, case["rows"], width, side, orig=orig)
        assert rc == 0 and n == vr.BUILDER_ROWS, message
        _same_columns(cols, vr.set_table_model(case["rows"], width, side, orig=orig), f"RAW {width_in} -> {width} side {side}")
        case = vr.set_builder_case(width_in, width, levels=True, max_levels=MAX_LEVELS_OF[width_in], seed=side)
        orig, cat = (case["orig"], None) if side == 1 else (None, case["cat"])
        rc, message, n, cols = _build_set(dev, case["rows"], width, side, case["nlev"], case["plen"], cat, orig)
        assert rc == 0 and n == vr.BUILDER_ROWS, message
        _same_columns(cols, vr.set_table_model(case["rows"], width, side, case["nlev"], case["plen"], cat, orig),
                      f"levels {width_in} -> {width} side {side}")


def test_builders_on_one_row(dev):
    rows = [[-7, 9, vr.INT32_MIN, 9, 2, -2]]
    rc, _, n, cols = _build_set(dev, rows, 16, 1, orig=[vr.INT32_MAX])
    assert rc == 0 and n == 1
    _same_columns(cols, vr.set_table_model(rows, 16, 1, orig=[vr.INT32_MAX]), "RAW, one row")
    rc, _, n, cols = _build_set(dev, [[-1, 9, -2, 2]], 32, 0, [2], [[1, 2, 0]], [1 << 63])
    assert rc == 0 and n == 1
    _same_columns(cols, vr.set_table_model([[-1, 9, -2, 2]], 32, 0, [2], [[1, 2, 0]], [1 << 63]), "levels, one row")
    for sort in (True, False):
        codes = [[3] * 200 + [77] * 56]
        rc, _, n, cols = _build_str(dev, codes, [200], 40, sort, [vr.INT32_MAX])
        assert rc == 0 and n == 1
        _same_columns(cols, vr.str_table_model(codes, [200], 40, sort, [vr.INT32_MAX]), f"strings, one row, sort={sort}")


@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "input_order"])
@pytest.mark.parametrize("stride,alphabet", [(64, 40), (128, 7), (256, 255), (256, 3), (512, 2)])
def test_str_builder_input_clauses(dev, stride, alphabet, sort):
    """Bytes >= alphabet past the length, lengths 0 and ``stride``, buckets beyond 255, both row orders; stride 256."""
    case = vr.str_builder_case(stride, alphabet)
    orig = case["orig"] if sort else None
    rc, message, n, cols = _build_str(dev, case["codes"], case["lengths"], alphabet, sort, orig)
    assert rc == 0 and n == vr.BUILDER_ROWS, message
    _same_columns(cols, vr.str_table_model(case["codes"], case["lengths"], alphabet, sort, orig), f"stride {stride} sort={sort}")
