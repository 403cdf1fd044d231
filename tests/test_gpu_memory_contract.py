"""The memory contract of every header include/nsm_hip*.h, entry by entry, inside a guard-band arena
(tests/support/arena.py): the 29 entries of nsm_hip.h against the oracle; the nine nsm_set_* and the nine nsm_edit_* entries
of the additive headers through the same case runners, under every measure and metric but the forwarding code 0, against the
plain-Python definitions; nsm_support_hits.  nsm_assign_hits, nsm_group_hits and nsm_span_hits have arena tests of their own
(the catalogue at the end checks that they still do).

Every other file of the suite compares results with the oracle and gives each buffer a ``torch`` tensor of its own: the
allocator rounds it up to 512 bytes, places nothing right behind it, and most outputs start as zeros.  A record written one
slot past ``capacity``, a queue half one entry too long, a builder column one row too long or an output the entry forgot to
initialise would pass all of them.  Here every table is re-homed into ONE tensor of seeded random bytes, every output is
carved at exactly the size the header states -- the hit counter as an 8-byte region of its own, never next to the records --
and the entry is called through ``ctypes``.  After the stream has drained, each case asserts

  (a) ``arena.check()``: no byte outside the carved regions changed (4096 guard bytes on both sides of every region);
  (b) every input region is byte-identical (the header types them ``const``);
  (c) every byte the header defines equals what the oracle gives;
  (d) every byte the header says is left alone still holds the arena's random bytes.

Bytes the header leaves undefined (top-k records beyond ``*out_count``, the split path's workspace) are not asserted.
tests/test_cpu_memory_contract.py checks the arena itself and the premises of these cases without a GPU.
"""
import copy
import ctypes
import re
import zlib
from pathlib import Path

import numpy as np
import pytest

from support import any_operands as ao
from support import arena as ar
from support import edge_support as es
from support import measure_probes as mp
from support import memory_cases as mc
from support import probe_tables
from support import threshold_probes as tp


pytestmark = pytest.mark.gpu

HEADERS = sorted((Path(__file__).resolve().parent.parent / "include").glob("nsm_hip*.h"))
NSM_E_BADARG = 10001  # include/nsm_hip.h
COVERED = {}  # C entry -> the tests that cover it


def covers(*entries):
    def mark(fn):
        for e in entries:
            COVERED.setdefault(e, []).append(fn.__name__)
        return fn

    return mark


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _stream(dev):
    import torch

    return torch.cuda.current_stream(dev).cuda_stream


def _sync(dev):
    import torch

    torch.cuda.synchronize(dev)


def _lib():
    from napkon_string_matching_amd import _lib as lib_module

    return lib_module, lib_module.load()


def _ok(rc, what):
    lib_module, lib = _lib()
    assert rc == 0, f"{what}: status {rc}: {lib.nsm_last_error()}"


def _tuples(rec: np.ndarray):
    """[n][2] float64 records -> (score, i, j)."""
    ij = rec.view(np.int32).reshape(-1, 4)
    return list(zip(rec[:, 0].tolist(), ij[:, 2].tolist(), ij[:, 3].tolist()))


def _canonical(hits):
    return sorted(hits, key=lambda h: (-h[0], h[1], h[2]))


def _arena(what, dev, nbytes):
    return ar.Arena(int(nbytes) + 16 * ar.GUARD, dev, seed=zlib.crc32(what.encode()))


def _put(arena, name, tensor):
    """An input column that is no part of a table: carved at its exact size and filled.  Returns its device address."""
    arena.carve(name, tensor.numel() * tensor.element_size())
    arena.fill(name, tensor)
    return arena.ptr(name)


def _region_bytes(*sizes):
    return sum(int(s) + ar.GUARD + ar.ALIGN for s in sizes)


def _with_caller_ids(table):
    """The table with caller ids that have gaps: row r reports ``mc.caller_id`` of what it reported."""
    out = copy.copy(table)
    out.orig = table.orig * 3 + 2
    return out


# ----------------------------------------------------------------------------------- hit lists: threshold and floor grids
def _check_hit_entry(dev, what, tables, prepare, want, extra_bytes=0, run_bytes=0):
    """``tables``: prefix -> table (re-homed here).  ``prepare(homed, arena)`` carves further inputs and returns
    ``call(hits_ptr, capacity, count_ptr, run, arena) -> status``.  One launch per capacity of ``mc.capacities`` with the
    counter zeroed, and one into a buffer that already counts ``mc.START_COUNT`` records."""
    want_set = set(want)
    assert len(want_set) == len(want) > max(mc.SMALL_CAPACITIES)
    runs = [(cap, 0) for cap in mc.capacities(len(want))] + [(len(want) + mc.START_COUNT - 2, mc.START_COUNT)]
    arena = _arena(what, dev, ar.table_bytes(*tables.values()) + extra_bytes +
                   sum(_region_bytes(cap * 16, 8, run_bytes, 32) for cap, _ in runs))
    homed = {prefix: ar.rehome(t, arena, prefix) for prefix, t in tables.items()}
    call = prepare(homed, arena)
    inputs = list(arena.regions)
    for run, (cap, start) in enumerate(runs):
        hname, cname = f"hits@{run}", f"count@{run}"
        arena.carve(hname, cap * 16)
        arena.carve(cname, 8)
        arena.fill(cname, np.array([start], dtype=np.uint64))
        _ok(call(arena.ptr(hname) if cap else 0, cap, arena.ptr(cname), run, arena), f"{what} capacity {cap}")
        _sync(dev)
        where = f"{what}, capacity {cap}, counter from {start}"
        arena.check(unchanged=inputs)                                                          # (a), (b)
        assert int(arena.read(cname, np.uint64)[0]) == start + len(want), where              # (c) it keeps counting
        live = min(cap, start + len(want))
        now, was = arena.read(hname), arena.poison(hname)
        got = _tuples(now[start * 16: live * 16].view(np.float64).reshape(-1, 2))
        assert len(set(got)) == len(got) and set(got) <= want_set, \
            f"{where}: {len(got) - len(set(got))} repeated records, not in the oracle's list: {sorted(set(got) - want_set)[:4]}"
        if cap >= start + len(want):
            assert _canonical(got) == want, where
        # (d) records already counted and the room beyond the last record: as they were
        assert now[: start * 16].tobytes() == was[: start * 16].tobytes(), f"{where}: records in front of the counter's start written"
        assert now[live * 16:].tobytes() == was[live * 16:].tobytes(), f"{where}: bytes behind the last record written"
    return arena


def _plain_grid(entry, prefixes, middle):
    """``prepare`` of an entry that takes its tables, ``middle`` (threshold, [mode,] flags) and the grid tail."""
    def prepare(homed, arena):
        lib = _lib()[1]
        structs = [homed[p].struct() for p in prefixes]
        stream = _stream(arena.buf.device)
        return lambda hits, cap, count, run, arena: getattr(lib, entry)(*structs, *middle, hits, cap, count, stream)

    return prepare


def _flags(**names):
    lib_module = _lib()[0]
    out = 0
    for name, on in names.items():
        if on:
            out |= getattr(lib_module, "FLAG_" + name.upper())
    return out


RAW_JACCARD_ROUTES = {"local": dict(prune=True, no_index=True), "exhaustive": dict(no_index=True),
                      "index_tile": dict(prune=True, index=True, tile_index=True),
                      "index_global_fold": dict(prune=True, index=True), "index_global_compact": dict(prune=True, index=True),
                      "index_global_64bit": dict(prune=True, index=True)}
POST_FORMAT = {"index_global_compact": 1, "index_global_64bit": 0}  # (every other route: the default, 2)


def _raw_jaccard_tables(g, dev, fmt):
    from napkon_string_matching_amd import tables

    if fmt == 2:
        return probe_tables.raw_jaccard_tables(g, dev)

    def make():
        keep = tables.COMPACT_POSTINGS, tables.RAW_POST_FORMAT
        tables.COMPACT_POSTINGS, tables.RAW_POST_FORMAT = fmt != 0, 1
        try:
            padded = np.full((len(g.left) + len(g.right), g.size), -1, dtype=np.int32)
            for r, row in enumerate(g.left + g.right):
                padded[r, : len(row)] = row
            lt = tables.SetTable.from_padded(padded[: len(g.left)], "left", dev, width=g.size)
            rt = tables.SetTable.from_padded(padded[len(g.left):], "right", dev, width=g.size)
        finally:
            tables.COMPACT_POSTINGS, tables.RAW_POST_FORMAT = keep
        assert rt.post is not None and rt.post_format == fmt
        return lt, rt

    return probe_tables.cached((g.name, "post_format", fmt), make)


@covers("nsm_jaccard_raw_grid")
@pytest.mark.parametrize("name,route", [(n, r) for n in tp.RAW_JACCARD for r in RAW_JACCARD_ROUTES
                                        if not (r == "index_tile" and n.endswith("_64"))])
def test_jaccard_raw_grid(dev, name, route):
    """The signature kernel, the per-tile LDS index and the global index in its three posting formats."""
    g = tp.grid(name)
    thr, want = mc.hit_case(name)
    lt, rt = _raw_jaccard_tables(g, dev, POST_FORMAT.get(route, 2))
    _check_hit_entry(dev, f"nsm_jaccard_raw_grid {name} {route}", {"left": lt, "right": rt},
                     _plain_grid("nsm_jaccard_raw_grid", ("left", "right"), (thr, _flags(**RAW_JACCARD_ROUTES[route]))), want)


RAW_INDEL_ROUTES = {64: {"two_stage": dict(prune=True), "one_stage": dict(prune=True, one_stage=True), "exhaustive": {}},
                    128: {"prune": dict(prune=True), "exhaustive": {}}}


@covers("nsm_indel_raw_grid")
@pytest.mark.parametrize("name,route", [(n, r) for n in tp.RAW_INDEL for r in RAW_INDEL_ROUTES[64 if n.endswith("_64") else 128]])
def test_indel_raw_grid(dev, name, route):
    """Stride 64: the two-stage scan, the one-stage scan and the exhaustive kernel; the wide kernels at 128, 256 and 512."""
    g = tp.grid(name)
    thr, want = mc.hit_case(name)
    lt, rt = probe_tables.raw_indel_tables(g, dev)
    flags = _flags(**RAW_INDEL_ROUTES[64 if g.size == 64 else 128][route])
    _check_hit_entry(dev, f"nsm_indel_raw_grid {name} {route}", {"left": lt, "right": rt},
                     _plain_grid("nsm_indel_raw_grid", ("left", "right"), (thr, flags)), want)


LEVELS_JACCARD_ROUTES = {f"{'prune' if prune else 'no_prune'}-index_{label}": dict(prune=prune, **index)
                         for prune in (True, False)
                         for label, index in (("auto", {}), ("never", dict(no_index=True)), ("global", dict(index=True)),
                                              ("tile", dict(index=True, tile_index=True)))}


@covers("nsm_jaccard_levels_grid")
@pytest.mark.parametrize("route", LEVELS_JACCARD_ROUTES)
@pytest.mark.parametrize("name", tp.LEVELS_JACCARD)
def test_jaccard_levels_grid(dev, name, route):
    g = tp.grid(name)
    thr, want = mc.hit_case(name)
    lt, rt = probe_tables.levels_jaccard_tables(g, dev, g.partition)
    middle = (thr, int(lt.category_mode), _flags(**LEVELS_JACCARD_ROUTES[route]))
    _check_hit_entry(dev, f"nsm_jaccard_levels_grid {name} {route}", {"left": lt, "right": rt},
                     _plain_grid("nsm_jaccard_levels_grid", ("left", "right"), middle), want)


# (at the low threshold of these cases NSM_FLAG_PRUNE alone, or no flag, is routed to the tile kernel: "tile" is that path)
ONE_WORD_ROUTES = {"wave_wide": dict(prune=True, wave_wide=True), "park": dict(prune=True, park=True),
                   "tile": dict(prune=True, tile=True), "split": dict(prune=True, split=True)}
MULTI_WORD_ROUTES = {"shared_tile": dict(prune=True), "park": dict(prune=True, park=True), "wave_wide": dict(prune=True, wave_wide=True)}
LEVELS_PREFIXES = ("left", "left_strings", "right", "right_strings")


def _levels_indel(dev, name, route, flags):
    """``nsm_indel_levels_grid`` with the workspace the library asks for (expected survivors: every pair), carved anew and
    left full of random bytes for every launch."""
    import torch

    g = tp.grid(name)
    thr, want = mc.hit_case(name)
    tabs = dict(zip(LEVELS_PREFIXES, probe_tables.levels_indel_tables(g, dev, g.partition)))
    lib = _lib()[1]
    mode = int(tabs["left"].category_mode if tabs["left"].category_mode is not None else g.mode)
    asked = int(lib.nsm_indel_levels_workspace_bytes(*[tabs[p].struct() for p in LEVELS_PREFIXES], thr, flags, float(g.pairs)))
    assert asked >= 1024 or route != "split"
    overflow = []

    def prepare(homed, arena):
        structs = [homed[p].struct() for p in LEVELS_PREFIXES]
        stream = _stream(dev)

        def call(hits, cap, count, run, arena):
            ws = 0
            if asked:
                arena.carve(f"workspace@{run}", asked)
                ws = arena.ptr(f"workspace@{run}")
            rc = lib.nsm_indel_levels_grid(*structs, thr, mode, flags, hits, cap, count, ws, asked, float(g.pairs), stream)
            if asked:
                _sync(dev)
                overflow.append(int(arena.read(f"workspace@{run}", np.uint64)[1]) & 0xFFFFFFFF)
            return rc

        return call

    try:
        _check_hit_entry(dev, f"nsm_indel_levels_grid {name} {route}", tabs, prepare, want, run_bytes=asked)
        if route == "split":
            assert overflow and not any(overflow), "the survivor queue overflowed: the split path did not produce the hits"
    finally:
        torch.cuda.synchronize(dev)
        assert lib.nsm_release(_stream(dev)) == 0  # the side stream and events of the split path


@covers("nsm_indel_levels_grid")
@pytest.mark.parametrize("route", ONE_WORD_ROUTES)
@pytest.mark.parametrize("name", tp.ONE_WORD)
def test_indel_levels_grid_one_word(dev, name, route):
    """The wave-wide kernel, the block-cooperative park kernel, the tile kernel, and the split path with the workspace it
    asks for."""
    _levels_indel(dev, name, route, _flags(**ONE_WORD_ROUTES[route]))


@covers("nsm_indel_levels_grid")
@pytest.mark.parametrize("route", MULTI_WORD_ROUTES)
@pytest.mark.parametrize("name", tp.MULTI_WORD)
def test_indel_levels_grid_multi_word(dev, name, route):
    _levels_indel(dev, name, route, _flags(**MULTI_WORD_ROUTES[route]))


def _any_operands(g, dev):
    """The operands of wide.indel_any_grid / wide.jaccard_any_grid: (struct, tensors) per argument, mode, flags."""
    from napkon_string_matching_amd import _lib as lib_module
    from napkon_string_matching_amd import wide

    left, right = ao.kernel_operands(g)
    use_cat = g.mode != lib_module.CAT_NONE
    flags = lib_module.FLAG_RAW_SCORE if g.raw else 0
    if g.kind == "indel":
        symbols = sorted({ch for items in (left, right) for it in items for s in it for ch in s})
        lut = {ch: k for k, ch in enumerate(symbols)}
        out = {}
        for side, items, cat in (("left", left, g.cat_l), ("right", right, g.cat_r)):
            strings, keep = wide._any_strings(items, lut, max(1, len(symbols)), dev)
            if use_cat:
                keep["cat"] = wide._dev(np.asarray(cat, dtype=np.uint64).view(np.int64), dev)
            items_struct = lib_module.NsmAnyItems(keep["first"].data_ptr(), keep["nlev"].data_ptr(), keep["orig"].data_ptr(),
                                                  keep["cat"].data_ptr() if use_cat else None, len(items))
            item_cols = {k: keep[k] for k in ("first", "nlev", "orig", "cat") if k in keep}
            out[side] = (items_struct, item_cols)
            out[side + "_strings"] = (strings, {k: keep[k] for k in ("codes", "offset")})
        return out, ("left", "left_strings", "right", "right_strings"), g.mode if use_cat else 0, flags
    deepest = max(max(len(it) for it in left), max(len(it) for it in right), 1)
    independent = deepest > wide.FAST_LEVELS or not all(wide._nested(it) for items in (left, right) for it in items)
    assert ("independent" if independent else "nested") == g.layout
    vocab = {}
    out = {"left": wide._any_sets(left, vocab, deepest, dev, g.cat_l if use_cat else None, independent),
           "right": wide._any_sets(right, vocab, deepest, dev, g.cat_r if use_cat else None, independent)}
    return out, ("left", "right"), g.mode if use_cat else 0, flags


@covers("nsm_indel_any_grid", "nsm_jaccard_any_grid")
@pytest.mark.parametrize("name", mc.ANY_GRIDS)
def test_any_grids(dev, name):
    g = ao.grid(name)
    thr, want = mc.any_case(name)
    operands, prefixes, mode, flags = _any_operands(g, dev)
    entry = "nsm_indel_any_grid" if g.kind == "indel" else "nsm_jaccard_any_grid"

    def prepare(homed, arena):
        lib = _lib()[1]
        structs = [homed[p][0] for p in prefixes]
        stream = _stream(dev)
        return lambda hits, cap, count, run, arena: getattr(lib, entry)(*structs, thr, int(mode), flags, hits, cap, count, stream)

    _check_hit_entry(dev, f"{entry} {name}", operands, prepare, want)


def _one_row_tables(g, dev):
    """prefix -> table of a grid for the entries that want ONE row per item (no partition), caller ids as they are."""
    if g.kind == "indel" and g.raw:
        return dict(zip(("left", "right"), probe_tables.raw_indel_tables(g, dev)))
    if g.kind == "jaccard" and g.raw:
        return dict(zip(("left", "right"), mp.raw_tables(g, dev)))  # (the probe grid's tables, or those of a measure's view of it)
    if g.kind == "indel":
        return dict(zip(LEVELS_PREFIXES, probe_tables.levels_indel_tables(g, dev, False)))
    return dict(zip(("left", "right"), probe_tables.levels_jaccard_tables(g, dev, False)))


def _item_tables(tabs):
    """The two tables whose ``orig`` are the caller ids."""
    return tabs["left"], tabs["right"]


def _mode_of(tabs, g):
    left = tabs["left"]
    return int(left.category_mode if getattr(left, "category_mode", None) is not None else g.mode)


@covers("nsm_indel_raw_floor_grid", "nsm_jaccard_raw_floor_grid", "nsm_indel_levels_floor_grid", "nsm_jaccard_levels_floor_grid")
@pytest.mark.parametrize("entry", mc.FLOOR_GRIDS)
def test_floor_grids(dev, entry):
    """Both floors, indexed by caller ids with gaps (3 k + 2); the floor columns are inputs and stay as they are; ``stats``
    is added to on every other launch and NULL on the rest."""
    _floor_grid_case(dev, entry, mc.FLOOR_GRIDS[entry])


def _code(variant):
    """The argument an entry of an additive header takes behind its last table: the measure or metric."""
    return () if variant is None else (mc.CODE[variant],)


def _floor_grid_case(dev, entry, name, variant=None):
    import torch

    lib_module, lib = _lib()
    g = mc.view(name, variant)
    thr, lf, rf, want = mc.floor_case(name, variant)
    tabs = _one_row_tables(g, dev)
    tabs["left"], tabs["right"] = _with_caller_ids(tabs["left"]), _with_caller_ids(tabs["right"])
    prefixes = list(tabs)
    middle = (lib_module.FLAG_PRUNE,) if g.raw else (_mode_of(tabs, g), lib_module.FLAG_PRUNE, 0, 0)
    stats_seen = []

    def prepare(homed, arena):
        structs = [homed[p].struct() for p in prefixes]
        lfp, rfp = _put(arena, "left_floor", torch.from_numpy(lf)), _put(arena, "right_floor", torch.from_numpy(rf))
        stream = _stream(dev)

        def call(hits, cap, count, run, arena):
            st = 0
            if run % 2:
                arena.carve(f"stats@{run}", 32)
                arena.fill(f"stats@{run}", np.array([11, 12, 13, 14], dtype=np.uint64))
                st = arena.ptr(f"stats@{run}")
            rc = getattr(lib, entry)(*structs, *_code(variant), thr, lfp, rfp, *middle, hits, cap, count, st, stream)
            if st:
                _sync(dev)
                stats_seen.append(arena.read(f"stats@{run}", np.uint64).tolist())
            return rc

        return call

    what = f"{entry} {g.name}" + (f" {variant}" if variant else "")
    _check_hit_entry(dev, what, tabs, prepare, want, extra_bytes=_region_bytes(lf.nbytes, rf.nbytes))
    assert stats_seen and all(all(a >= b for a, b in zip(s, (11, 12, 13, 14))) and s[0] >= 11 + len(want) for s in stats_seen)


@covers(*{e for e, _, _ in mc.additive(mc.FLOOR_GRIDS)})
@pytest.mark.parametrize("entry,sibling,variant", mc.additive(mc.FLOOR_GRIDS))
def test_floor_grids_of_the_additive_headers(dev, entry, sibling, variant):
    """``nsm_set_*_floor_grid`` under Dice, overlap and containment and ``nsm_edit_*_floor_grid`` under both Levenshtein
    metrics: the sibling's grid, capacities, caller ids and ``stats`` runs, the code behind the last table; the expected
    records are the definition's (tests/support/set_measures.py, edit_distance.py)."""
    _floor_grid_case(dev, entry, mc.FLOOR_GRIDS[sibling], variant)


# ------------------------------------------------------------------------------------------------- split-path workspace
@covers("nsm_indel_levels_workspace_bytes")
@pytest.mark.parametrize("name", tp.ONE_WORD)
def test_split_workspace_of_any_size(dev, name):
    """"ANY size is safe", "reads nothing from it on entry": the forced split path with workspaces of 1024 bytes, of
    512 + 16 * 100, of what the library asks for, and of 8 bytes more or less -- sizes that are no multiple of the 16 bytes
    two queue entries take.  The workspace is random bytes on entry and its guard is intact afterwards; the hits are the
    park kernel's and the oracle's.  The small queues overflow, the recommended one does not -- and the overflow word is set
    exactly when a round's queue counter (it keeps counting) exceeds the entries of a half.

    A wave appends its survivors to the queue in one batch, and only when the whole batch fits -- so none of those sizes
    makes a wave write the LAST entry of the second half, the one that ends the workspace.  Two more sizes do, by
    construction: with two rounds (expected survivors = 1.5 queue halves) the second round fills the second half; its
    survivor count S is read from the queue counter of a first call, and the halves are then given S entries (the second
    half is filled to its last entry: no overflow there, guard intact) and S - 1 entries (one short: overflow)."""
    import torch

    from napkon_string_matching_amd import grid

    lib_module, lib = _lib()
    g = tp.grid(name)
    thr, want = mc.hit_case(name)
    raw_tabs = probe_tables.levels_indel_tables(g, dev, g.partition)
    tabs = dict(zip(LEVELS_PREFIXES, raw_tabs))
    park = grid.indel_levels_grid(*raw_tabs, thr, category_mode=g.mode, capacity=g.pairs + 1, park=True).as_tuples()
    assert park == want
    flags = lib_module.FLAG_PRUNE | lib_module.FLAG_SPLIT
    mode = _mode_of(tabs, g)
    asked = int(lib.nsm_indel_levels_workspace_bytes(*[tabs[p].struct() for p in LEVELS_PREFIXES], thr, flags, float(g.pairs)))
    assert asked >= 512 + 16 * 65536 and (asked - 512) % 16 == 0
    cap = len(want) + 1
    arena = _arena(f"workspace {name}", dev, ar.table_bytes(*tabs.values()) + 12 * _region_bytes(asked, cap * 16, 8))
    homed = {p: ar.rehome(t, arena, p) for p, t in tabs.items()}
    structs = [homed[p].struct() for p in LEVELS_PREFIXES]
    inputs = list(arena.regions)
    runs = []

    def launch(nbytes, expected):
        """One call with a workspace of ``nbytes`` random bytes; (a), (b), the hits.  Returns the control words."""
        tag = len(runs)
        runs.append(nbytes)
        arena.carve(f"workspace@{tag}", nbytes)
        arena.carve(f"hits@{tag}", cap * 16)
        arena.carve(f"count@{tag}", 8)
        arena.zero(f"count@{tag}")
        _ok(lib.nsm_indel_levels_grid(*structs, thr, mode, flags, arena.ptr(f"hits@{tag}"), cap, arena.ptr(f"count@{tag}"),
                                      arena.ptr(f"workspace@{tag}"), nbytes, float(expected), _stream(dev)), name)
        _sync(dev)
        arena.check(unchanged=inputs)
        assert int(arena.read(f"count@{tag}", np.uint64)[0]) == len(want), nbytes
        rec = arena.read(f"hits@{tag}", np.float64).reshape(-1, 2)
        assert _canonical(_tuples(rec[: len(want)])) == park, nbytes
        assert arena.read(f"hits@{tag}")[len(want) * 16:].tobytes() == arena.poison(f"hits@{tag}")[len(want) * 16:].tobytes()
        ctl = arena.read(f"workspace@{tag}")[:512].view(np.uint64)
        return int(ctl[1]) & 0xFFFFFFFF, [int(v) for v in ctl[2:64]]

    try:
        for nbytes in (1024, 1024 + 8, 512 + 16 * 100, 512 + 16 * 100 + 8, asked - 8, asked):
            overflowed, counters = launch(nbytes, g.pairs)
            assert overflowed == (0 if nbytes >= asked - 8 else 1), (nbytes, overflowed)
            assert overflowed == int(any(c > (nbytes - 512) // 16 for c in counters)), (nbytes, counters[:4])  # (they keep counting)
        # two rounds, whatever the queue's size: 1 <= expected / entries < 2
        entries = (asked - 512) // 16
        overflowed, counters = launch(asked, 1.5 * entries)
        first, second = counters[0], counters[1]
        assert overflowed == 0 and first > 32 and not any(counters[2:]), counters[:4]
        if not g.partition:  # (83 left rows without a partition are two slices; the partitioned grid here is one, so it
            assert second > 32  # runs one round and never uses the second half)
        if second > 32:
            for entries, nbytes in ((second, 512 + 16 * second), (second, 512 + 16 * second + 8),
                                    (second - 1, 512 + 16 * (second - 1)), (second - 1, 512 + 16 * (second - 1) + 8)):
                overflowed, again = launch(nbytes, 1.5 * entries)
                assert again[:3] == [first, second, 0], (again[:3], first, second)  # the same two rounds
                assert overflowed == int(first > entries or second > entries), (nbytes, overflowed, first, second)
    finally:
        torch.cuda.synchronize(dev)
        assert lib.nsm_release(_stream(dev)) == 0


# ----------------------------------------------------------------------------------------------------------------- top-k
@covers("nsm_indel_raw_top_k", "nsm_jaccard_raw_top_k", "nsm_indel_raw_top_k_grouped", "nsm_jaccard_raw_top_k_grouped",
        "nsm_indel_levels_top_k", "nsm_jaccard_levels_top_k")
@pytest.mark.parametrize("entry", mc.TOP_K_GRIDS)
def test_top_k(dev, entry):
    """``out`` at exactly ``left->n * min(k, right->n)`` records (the entry clamps k; the host allocates that much) and
    ``stats`` at 32 bytes; rows with no record, with fewer than k and with more; the levels entries with a category
    predicate and a blacklist.  A run with ``stats = NULL`` and one with it give the same records; ``stats`` is added to."""
    _top_k_case(dev, entry, mc.TOP_K_GRIDS[entry])


@covers(*{e for e, _, _ in mc.additive(mc.TOP_K_GRIDS)})
@pytest.mark.parametrize("entry,sibling,variant", mc.additive(mc.TOP_K_GRIDS))
def test_top_k_of_the_additive_headers(dev, entry, sibling, variant):
    """The six ``nsm_set_*`` / ``nsm_edit_*`` top-k entries, plain, grouped (the code stands before ``right_group``) and
    levels with a category predicate and a blacklist, under every code but 0, against the definitions."""
    _top_k_case(dev, entry, mc.grid_name(mc.TOP_K_GRIDS, sibling, variant), variant)


def _top_k_case(dev, entry, name, variant=None):
    import torch

    from napkon_string_matching_amd import grid

    lib_module, lib = _lib()
    g = mc.view(name, variant)
    thr, allowed, banned = mc.top_k_case(name, variant)
    tabs = _one_row_tables(g, dev)
    prefixes = list(tabs)
    left, right = _item_tables(tabs)
    grouped = entry.endswith("_grouped")
    groups = tp.groups_of(g) if grouped else None
    ranks = tp.RowRanks(allowed, None if groups is None else groups.tolist())
    bs, bj = grid.banned_csr(banned, len(g.left), dev)
    k_effs = [min(k, right.n) for k in mc.TOP_K]
    arena = _arena(entry + (f" {variant}" if variant else ""), dev,
                   ar.table_bytes(*tabs.values()) + _region_bytes(4 * len(g.right), 4 * (len(g.left) + 1), 8 * len(allowed)) +
                   sum(2 * _region_bytes(left.n * k * 16, 8, 32) for k in k_effs))
    homed = {p: ar.rehome(t, arena, p) for p, t in tabs.items()}
    structs = [homed[p].struct() for p in prefixes]
    front = (_put(arena, "right_group", torch.from_numpy(groups)),) if grouped else ()
    tail = () if g.raw else ((_put(arena, "banned_start", bs), _put(arena, "banned_j", bj)) if bs is not None else (0, 0))
    inputs = list(arena.regions)
    for k, k_eff in zip(mc.TOP_K, k_effs):
        want = ranks.cut(thr, k)
        assert len(want) <= left.n * k_eff
        seen = []
        for with_stats in (False, True):
            tag = f"{k}{'s' if with_stats else ''}"
            arena.carve(f"out@{tag}", left.n * k_eff * 16)
            arena.carve(f"count@{tag}", 8)
            arena.zero(f"count@{tag}")
            st = 0
            if with_stats:
                arena.carve(f"stats@{tag}", 32)
                arena.fill(f"stats@{tag}", np.array([11, 12, 13, 14], dtype=np.uint64))
                st = arena.ptr(f"stats@{tag}")
            middle = (thr, k, lib_module.FLAG_PRUNE) if g.raw else (thr, k, _mode_of(tabs, g), lib_module.FLAG_PRUNE, *tail)
            _ok(getattr(lib, entry)(*structs, *_code(variant), *front, *middle, arena.ptr(f"out@{tag}"), arena.ptr(f"count@{tag}"), st,
                                    _stream(dev)), f"{entry} {variant or ''} k={k}")
            _sync(dev)
            arena.check(unchanged=inputs)
            n = int(arena.read(f"count@{tag}", np.uint64)[0])
            assert n == len(want), (entry, k, n, len(want))
            got = _canonical(_tuples(arena.read(f"out@{tag}", np.float64).reshape(-1, 2)[:n]))
            assert got == want, f"{entry} k={k}: {probe_tables.first_difference(got, want)}"
            seen.append(got)
            if with_stats:
                after = arena.read(f"stats@{tag}", np.uint64).tolist()
                assert all(a >= b for a, b in zip(after, (11, 12, 13, 14))) and after[0] > 11, after
        assert seen[0] == seen[1]


# -------------------------------------------------------------------------------------------------------------- profiles
@covers("nsm_indel_raw_profile", "nsm_jaccard_raw_profile", "nsm_indel_levels_profile", "nsm_jaccard_levels_profile")
@pytest.mark.parametrize("empty", [None, "left", "right"])
@pytest.mark.parametrize("entry", mc.PROFILE_GRIDS)
def test_profiles(dev, entry, empty):
    """Caller ids with gaps (3 k + 2); ``left_best`` / ``right_best`` at largest id + 1 entries and ``pairs`` at T, all
    random bytes on entry: "the call initialises its outputs itself ... other entries stay as they are".  ``empty``: that
    side's table has no rows (its columns are still there) -- pairs are 0, the other side's entries -1.0."""
    _profile_case(dev, entry, mc.PROFILE_GRIDS[entry], empty)


@covers(*{e for e, _, _ in mc.additive(mc.PROFILE_GRIDS)})
@pytest.mark.parametrize("empty", [None, "left", "right"])
@pytest.mark.parametrize("entry,sibling,variant", mc.additive(mc.PROFILE_GRIDS))
def test_profiles_of_the_additive_headers(dev, entry, sibling, variant, empty):
    """``nsm_set_*_profile`` and ``nsm_edit_*_profile`` under every code but 0: the sibling's conditions, the definitions'
    pair counts and best scores."""
    _profile_case(dev, entry, mc.grid_name(mc.PROFILE_GRIDS, sibling, variant), empty, variant)


def _profile_case(dev, entry, name, empty, variant=None):
    lib_module, lib = _lib()
    g = mc.view(name, variant)
    ladder, pairs, best_l, best_r = mc.profile_case(name, variant)
    tabs = _one_row_tables(g, dev)
    tabs["left"], tabs["right"] = _with_caller_ids(tabs["left"]), _with_caller_ids(tabs["right"])
    prefixes = list(tabs)
    ids_l, ids_r = max(best_l) + 1, max(best_r) + 1
    if empty:
        pairs = [0] * len(ladder)
        best_l = {} if empty == "left" else {i: -1.0 for i in best_l}
        best_r = {} if empty == "right" else {j: -1.0 for j in best_r}
    arena = _arena(f"{entry} {empty}" + (f" {variant}" if variant else ""), dev,
                   ar.table_bytes(*tabs.values()) + _region_bytes(8 * len(ladder), 8 * ids_l, 8 * ids_r, 32))
    homed = {p: ar.rehome(t, arena, p) for p, t in tabs.items()}
    structs = {p: homed[p].struct() for p in prefixes}
    if empty:
        structs[empty].n = 0
    inputs = list(arena.regions)
    for name, nbytes in (("pairs", 8 * len(ladder)), ("left_best", 8 * ids_l), ("right_best", 8 * ids_r), ("stats", 32)):
        arena.carve(name, nbytes)
    arena.fill("stats", np.array([11, 12, 13, 14], dtype=np.uint64))
    t = (ctypes.c_double * len(ladder))(*ladder)
    middle = (lib_module.FLAG_PRUNE,) if g.raw else (_mode_of(tabs, g), lib_module.FLAG_PRUNE, 0, 0)
    _ok(getattr(lib, entry)(*structs.values(), *_code(variant), t, len(ladder), *middle, arena.ptr("pairs"), arena.ptr("left_best"),
                            arena.ptr("right_best"), arena.ptr("stats"), _stream(dev)), f"{entry} {variant or ''}")
    _sync(dev)
    arena.check(unchanged=inputs)
    assert arena.read("pairs", np.uint64).tolist() == pairs  # fully written
    for name, best in (("left_best", best_l), ("right_best", best_r)):
        now, was = arena.read(name, np.uint64), arena.poison(name, np.uint64)
        want = was.copy()
        for ident, score in best.items():
            want[ident] = np.float64(score).view(np.uint64)
        wrong = np.flatnonzero(now != want)
        assert wrong.size == 0, f"{entry} {name}: ids {wrong[:8].tolist()} (an id with k % 3 != 2 names no item and must stay as it was)"
    after = arena.read("stats", np.uint64).tolist()
    assert all(a >= b for a, b in zip(after, (11, 12, 13, 14))) and ((after[0] > 11) == (empty is None))


# ---------------------------------------------------------------------------------------------------------- listed pairs
@covers("nsm_indel_raw_pairs", "nsm_jaccard_raw_pairs", "nsm_indel_levels_pairs", "nsm_jaccard_levels_pairs")
@pytest.mark.parametrize("entry", mc.PAIRS_GRIDS)
def test_listed_pairs(dev, entry):
    """"the call writes pairs[p].score and nothing else": the i and j bytes of every record, the id -> row maps and the
    guard behind the last record stay as they are; duplicates, ids outside the maps and ids whose map entry is -1."""
    _pairs_case(dev, entry, mc.PAIRS_GRIDS[entry])


@covers(*{e for e, _, _ in mc.additive(mc.PAIRS_GRIDS)})
@pytest.mark.parametrize("entry,sibling,variant", mc.additive(mc.PAIRS_GRIDS))
def test_listed_pairs_of_the_additive_headers(dev, entry, sibling, variant):
    """``nsm_set_*_pairs`` and ``nsm_edit_*_pairs`` under every code but 0 on the sibling's grid and lists.  The grid keeps
    its empty rows: a pair whose measure divides by zero gets -1.0, as nsm_hip_measures.h says."""
    _pairs_case(dev, entry, mc.PAIRS_GRIDS[sibling], variant)


def _pairs_case(dev, entry, name, variant=None):
    import torch

    from napkon_string_matching_amd import grid

    lib = _lib()[1]
    g = tp.grid(name)
    tabs = _one_row_tables(g, dev)
    prefixes = list(tabs)
    left, right = _item_tables(tabs)
    lmap, rmap = grid._row_map(left.orig, left.n, dev).clone(), grid._row_map(right.orig, right.n, dev).clone()
    assert lmap.numel() == len(g.left) and rmap.numel() == len(g.right) and int(lmap.min()) >= 0
    lmap[list(mc.UNMAPPED_LEFT)] = -1
    rmap[list(mc.UNMAPPED_RIGHT)] = -1
    arena = _arena(entry + (f" {variant}" if variant else ""), dev,
                   ar.table_bytes(*tabs.values()) + _region_bytes(4 * lmap.numel(), 4 * rmap.numel()) +
                   sum(_region_bytes(16 * n) for n in mc.PAIR_COUNTS))
    homed = {p: ar.rehome(t, arena, p) for p, t in tabs.items()}
    structs = [homed[p].struct() for p in prefixes]
    lptr, rptr = _put(arena, "left_row", lmap), _put(arena, "right_row", rmap)
    inputs = list(arena.regions)
    for n_pairs in mc.PAIR_COUNTS:
        pairs = mc.pair_list(g, n_pairs)
        region = f"pairs@{n_pairs}"
        arena.carve(region, 16 * n_pairs)
        records = arena.poison(region, np.float64).reshape(-1, 2)  # (the scores stay random bytes)
        ij = records.view(np.int32).reshape(-1, 4)
        ij[:, 2], ij[:, 3] = [p[0] for p in pairs], [p[1] for p in pairs]
        arena.fill(region, records)
        _ok(getattr(lib, entry)(*structs, *_code(variant), lptr, int(lmap.numel()), rptr, int(rmap.numel()), arena.ptr(region), n_pairs,
                                _stream(dev)), f"{entry} {variant or ''}")
        _sync(dev)
        arena.check(unchanged=inputs)
        now = arena.read(region, np.float64).reshape(-1, 2)
        assert now.view(np.int32).reshape(-1, 4)[:, 2:].tobytes() == ij[:, 2:].tobytes(), f"{entry}: i / j of a record written"
        want = np.array(mc.pair_scores(g, pairs, variant), dtype=np.float64)
        wrong = np.flatnonzero(now[:, 0].view(np.uint64) != want.view(np.uint64))
        assert wrong.size == 0, f"{entry} n_pairs={n_pairs}: records {wrong[:6].tolist()}: got {now[wrong[:6], 0].tolist()}, " \
                                f"want {want[wrong[:6]].tolist()} for {[pairs[w] for w in wrong[:6]]}"


# ---------------------------------------------------------------------------------------------------------- edge support
def _support_call(dev, what, lists, nodes, min_score, min_support, with_stats):
    """One ``nsm_support_hits`` call with every list's records, ``support[l]`` at exactly ``lists[l].n`` words and
    ``stats`` at exactly 40 bytes (or NULL) in one arena.  Returns (status, arena, input regions)."""
    lib_module, lib = _lib()
    records = [mc.support_records(hits) for hits, _, _ in lists]
    arena = _arena(what, dev, _region_bytes(40, *[r.nbytes for r in records], *[4 * len(r) for r in records]))
    descs = (lib_module.NsmHitList * len(lists))()
    out = (ctypes.c_void_p * len(lists))()
    for k, (slot, rec, (_, left_base, right_base)) in enumerate(zip(descs, records, lists)):
        if len(rec):
            arena.carve(f"hits{k}", rec.nbytes)
            arena.fill(f"hits{k}", rec)
        slot.hits, slot.n = (arena.ptr(f"hits{k}") if len(rec) else None), len(rec)
        slot.left_base, slot.left_ids, slot.right_base, slot.right_ids = left_base, nodes - left_base, right_base, nodes - right_base
    inputs = list(arena.regions)
    for k, rec in enumerate(records):
        if len(rec):
            arena.carve(f"support{k}", 4 * len(rec))
        out[k] = arena.ptr(f"support{k}") if len(rec) else None
    st = 0
    if with_stats:
        arena.carve("stats", 40)
        arena.fill("stats", np.array(mc.SUPPORT_STATS_START, dtype=np.uint64))
        st = arena.ptr("stats")
    rc = lib.nsm_support_hits(descs, len(lists), nodes, float(min_score), min_support, out, st, _stream(dev))
    _sync(dev)
    return rc, arena, inputs


@covers("nsm_support_hits")
@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "stats_null"])
@pytest.mark.parametrize("min_support", [0, 1])
def test_support_hits(dev, min_support, with_stats):
    """include/nsm_hip_support.h: ``support[l]`` has ``lists[l].n`` words, ``stats`` five, ADDED to; the hit lists are
    inputs.  Four lists and one with ``n = 0`` (no records, no words: both pointers NULL); one counting pass and a peel."""
    from napkon_string_matching_amd import grid

    lists, nodes, min_score = mc.support_case()
    words, rounds = grid.truss_of_hits(lists, nodes, min_support, min_score)
    rc, arena, inputs = _support_call(dev, f"nsm_support_hits {min_support}", lists, nodes, min_score, min_support, with_stats)
    _ok(rc, f"nsm_support_hits min_support={min_support}")
    arena.check(unchanged=inputs)
    for k, want in enumerate(words):
        if len(want):
            got = arena.read(f"support{k}", np.int32)
            assert np.array_equal(got, want), f"list {k}: records {np.flatnonzero(got != want)[:6].tolist()}"
    if with_stats:
        edge_records, distinct = es.edge_counts(lists, nodes, min_score)
        total, alive = es.final_triangles_x3(lists, nodes, words)
        added = [edge_records, distinct, alive, rounds, total]
        assert arena.read("stats", np.uint64).tolist() == [a + b for a, b in zip(mc.SUPPORT_STATS_START, added)]


@covers("nsm_support_hits")
@pytest.mark.parametrize("side", ["i", "j", "negative"])
def test_support_hits_refuses_an_id_outside_its_list(dev, side):
    """The header's check on the device: an id outside ``[0, left_ids)`` / ``[0, right_ids)`` -- whatever the record's
    score -- returns NSM_E_BADARG BEFORE anything is written: ``support`` and ``stats`` still hold the arena's bytes."""
    lib_module, lib = _lib()
    lists, nodes, min_score = mc.support_case()
    lists = mc.support_case_with_bad_id(lists, nodes, side)
    rc, arena, inputs = _support_call(dev, f"nsm_support_hits bad {side}", lists, nodes, min_score, 1, True)
    assert rc == NSM_E_BADARG and b"outside" in lib.nsm_last_error(), (rc, lib.nsm_last_error())
    arena.check(unchanged=list(arena.regions))  # inputs, every support[l] and stats: as they were


# ------------------------------------------------------------------------------------------------------------------ sort
def _sort_case(dev, n, cap, id_limit, scratch, capture=False):
    import torch

    lib = _lib()[1]
    arena = _arena(f"sort {n} {cap} {id_limit}", dev, _region_bytes(cap * 16, 8, n * 16))
    rec = mc.sort_records(cap, n, 1000)
    arena.carve("hits", cap * 16)
    arena.fill("hits", rec)
    arena.carve("count", 8)
    arena.fill("count", np.array([n], dtype=np.uint64))
    sptr = 0
    if scratch:
        arena.carve("scratch", n * 16)  # exactly n records, as grid.sort_hits_device allocates with n_hint = n
        sptr = arena.ptr("scratch")
    if capture:
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                _ok(lib.nsm_sort_hits(arena.ptr("hits"), sptr, cap, arena.ptr("count"), n, id_limit, stream.cuda_stream), "nsm_sort_hits")
            graph.replay()
    else:
        _ok(lib.nsm_sort_hits(arena.ptr("hits"), sptr, cap, arena.ptr("count"), n, id_limit, _stream(dev)), "nsm_sort_hits")
    _sync(dev)
    arena.check(unchanged=["count"] + (["scratch"] if capture else []))
    now = arena.read("hits", np.float64).reshape(-1, 2)
    assert now[:n].tobytes() == mc.sorted_records(rec[:n]).tobytes(), f"n={n} id_limit={id_limit}: the first n records are not in canonical order"
    assert now[n:].tobytes() == rec[n:].tobytes(), f"n={n} capacity={cap}: records [n, capacity) written"


@covers("nsm_sort_hits")
@pytest.mark.parametrize("id_limit", [0, 1000])
@pytest.mark.parametrize("n,cap", mc.SORT_SIZES)
def test_sort_hits(dev, n, cap, id_limit):
    """``n < capacity`` live records on both sides of 8192 with ``n_hint = n``: ``scratch = NULL`` below, a scratch of
    exactly n records above ("with n_hint the sort touches at most n_hint records of it").  Records [n, capacity) and the
    guard behind the n-record scratch stay as they are."""
    _sort_case(dev, n, cap, id_limit, scratch=n > 8192)


def test_sort_hits_on_a_capturing_stream(dev):
    """The bitonic path of a captured call: no scratch record is needed, none is written."""
    _sort_case(dev, 8190, 8190 + 300, 0, scratch=False)  # (eager first: the kernel attribute is set outside a capture)
    n, cap = mc.SORT_SIZES[2]
    _sort_case(dev, n, cap, 1000, scratch=True, capture=True)


# -------------------------------------------------------------------------------------------------------------- builders
BUILD_ROWS = (1, 63, 64, 65, 3001)


def _carve_like(arena, prefix, table):
    """The table with every column an arena view of the same size, still random bytes: what a builder is handed."""
    out = copy.copy(table)
    for col, t in ar._tensors_of(table).items():
        setattr(out, col, arena.carve(f"{prefix}.{col}", t.numel() * t.element_size(), t.dtype, tuple(t.shape)))
    return out


def _pointers(struct, arena, prefix, table):
    """An empty column has no ``data_ptr``: name its region."""
    for col, t in ar._tensors_of(table).items():
        if t.numel() == 0 and hasattr(struct, col):
            setattr(struct, col, arena.ptr(f"{prefix}.{col}"))
    return struct


def _same_columns(arena, prefix, want, what):
    for col, t in ar._tensors_of(want).items():
        got = arena.read(f"{prefix}.{col}")
        assert got.tobytes() == t.contiguous().numpy().tobytes(), f"{what}: column {col} differs from the numpy encoder"


SET_TABLE_CASES = {"raw-left": dict(side="left"), "raw-right-fold": dict(side="right", fmt=2), "raw-right-compact": dict(side="right", fmt=1),
                   "raw-right-64bit": dict(side="right", fmt=0), "raw-right-no_index": dict(side="right", index=False),
                   "levels-plain": dict(side="left", mode=0), "levels-partition": dict(side="right", mode=1, partition=True, fmt=1),
                   "levels-partition-64bit": dict(side="right", mode=1, partition=True, fmt=0),
                   "levels-both_empty-partition": dict(side="left", mode=2, partition=True),
                   "levels-lanes": dict(side="right", mode=2, partition=False, fmt=1),
                   "levels-lanes-no_index": dict(side="right", mode=1, partition=False, index=False)}


@covers("nsm_build_set_table")
@pytest.mark.parametrize("rows", BUILD_ROWS)
@pytest.mark.parametrize("case", SET_TABLE_CASES)
def test_build_set_table(dev, case, rows):
    """Every output column at exactly the size tables.py allocates (and the header states): rows x width ids, the posting
    column at rows x width entries of the format's size, ``post_start`` at 5 keys + 1, ``size_start`` at width + 2,
    ``seg_start`` at 65; byte-equal to the numpy encoder; the caller's arrays unchanged."""
    import torch

    from napkon_string_matching_amd import synthetic, tables

    lib_module, lib = _lib()
    spec = SET_TABLE_CASES[case]
    levels, side, fmt = case.startswith("levels"), spec["side"], spec.get("fmt", 2)
    width = 16
    orig = (np.arange(rows, dtype=np.int32)[::-1] * 3 + 2).copy()
    keep = tables.COMPACT_POSTINGS, tables.RAW_POST_FORMAT
    tables.COMPACT_POSTINGS, tables.RAW_POST_FORMAT = fmt != 0, (1 if fmt == 1 else 2)
    try:
        if levels:
            c = synthetic.c5_cohort(rows, 7 + rows, vocab=300, n_categories=3)
            ids = np.pad(c["ids"], ((0, 0), (0, width - c["ids"].shape[1])), constant_values=-1).astype(np.int32)
            nlev = c["nlev"].astype(np.int32).copy()
            nlev[::5] = 2
            plen = np.take_along_axis(c["plen"], np.minimum(np.arange(c["plen"].shape[1])[None, :], nlev[:, None] - 1), axis=1)
            cat = c["cat"].copy()
            cat[::17] = 0
            mode, part = spec["mode"], spec.get("partition", False)
            want = tables.SetTable.from_nested_arrays(ids, plen, nlev, side, "cpu", categories=cat if mode else None, width=width,
                                                      category_mode=mode, partition=part, orig=orig, index=spec.get("index"))
            assert want.max_levels == plen.shape[1] and (want.seg is not None) == bool(part and mode)
        else:
            rng = np.random.default_rng(rows)
            ids = np.full((rows, width), -1, dtype=np.int32)
            for r in range(rows):
                k = int(rng.integers(0 if r else 1, width + 1))  # (row 0 is never empty: the table has a vocabulary)
                ids[r, :k] = rng.choice(60, size=k, replace=False)
            nlev = plen = cat = None
            mode, part = 0, False
            want = tables.SetTable.from_padded(ids, side, "cpu", width=width, orig=orig, index=spec.get("index"))
    finally:
        tables.COMPACT_POSTINGS, tables.RAW_POST_FORMAT = keep
    assert (want.post is not None) == (side == "right" and spec.get("index") is not False)
    assert want.post is None or want.post_format == (1 if (levels and fmt) else fmt)
    ins = {"ids_in": ids, "nlev_in": nlev, "plen_in": plen, "cat_in": cat if (levels and mode) else None, "orig_in": orig}
    ins = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int64) if v is not None and v.dtype == np.uint64 else v)
           for k, v in ins.items() if v is not None}
    arena = _arena(f"set {case} {rows}", dev, 2 * ar.table_bytes(want) + ar.nbytes_of(*ins.values()))
    ptr = {k: _put(arena, k, v) for k, v in ins.items()}
    inputs = list(arena.regions)
    out = _carve_like(arena, "out", want)
    st = _pointers(out.struct(), arena, "out", want)
    st.n = want.n  # capacity in rows: exactly what the columns hold
    flags = lib_module.BUILD_PARTITION if (part and mode) else 0
    _ok(lib.nsm_build_set_table(ptr["ids_in"], rows, width, 0 if side == "left" else 1, ptr.get("nlev_in"), ptr.get("plen_in"),
                                ptr.get("cat_in"), ptr["orig_in"], mode if levels else 0, flags, ctypes.byref(st), _stream(dev)), case)
    _sync(dev)
    arena.check(unchanged=inputs)
    assert st.n == want.n and tuple(st.post_sq) == tuple(want.post_sq)
    _same_columns(arena, "out", want, f"nsm_build_set_table {case} rows={rows}")


@covers("nsm_build_str_table")
@pytest.mark.parametrize("rows", BUILD_ROWS)
@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("stride", [64, 128, 512])
def test_build_str_table(dev, stride, sort, rows):
    """The columns at exactly ``rows`` rows, as the header sizes them (tables.py keeps one spare row behind them for the
    one-word levels kernel and fills it itself: the builder must not)."""
    import torch

    from napkon_string_matching_amd import tables

    lib_module, lib = _lib()
    rng = np.random.default_rng(stride + rows)
    alphabet = 37
    lengths = rng.integers(0, stride + 1, size=rows).astype(np.int32)
    codes = rng.integers(0, alphabet, size=(rows, stride)).astype(np.uint8)  # (garbage past the length must not matter)
    lengths[0] = stride
    orig = (np.arange(rows, dtype=np.int32)[::-1] * 3 + 2).copy()
    want = tables.StrTable.from_codes(codes, lengths, alphabet, "cpu", orig=orig, sort=sort)
    assert (want.hist16 is not None) == (sort and stride == 64) and (want.len_start is not None) == sort
    ins = {"codes_in": torch.from_numpy(codes), "len_in": torch.from_numpy(lengths), "orig_in": torch.from_numpy(orig)}
    arena = _arena(f"str {stride} {sort} {rows}", dev, 2 * ar.table_bytes(want) + ar.nbytes_of(*ins.values()))
    ptr = {k: _put(arena, k, v) for k, v in ins.items()}
    inputs = list(arena.regions)
    out = _carve_like(arena, "out", want)
    st = out.struct()
    _ok(lib.nsm_build_str_table(ptr["codes_in"], ptr["len_in"], ptr["orig_in"], rows, lib_module.BUILD_SORT if sort else 0,
                                ctypes.byref(st), _stream(dev)), "nsm_build_str_table")
    _sync(dev)
    arena.check(unchanged=inputs)
    assert st.n == rows
    _same_columns(arena, "out", want, f"nsm_build_str_table stride={stride} sort={sort} rows={rows}")


def _level_items_expected(first, nlev, cat, orig, partition):
    """tables.encode_level_codes' numpy path from the builder's inputs on: deeper items first (stable); with a partition one
    row per (item, category), grouped by category."""
    item = np.arange(len(first))
    seg = seg_start = None
    if partition:
        rows = [np.flatnonzero((cat >> np.uint64(c)) & np.uint64(1)) for c in range(64)]
        seg = np.concatenate([np.full(len(r), c, dtype=np.int32) for c, r in enumerate(rows)])
        item = np.concatenate(rows)
        order = np.lexsort((-nlev[item], seg))
        item, seg = item[order], seg[order]
        seg_start = np.zeros(65, dtype=np.int32)
        seg_start[1:] = np.cumsum(np.bincount(seg, minlength=64)[:64])
    else:
        item = item[np.argsort(-nlev, kind="stable")]
    cols = {"first": first[item], "nlev": nlev[item], "orig": orig[item]}
    if cat is not None:
        cols["cat"] = cat[item]
    if partition:
        cols.update(seg=seg, seg_start=seg_start)
    return cols


@covers("nsm_build_level_items")
@pytest.mark.parametrize("rows", BUILD_ROWS)
@pytest.mark.parametrize("layout", ["plain", "lanes", "partition"])
def test_build_level_items(dev, layout, rows):
    import torch

    from napkon_string_matching_amd import tables

    lib_module, lib = _lib()
    rng = np.random.default_rng(rows + len(layout))
    nlev = rng.integers(1, 7, size=rows).astype(np.int32)
    first = (np.cumsum(nlev) - nlev).astype(np.int32)
    orig = (np.arange(rows, dtype=np.int32)[::-1] * 3 + 2).copy()
    cat = None if layout == "plain" else rng.choice(np.array([1, 2, 3, 5, 1 << 40, 1 << 63], dtype=np.uint64), size=rows)
    want = _level_items_expected(first, nlev, cat, orig, layout == "partition")
    n_out = len(want["first"])
    assert n_out == (rows if layout != "partition" else int(np.bitwise_count(cat).sum()))
    ins = {"first_in": first, "nlev_in": nlev, "orig_in": orig}
    if cat is not None:
        ins["cat_in"] = cat.view(np.int64)
    ins = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ins.items()}
    arena = _arena(f"items {layout} {rows}", dev, ar.nbytes_of(*ins.values()) + _region_bytes(*[2 * v.nbytes for v in want.values()]) +
                   8 * ar.GUARD)
    ptr = {k: _put(arena, k, v) for k, v in ins.items()}
    inputs = list(arena.regions)
    for col, v in want.items():
        arena.carve(f"out.{col}", v.nbytes)
    at = lambda col: arena.ptr(f"out.{col}") if col in want else None
    st = lib_module.NsmLevelItems(at("first"), at("nlev"), at("orig"), at("cat"), at("seg"), at("seg_start"), n_out)
    _ok(lib.nsm_build_level_items(ptr["first_in"], ptr["nlev_in"], ptr.get("cat_in"), ptr["orig_in"], rows,
                                  lib_module.CAT_INTERSECT if cat is not None else lib_module.CAT_NONE,
                                  lib_module.BUILD_PARTITION if layout == "partition" else 0, ctypes.byref(st), _stream(dev)), layout)
    _sync(dev)
    arena.check(unchanged=inputs)
    assert st.n == n_out
    for col, v in want.items():
        assert arena.read(f"out.{col}").tobytes() == np.ascontiguousarray(v).tobytes(), f"nsm_build_level_items {layout} rows={rows}: {col}"
    assert tables.MAX_LEVELS >= int(nlev.max())


# ---------------------------------------------------------------------------------------------------------- the catalogue
COVERED_HERE_BY_NAME = {"nsm_support_hits"}  # (its name has none of the kinds' endings; test_support_hits above)
PINNED_ELSEWHERE = {"nsm_assign_hits": "test_gpu_assign.py", "nsm_group_hits": "test_gpu_groups.py",
                    "nsm_span_hits": "test_gpu_forest.py"}  # entry -> the file whose arena test pins its memory contract


def test_every_entry_with_caller_memory_is_covered():
    """Every ``nsm_*`` grid, floor, top-k, profile, pairs, sort and build entry of EVERY header ``include/nsm_hip*.h`` has a
    case in this file, and so has ``nsm_support_hits``.  The three other hit-list entries are pinned in arena tests of their
    own files, which must still import the arena and name the entry.  An entry of a new header is either of a known kind --
    then it needs a case here -- or of none: then it has to be placed in one of the two lists by hand."""
    declared = {}
    for header in HEADERS:
        for e in re.findall(r"^(?:int|uint64_t)\s+(nsm_\w+)\(", header.read_text(encoding="utf-8"), flags=re.M):
            assert e not in declared, f"{e} is declared in {declared[e]} and in {header.name}"
            declared[e] = header.name
    assert [h.name for h in HEADERS] == ["nsm_hip.h", "nsm_hip_assign.h", "nsm_hip_edit.h", "nsm_hip_groups.h", "nsm_hip_measures.h",
                                         "nsm_hip_span.h", "nsm_hip_support.h"]
    kinds = r"_grid$|_top_k|_profile$|_pairs$|^nsm_sort_hits$|^nsm_build_|_workspace_bytes$"
    wanted = {e for e in declared if re.search(kinds, e)} | COVERED_HERE_BY_NAME
    per_header = {h.name: sum(1 for e in wanted if declared[e] == h.name) for h in HEADERS}
    assert per_header == {"nsm_hip.h": 29, "nsm_hip_measures.h": 9, "nsm_hip_edit.h": 9, "nsm_hip_support.h": 1,
                          "nsm_hip_assign.h": 0, "nsm_hip_groups.h": 0, "nsm_hip_span.h": 0}, per_header
    assert len(wanted) == 48
    assert set(declared) - wanted == {"nsm_abi_version", "nsm_release", "nsm_release_all"} | set(PINNED_ELSEWHERE), \
        sorted(set(declared) - wanted)
    assert wanted == set(COVERED), (sorted(wanted - set(COVERED)), sorted(set(COVERED) - wanted))
    assert all(name in globals() for names in COVERED.values() for name in names)
    for entry, file in PINNED_ELSEWHERE.items():
        text = (Path(__file__).resolve().parent / file).read_text(encoding="utf-8")
        assert re.search(r"^from support import arena\b", text, flags=re.M) and f'_lib.entry("{entry}")' in text and \
            "arena.check(" in text, f"{file} no longer runs {entry} inside the guard-band arena"
