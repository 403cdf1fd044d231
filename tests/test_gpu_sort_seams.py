"""``nsm_sort_hits`` (csrc/hits_sort.hip) at the seams of its three code paths, and the ``id_limit`` every Python wrapper
promises it.  The cases, the reference order and the expectations are tests/support/sort_seams.py (checked without a GPU
by tests/test_cpu_sort_seams.py); this file only runs them.

A. The C entry through ctypes, every buffer carved from one guard-band arena (tests/support/arena.py) at exactly the size
   the header states: records, the 8-byte counter, a scratch of ``bound`` records.  The result is compared byte for byte
   with numpy's lexsort by (score descending by its bits, i, j); records between the live count and the bound are
   unspecified and not looked at; records from n_hint on, the counter and every guard byte must be as they were.  A captured
   case is ONE capture on a side stream and ONE replay.

B. Every wrapper that hands the sort an ``id_limit``, on the smallest tables that give more than 8192 records (below that the
   one-workgroup path ignores the promise): relabeling the tables' caller ids must commute with the result.  The identity
   run is checked against the oracle, every other run against the identity run's records mapped on the host."""
import copy

import numpy as np
import pytest

from support import arena as ar
from support import sort_seams as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    """The library, after one eager call on this device: the one-workgroup kernel's shared-memory attribute is set on the
    first call, which must not happen inside a capture."""
    import torch

    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    rec = torch.zeros((4, 2), dtype=torch.float64, device=dev)
    cnt = torch.full((1,), 3, dtype=torch.int64, device=dev)
    assert lib.nsm_sort_hits(rec.data_ptr(), 0, 4, cnt.data_ptr(), 0, 0, torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize(dev)
    return lib


def _drain(dev, what: str) -> None:
    """Wait for the device.  A HIP error here is no failed assertion: the session ends, so that nothing more is launched on
    a device that has reported a fault."""
    import torch

    try:
        torch.cuda.synchronize(dev)
    except RuntimeError as e:
        pytest.exit(f"{what}: the device reported an error, the session stops here: {e}", returncode=3)


# ---------------------------------------------------------------------------------------------------------- A: the entry
def _run(lib, dev, c: ss.Case) -> None:
    import torch

    sizes = [c.capacity * 16, 8] + ([c.bound * 16] if c.scratch else [])
    arena = ar.Arena(sum(s + ar.GUARD + ar.ALIGN for s in sizes) + 4 * ar.GUARD, dev, seed=len(c.name) + c.n)
    before = ss.buffer(c)
    arena.carve("hits", c.capacity * 16)
    arena.fill("hits", before)
    arena.carve("count", 8)
    arena.fill("count", np.array([c.count], dtype=np.uint64))
    sptr = 0
    if c.scratch:
        arena.carve("scratch", c.bound * 16)
        sptr = arena.ptr("scratch")
    args = (arena.ptr("hits"), sptr, c.capacity, arena.ptr("count"), c.n_hint, c.id_limit)
    if c.captured:
        stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(stream):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                rc = lib.nsm_sort_hits(*args, stream.cuda_stream)
            graph.replay()
    else:
        rc = lib.nsm_sort_hits(*args, torch.cuda.current_stream(dev).cuda_stream)
    _drain(dev, c.name)
    assert rc == 0, f"{c.name}: status {rc}: {lib.nsm_last_error()}"
    # the counter is an input; a captured call has nowhere to put a sort's temporary keys and never touches the scratch
    arena.check(unchanged=["count"] + (["scratch"] if c.captured and c.scratch else []))
    ss.check(c, before, arena.read("hits", np.float64).reshape(-1, 2))


@pytest.mark.parametrize("name", ss.NAMES)
def test_sort_hits_case(lib, dev, name):
    _run(lib, dev, ss.BY_NAME[name])


# ------------------------------------------------------------------------------------------------------- B: the wrappers
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _padded(rows, width=16):
    ids = np.full((len(rows), width), -1, dtype=np.int32)
    for r, row in enumerate(rows):
        ids[r, : len(row)] = row
    return ids


def _tables(kind: str, relabeling: str, dev):
    """The tables of one kind under one relabeling, as the wrapper's leading arguments."""
    import torch

    from napkon_string_matching_amd import tables

    lo, ro = ss.relabelings()[relabeling]
    it = ss.wrapper_items()

    def make():
        if kind == "jaccard_raw":
            return (tables.SetTable.from_padded(_padded(it["left_sets"]), "left", dev, width=16, orig=lo),
                    tables.SetTable.from_padded(_padded(it["right_sets"]), "right", dev, width=16, orig=ro))
        if kind == "indel_raw":
            left, right = it["left_strings"], it["right_strings"]
            alpha = tables.Alphabet(left + right)
            stride = tables.pick_stride(max(len(s) for s in left + right))
            side = lambda strings, orig: tables.StrTable.from_codes(*alpha.encode(strings, stride), alpha.size, dev, orig=orig)
            return side(left, lo), side(right, ro)
        if kind == "jaccard_levels":
            def side(levels, name, orig):
                plen = np.array([[len(lv[0]), len(lv[1])] for lv in levels], dtype=np.uint8)
                return tables.SetTable.from_nested_arrays(_padded([lv[1] for lv in levels]), plen, np.full(len(levels), 2, np.int32),
                                                          name, dev, width=16, partition=False, orig=orig)
            return side(it["left_set_levels"], "left", lo), side(it["right_set_levels"], "right", ro)
        li, ls, ri, rs = tables.encode_level_strings(it["left_string_levels"], it["right_string_levels"], dev, partition=False)

        def renamed(items, orig):  # (the encoder numbers the items itself: rename what it reports)
            if orig is None:
                return items
            out = copy.copy(items)
            out.orig = torch.from_numpy(orig).to(dev)[items.orig.long()].contiguous()
            return out
        return renamed(li, lo), ls, renamed(ri, ro), rs

    return _cached((kind, relabeling), make)


def _oracle(kind: str):
    """(score, i, j) of the kind's threshold-0.0 grid on row numbers, from the C oracle: every pair."""
    from oracle import native

    it = ss.wrapper_items()
    cp = lambda s: [ord(ch) for ch in s]

    def make():
        if kind == "jaccard_raw":
            hits = native.jaccard_raw(native.csr(it["left_sets"]), native.csr(it["right_sets"]), 0.0, cap=1 << 14)
        elif kind == "indel_raw":
            hits = native.indel_raw(native.csr([cp(s) for s in it["left_strings"]]), native.csr([cp(s) for s in it["right_strings"]]),
                                    0.0, cap=1 << 14)
        elif kind == "jaccard_levels":
            hits = native.levels(False, it["left_set_levels"], it["right_set_levels"], 0.0, cap=1 << 14)
        else:
            levels = lambda items: [[cp(s) for s in lv] for lv in items]
            hits = native.levels(True, levels(it["left_string_levels"]), levels(it["right_string_levels"]), 0.0, cap=1 << 14)
        assert len(hits) == ss.N_LEFT * ss.N_RIGHT > ss.LDS_MAX
        return (np.array([h[0] for h in hits], np.float64), np.array([h[1] for h in hits], np.int32),
                np.array([h[2] for h in hits], np.int32))

    return _cached(("oracle", kind), make)


def _call(wrapper: str, tabs):
    from napkon_string_matching_amd import grid

    fn = getattr(grid, wrapper)
    try:
        if wrapper.endswith("_top_k"):
            return fn(*tabs, ss.TOP_K, 0.0)
        return fn(*tabs, 0.0, capacity=1 << 14)
    except RuntimeError as e:  # (torch's: a HIP error at one of the wrapper's synchronisations; see _drain)
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"{wrapper}: the device reported an error, the session stops here: {e}", returncode=3)
        raise


@pytest.mark.parametrize("relabeling", ss.RELABELINGS)
@pytest.mark.parametrize("wrapper", ss.WRAPPERS)
def test_wrapper_id_limit(dev, wrapper, relabeling):
    from napkon_string_matching_amd import grid

    kind = "_".join(wrapper.split("_")[:2])
    lo, ro = ss.relabelings()[relabeling]
    tabs = _tables(kind, relabeling, dev)
    if relabeling.startswith("negative") and wrapper in ss.REFUSES_NEGATIVE_IDS:
        with pytest.raises(ValueError, match=ss.REFUSAL):
            _call(wrapper, tabs)
        return
    base = _oracle(kind)
    if wrapper.endswith("_assign"):
        taken = _cached(("assign", kind), lambda: grid.assign_of_hits(grid.Hits(*base)))
        base = (taken.score, taken.i, taken.j)
        assert 0 < len(taken) <= min(ss.N_LEFT, ss.N_RIGHT)
    want = ss.relabelled(*base, lo, ro)
    got = _call(wrapper, tabs)
    assert len(got) == len(want[0]), f"{wrapper} / {relabeling}: {len(got)} records, expected {len(want[0])}"
    got_w, want_w = ss.words(ss.records(got.score, got.i, got.j)), ss.words(ss.records(*want))
    wrong = np.flatnonzero((got_w != want_w).any(axis=1))
    assert wrong.size == 0, (f"{wrapper} / {relabeling}: {wrong.size} records differ, first at {int(wrong[0])}: got "
                             f"{(got.score[wrong[0]], got.i[wrong[0]], got.j[wrong[0]])}, want "
                             f"{tuple(v[wrong[0]] for v in want)}")
