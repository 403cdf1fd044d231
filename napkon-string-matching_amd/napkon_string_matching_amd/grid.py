"""Launch wrappers: one N x M pair grid -> the list of above-threshold hits.

This is the device half of the reference's per-pair loop
(``gen_comparable``: types/comparable_data.py:223-232,243 and ``compare``: :123-126).  The
per-item error surfaces of the reference (``ZeroDivisionError`` for empty-vs-empty Jaccard,
score_functions.py:13; ``IndexError`` for a zero-level item, comparable_data.py:262) are raised
here, before the launch, from per-item properties; the kernels never see such a pair as a hit.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from .tables import LevelItems, SetTable, StrTable

HIT_BYTES = 16
DEFAULT_CAPACITY = 1 << 20


@dataclass
class Hits:
    """Above-threshold pairs in canonical order (score descending, then i, then j)."""

    score: np.ndarray  # float64
    i: np.ndarray  # int32, caller's left item index
    j: np.ndarray  # int32, caller's right item index

    def __len__(self) -> int:
        return int(self.score.shape[0])

    def as_tuples(self):
        return list(zip(self.score.tolist(), self.i.tolist(), self.j.tolist()))


def _require_gpu(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.NsmLibraryError(
            "the match loop only runs on an MI355X (HIP device); there is no CPU fallback"
        )
    return dev


class HitBuffer:
    """Caller-owned hit storage: ``capacity`` 16-byte records followed by the device counter, in ONE
    allocation -- so that the multi-GPU exchange is a single all-gather of ``storage``."""

    def __init__(self, capacity: int, device) -> None:
        self.capacity = int(capacity)
        rows = max(1, self.capacity)
        self.storage = torch.zeros((rows + 1, 2), dtype=torch.float64, device=device)
        self.records = self.storage[:rows]
        self.count = self.storage[rows:].view(torch.int64).view(-1)[:1]  # the trailing record's first 8 bytes
        self.scratch: Optional[torch.Tensor] = None

    def reset(self) -> None:
        self.count.zero_()

    def views(self, n: int):
        score = self.records[:n, 0]
        ij = self.records.view(torch.int32).view(-1, 4)[:n, 2:4]
        return score, ij[:, 0], ij[:, 1]


SMALL_SORT_MAX = 8192  # records nsm_sort_hits orders in one workgroup's LDS (no scratch buffer needed)


def sort_hits_device(buf: HitBuffer, n: int, id_limit: int = 0) -> Hits:
    """Canonical order on the device, then one D2H copy of the n records.  The host has read the counter (``n``), so
    the sort's geometry follows the hits, not the buffer: one launch up to 8192 records at any capacity."""
    if n == 0:
        return Hits(np.zeros(0, np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    lib = _lib.load()
    scratch_ptr = 0
    if n > SMALL_SORT_MAX:
        if buf.scratch is None or buf.scratch.shape[0] < n:
            buf.scratch = torch.empty((n, 2), dtype=torch.float64, device=buf.records.device)
        scratch_ptr = buf.scratch.data_ptr()
    stream = torch.cuda.current_stream(buf.records.device).cuda_stream
    _lib.check(
        lib.nsm_sort_hits(buf.records.data_ptr(), scratch_ptr, buf.capacity, buf.count.data_ptr(), n,
                          max(0, min(int(id_limit), 0x7FFFFFFF)), stream),
        "nsm_sort_hits",
    )
    host = buf.records[:n].cpu().numpy()
    ij = host.view(np.int32).reshape(n, 4)
    return Hits(host[:, 0].copy(), ij[:, 2].copy(), ij[:, 3].copy())


class PendingHits:
    """The hits of a finished grid still in their device buffer (``run_grid(..., defer=True)``): ``finish()`` orders them
    and copies them to the host as always; ``storage(capacity)`` is the wire format of the multi-GPU exchange
    (``distributed.all_gather_storage``) at a capacity the ranks agreed on -- ``capacity`` records and the counter record,
    built on the device, so a sharded ``compare()`` moves its hits GPU -> RCCL -> GPU without a detour through the host."""

    def __init__(self, buf: HitBuffer, n: int, id_limit: int) -> None:
        self.buf, self.n, self.id_limit = buf, int(n), int(id_limit)

    def finish(self) -> Hits:
        return sort_hits_device(self.buf, self.n, self.id_limit)

    def storage(self, capacity: int) -> torch.Tensor:
        out = torch.zeros((int(capacity) + 1, 2), dtype=torch.float64, device=self.buf.records.device)
        out[: self.n] = self.buf.records[: self.n]
        out[int(capacity):].view(torch.int64).view(-1)[0] = self.n
        return out


def run_grid(launch: Callable[[HitBuffer, int], int], device, capacity: Optional[int], what: str,
             id_limit: int = 0, defer: bool = False):
    """Run ``launch`` with a hit buffer, growing it once if the counter overflowed.  ``id_limit``: an upper bound of
    the row ids the grid reports (the larger side's item count), 0 = unknown.  ``defer``: return the hits in their
    device buffer (``PendingHits``) instead of ordering and copying them."""
    dev = _require_gpu(device)
    buf = HitBuffer(capacity or DEFAULT_CAPACITY, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _attempt in range(2):
        buf.reset()
        _lib.check(launch(buf, stream), what)
        n = int(buf.count.item())  # synchronises the stream
        if n <= buf.capacity:
            return PendingHits(buf, n, id_limit) if defer else sort_hits_device(buf, n, id_limit)
        buf = HitBuffer(n, dev)
    raise _lib.NsmLibraryError(f"{what}: hit count changed between two identical launches")


# ------------------------------------------------------------------------------- token-set measures
def check_measure(measure) -> int:
    """The code (``_lib.MEASURES``, include/nsm_hip_measures.h) of a measure name: "union" (Jaccard, the default of every
    ``jaccard_*`` wrapper), "mean" (Dice), "smaller" (overlap), "left" (containment of left in right)."""
    try:
        return _lib.MEASURES[measure]
    except (KeyError, TypeError):
        raise ValueError(f"measure must be one of {tuple(_lib.MEASURES)}, not {measure!r}") from None


def measure_divides_by_zero(measure: str, a: int, b: int) -> bool:
    """Whether the measure's denominator is zero for a left set of ``a`` and a right set of ``b`` tokens."""
    code = check_measure(measure)
    if code == _lib.MEASURE_SMALLER:
        return a == 0 or b == 0
    if code == _lib.MEASURE_LEFT:
        return a == 0
    return a == 0 and b == 0


def check_measure_grid(measure: str, left_empty: bool, n_left: int, right_empty: bool, n_right: int) -> None:
    """The whole-grid ``ZeroDivisionError`` of a measure: ``left_empty`` / ``right_empty`` say whether that side holds an
    empty set.  "union" / "mean": an empty set on both sides; "smaller": an empty set on either side while the other has
    items; "left": an empty left set while the right side has items."""
    code = check_measure(measure)
    if code == _lib.MEASURE_SMALLER:
        bad = (left_empty and n_right > 0) or (right_empty and n_left > 0)
    elif code == _lib.MEASURE_LEFT:
        bad = left_empty and n_right > 0
    else:
        bad = left_empty and right_empty
    if bad:
        raise ZeroDivisionError("division by zero")


def _set_entry(entry: str, measure: str):
    """(C entry, what it takes between the tables and the rest) of a ``nsm_jaccard_*`` per-item query under ``measure``:
    the entry itself for "union", else its ``nsm_set_*`` counterpart with the measure code behind the tables."""
    code = check_measure(measure)
    if code == _lib.MEASURE_UNION:
        return entry, ()
    entry = entry.replace("nsm_jaccard_", "nsm_set_")
    _lib.entry(entry)  # (NsmLibraryError for a library without the measures)
    return entry, (code,)


def _check_set_sides(left: SetTable, right: SetTable, measure: str) -> None:
    """The preconditions of the RAW per-item Jaccard wrappers: the two paddings, then the measure's division by zero."""
    if left.side != "left" or right.side != "right":
        raise ValueError("tables must be encoded with side='left' and side='right' (distinct padding)")
    check_measure_grid(measure, left.has_empty, left.n, right.has_empty, right.n)


# ------------------------------------------------------------------------------- string metrics
def check_metric(metric) -> int:
    """The code (``_lib.METRICS``, include/nsm_hip_edit.h) of a string metric name: "indel" (the Indel ratio of
    ``fuzzy_match``, the default of every ``indel_*`` wrapper), "edit" (normalised Levenshtein similarity) and
    "edit_within" (the best approximate occurrence of the left string inside the right one)."""
    try:
        return _lib.METRICS[metric]
    except (KeyError, TypeError):
        raise ValueError(f"metric must be one of {tuple(_lib.METRICS)}, not {metric!r}") from None


def _edit_entry(entry: str, metric: str):
    """(C entry, what it takes between the tables and the rest) of a ``nsm_indel_*`` per-item query under ``metric``: the
    entry itself for "indel", else its ``nsm_edit_*`` counterpart with the metric code behind the tables.  A query the
    library has no ``nsm_edit_*`` entry for is a ``NotImplementedError``, before the device is asked."""
    code = check_metric(metric)
    if code == _lib.METRIC_INDEL:
        return entry, ()
    entry = entry.replace("nsm_indel_", "nsm_edit_")
    if entry not in _lib.EDIT_EXPORTS:
        raise NotImplementedError(f"{entry}: metric {metric!r} has no kernel for this query (the threshold-grid and general "
                                  "kernels are Indel-only)")
    _lib.entry(entry)  # (NsmLibraryError for a library without the metrics)
    return entry, (code,)


# ------------------------------------------------------------------------------- RAW grids
def jaccard_raw_grid(
    left: SetTable, right: SetTable, threshold: float, prune: bool = True, capacity: Optional[int] = None,
    index: Optional[bool] = None, defer: bool = False, measure: str = "union",
) -> Hits:
    """``intersection_vs_union`` on one set per item, all N x M pairs, hits ``>= threshold``.
    ``index``: None = the library decides (candidates from the right table's global inverted index where its posting
    statistics say they are few, from a per-tile index at low thresholds, else the signature kernel over all pairs);
    True = force an index (the global one when the right table carries it), "tile" = force the per-tile index,
    False = never an index.
    ``measure``: another token-set measure (``check_measure``) -- its threshold grid is the floor grid without floors
    (``nsm_set_raw_floor_grid``, the per-item sweep); ``index`` does not apply to it."""
    if check_measure(measure) != _lib.MEASURE_UNION:
        return jaccard_raw_floor_grid(left, right, threshold, prune=prune, capacity=capacity, defer=defer, measure=measure)
    if left.side != "left" or right.side != "right":
        raise ValueError("tables must be encoded with side='left' and side='right' (distinct padding)")
    if left.has_empty and right.has_empty:
        # score_functions.py:13 -- len(set() | set()) == 0
        raise ZeroDivisionError("division by zero")
    lib = _lib.load()
    ls, rs = left.struct(), right.struct()
    flags = (_lib.FLAG_PRUNE if prune else 0) | (0 if index is None else (_lib.FLAG_INDEX if index else _lib.FLAG_NO_INDEX))
    if index == "tile":
        flags |= _lib.FLAG_TILE_INDEX

    def launch(buf: HitBuffer, stream: int) -> int:
        return lib.nsm_jaccard_raw_grid(
            ls, rs, float(threshold), flags, buf.records.data_ptr(), buf.capacity, buf.count.data_ptr(), stream
        )

    # (0 = unknown on either side: the sort keeps all 32 bits of the ids)
    id_limit = max(left.id_limit, right.id_limit) if left.id_limit and right.id_limit else 0
    return run_grid(launch, left.ids.device, capacity, "nsm_jaccard_raw_grid", id_limit=id_limit, defer=defer)


def indel_raw_grid(
    left: StrTable, right: StrTable, threshold: float, prune: bool = True, capacity: Optional[int] = None,
    two_stage: bool = True, pack: Optional[bool] = None, defer: bool = False, one_group: bool = False, metric: str = "indel",
) -> Hits:
    """``fuzzy_match`` (QRatio/100 = Indel ratio after default_process) on one string per item.
    ``two_stage=False``: the 32-bucket histogram test for every pair even when both tables carry the ``hist16``
    column that selects the two-stage kernel (A/B runs, tests; same hits).
    ``pack``: None = the library decides whether the two-stage scan codes its left operand words once per call (a
    pre-pass into a buffer the library keeps per stream, where the grid is large enough); True = force it, False = never (same hits).
    ``one_group``: where the call packs, the persistent form of the scan (waves that pull work items from a list) as ONE workgroup
    (tests; same hits).
    ``metric``: another string metric (``check_metric``) -- its threshold grid is the floor grid without floors
    (``nsm_edit_raw_floor_grid``, the per-item sweep); ``two_stage``, ``pack`` and ``one_group`` do not apply to it."""
    if check_metric(metric) != _lib.METRIC_INDEL:
        return indel_raw_floor_grid(left, right, threshold, prune=prune, capacity=capacity, defer=defer, metric=metric)
    lib = _lib.load()
    ls, rs = left.struct(), right.struct()
    flags = ((_lib.FLAG_PRUNE if prune else 0) | (0 if two_stage else _lib.FLAG_ONE_STAGE)
             | (0 if pack is None else (_lib.FLAG_PACK if pack else _lib.FLAG_NO_PACK))
             | (_lib.FLAG_ONE_GROUP if one_group else 0))

    def launch(buf: HitBuffer, stream: int) -> int:
        return lib.nsm_indel_raw_grid(
            ls, rs, float(threshold), flags, buf.records.data_ptr(), buf.capacity, buf.count.data_ptr(), stream
        )

    return run_grid(launch, left.codes.device, capacity, "nsm_indel_raw_grid", defer=defer)


# ------------------------------------------------------------------------------- RAW top-k
TOP_K_MAX = 4096  # largest k the kernels keep per row (after clamping to the right side's rows)


def check_k(k) -> int:
    """``k`` of a top-k query: an ``int`` (not a bool) of at least 1, else ``ValueError`` -- before any device work."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 1:
        raise ValueError(f"k must be an int >= 1, got {k!r}")
    return int(k)


def select_top_k(hits: Hits, k: int, groups=None) -> Hits:
    """The first ``k`` records of every left item (score descending, j ascending), returned in canonical order: the
    definition of a top-k query in terms of a threshold grid's hits (also how per-part results are merged).
    ``groups`` (one id per right index, any integer array): first only the best record of every (left item, group) is
    kept -- the group's representative, first in (score descending, j ascending) -- then the ``k`` best representatives
    per left item: the grouped query of ``nsm_*_raw_top_k_grouped``."""
    if len(hits) == 0:
        return hits
    by_row = np.lexsort((hits.j, -hits.score, hits.i))
    if groups is not None:
        # ordered by (i, group, score descending, j): the first record of every (i, group) run is the representative
        g = np.asarray(groups)[hits.j]
        by_group = np.lexsort((hits.j, -hits.score, g, hits.i))
        gi, gg = hits.i[by_group], g[by_group]
        reps = by_group[np.r_[True, (gi[1:] != gi[:-1]) | (gg[1:] != gg[:-1])]]
        by_row = reps[np.lexsort((hits.j[reps], -hits.score[reps], hits.i[reps]))]
    i_sorted = hits.i[by_row]
    start = np.r_[0, np.flatnonzero(i_sorted[1:] != i_sorted[:-1]) + 1]
    rank = np.arange(len(by_row)) - np.repeat(start, np.diff(np.r_[start, len(by_row)]))
    keep = by_row[rank < k]
    order = keep[np.lexsort((hits.j[keep], hits.i[keep], -hits.score[keep]))]
    return Hits(hits.score[order], hits.i[order], hits.j[order])


def _device_groups(groups, n_right: int, orig: torch.Tensor, device, what: str) -> torch.Tensor:
    """``groups`` of a grouped top-k query as the int32 device column the C entries read: one id per right caller index.
    The length is checked before any device work (``ValueError``); the column must also cover every caller id of the table."""
    if isinstance(groups, torch.Tensor):
        if groups.dim() != 1 or groups.dtype != torch.int32:
            raise ValueError(f"{what}: groups must be a one-dimensional int32 tensor")
        n = int(groups.shape[0])
    else:
        groups = np.ascontiguousarray(groups)
        if groups.ndim != 1 or not np.issubdtype(groups.dtype, np.integer):
            raise ValueError(f"{what}: groups must be a one-dimensional integer array")
        n = int(groups.shape[0])
    if n != n_right:
        raise ValueError(f"{what}: {n} group ids for {n_right} right items")
    dev = _require_gpu(device)
    if not isinstance(groups, torch.Tensor):
        if groups.size and (groups.min() < -(1 << 31) or groups.max() >= (1 << 31)):
            raise ValueError(f"{what}: group ids must fit int32")
        groups = torch.from_numpy(groups.astype(np.int32))
    groups = groups.to(dev).contiguous()
    if n_right and int(orig.max().item()) >= n:  # (tables built with caller ids of their own)
        raise ValueError(f"{what}: the right table reports ids up to {int(orig.max().item())}, beyond the {n} group ids")
    return groups


def _top_k(launch: Callable, n_left: int, n_right: int, k: int, device, what: str, stats: Optional[list] = None,
           id_limit: int = 0) -> Hits:
    """Run a top-k launch ``launch(out, out_count, stats, k, stream)`` into a buffer of ``n_left * min(k, n_right)`` records
    (the output size is known in advance: no retry), then order the records canonically on the device."""
    dev = _require_gpu(device)
    k_eff = min(k, max(n_right, 1))
    if k_eff > TOP_K_MAX:  # (what the C entry would answer with NSM_E_UNSUPPORTED, before n_left * k records are allocated)
        raise NotImplementedError(f"{what}: k = {k_eff} (after clamping to the right side's {n_right} rows) exceeds the "
                                  f"supported {TOP_K_MAX}")
    buf = HitBuffer(max(1, n_left * k_eff), dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    buf.reset()
    if n_left and n_right:
        _lib.check(launch(buf.records, buf.count, st, k_eff, torch.cuda.current_stream(dev).cuda_stream), what)
    n = int(buf.count.item())  # synchronises the stream
    if stats is not None:
        stats[:] = [int(v) for v in st.tolist()]
    return sort_hits_device(buf, n, id_limit)


def _raw_top_k(entry: str, left, right, device, k: int, threshold: float, prune: bool, stats: Optional[list], groups,
               id_limit: int = 0, head: tuple = ()) -> Hits:
    """A RAW top-k query through the C entry ``entry``, or with ``groups`` through ``entry + "_grouped"`` (the same
    arguments with the group column in front of the threshold).  ``head``: what the entry takes right behind the tables
    (``_set_entry``)."""
    what = entry if groups is None else entry + "_grouped"
    gcol = None if groups is None else _device_groups(groups, right.n, right.orig, device, what)
    fn = getattr(_lib.load(), what)
    ls, rs = left.struct(), right.struct()
    flags = _lib.FLAG_PRUNE if prune else 0
    group_arg = head if gcol is None else (*head, gcol.data_ptr())
    return _top_k(lambda out, cnt, st, kk, stream: fn(
        ls, rs, *group_arg, float(threshold), kk, flags, out.data_ptr(), cnt.data_ptr(), st.data_ptr(), stream),
        left.n, right.n, k, device, what, stats, id_limit)


def indel_raw_top_k(left: StrTable, right: StrTable, k: int, threshold: float, prune: bool = True,
                    stats: Optional[list] = None, groups=None, metric: str = "indel") -> Hits:
    """For every left item the first ``min(k, #hits of its row)`` records of ``indel_raw_grid(left, right, threshold)``
    in the order (score descending, j ascending), all of them in canonical order.  ``stats``: a list that receives
    [pairs in visited classes, pairs past the length bound, pairs past the histogram bound, exact LCS evaluations].
    ``groups``: an int32 device tensor or integer array with one group id per right caller index -- then a left item gets
    the best record of every group (its representative) and of those the first ``k``: ``select_top_k(hits, k, groups)`` of
    the threshold grid's hits, computed by ``nsm_indel_raw_top_k_grouped`` with lists of one record per group.
    ``metric``: another string metric (``check_metric``: ``nsm_edit_raw_top_k``); stats[3] then counts the exact distances."""
    k = check_k(k)
    entry, head = _edit_entry("nsm_indel_raw_top_k", metric)
    return _raw_top_k(entry, left, right, left.codes.device, k, threshold, prune, stats, groups, head=head)


def jaccard_raw_top_k(left: SetTable, right: SetTable, k: int, threshold: float, prune: bool = True,
                      stats: Optional[list] = None, groups=None, measure: str = "union") -> Hits:
    """``intersection_vs_union`` counterpart of ``indel_raw_top_k``; stats[2] counts the pairs past the signature bound,
    stats[3] the exact merges.  ``groups`` as there (``nsm_jaccard_raw_top_k_grouped``).  ``measure``: another token-set
    measure (``check_measure``: ``nsm_set_raw_top_k``)."""
    k = check_k(k)
    entry, head = _set_entry("nsm_jaccard_raw_top_k", measure)
    if left.side != "left" or right.side != "right":
        raise ValueError("tables must be encoded with side='left' and side='right' (distinct padding)")
    if groups is not None and len(groups) != right.n:  # (a wrong length is reported before the division by zero)
        raise ValueError(f"{entry}_grouped: {len(groups)} group ids for {right.n} right items")
    check_measure_grid(measure, left.has_empty, left.n, right.has_empty, right.n)  # score_functions.py:13, as for the grid
    id_limit = max(left.id_limit, right.id_limit) if left.id_limit and right.id_limit else 0
    return _raw_top_k(entry, left, right, left.ids.device, k, threshold, prune, stats, groups, id_limit, head)


# ------------------------------------------------------------------------------- levels top-k
def banned_csr(banned, n_ids: int, device):
    """The device CSR of a blacklist that ``nsm_*_levels_top_k`` read: ``banned`` = (left ids, right ids) of the banned
    pairs, in the tables' caller ids (``orig``); ``n_ids`` = one more than the largest left caller id.  Returns
    (banned_start int32 [n_ids + 1], banned_j int32, each item's ids ascending), or (None, None) for no blacklist."""
    if banned is None:
        return None, None
    bi = np.asarray(banned[0], dtype=np.int64).reshape(-1)
    bj = np.asarray(banned[1], dtype=np.int64).reshape(-1)
    if bi.shape != bj.shape:
        raise ValueError("banned: the left and right id arrays differ in length")
    if len(bi) == 0:
        return None, None
    if int(bi.min()) < 0 or int(bj.min()) < 0:
        raise ValueError("banned: caller ids must be >= 0")
    n = max(int(n_ids), int(bi.max()) + 1)
    order = np.lexsort((bj, bi))
    start = np.zeros(n + 1, dtype=np.int32)
    start[1:] = np.cumsum(np.bincount(bi, minlength=n))
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
    return to_dev(start), to_dev(bj[order])


def _left_id_limit(orig: torch.Tensor, n: int) -> int:
    """An exclusive upper bound of a device table's caller ids, as ``tables._id_limit`` gives it: max(orig) + 1, and 0
    (= unknown: ``nsm_sort_hits`` then keeps all 32 bits) for an empty table or one that holds a negative id."""
    if not n:
        return 0
    lo, hi = torch.stack(torch.aminmax(orig[:n])).tolist()  # (one synchronisation)
    return 0 if lo < 0 else int(hi) + 1


def _id_count(orig: torch.Tensor, n: int, what: str) -> int:
    """``_left_id_limit`` as the length of an array the kernels index by caller id: a negative id has no slot there."""
    ids = _left_id_limit(orig, n)
    if n and not ids:
        raise ValueError(f"{what}: caller ids must be >= 0")
    return ids


def _levels_top_k(entry: str, tables: tuple, left, right, device, k: int, threshold: float, category_mode: int, prune: bool,
                  banned, stats: Optional[list], head: tuple = ()) -> Hits:
    """A levels top-k query through the C entry ``entry``: ``tables`` in the entry's argument order, ``left`` / ``right``
    the two item tables among them (row counts, caller ids, the encoder's category predicate)."""
    fn = getattr(_lib.load(), entry)
    if left.category_mode is not None:  # the encoder may have dropped the predicate (no categories given)
        category_mode = left.category_mode
    structs = [t.struct() for t in tables]
    flags = _lib.FLAG_PRUNE if prune else 0
    bs, bj = banned_csr(banned, _id_count(left.orig, left.n, "banned") if banned is not None else 0, device)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    return _top_k(lambda out, cnt, st, kk, stream: fn(
        *structs, *head, float(threshold), kk, int(category_mode), flags, ptr(bs), ptr(bj), out.data_ptr(), cnt.data_ptr(),
        st.data_ptr(), stream), left.n, right.n, k, device, entry, stats)


def indel_levels_top_k(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, k: int,
                       threshold: float, category_mode: int = _lib.CAT_NONE, prune: bool = True, banned=None,
                       stats: Optional[list] = None, metric: str = "indel") -> Hits:
    """For every left item the first ``min(k, #hits of its row)`` records of ``indel_levels_grid(...)`` without the
    ``banned`` pairs, in the order (score descending, j ascending), all of them in canonical order.  ``banned``: None or
    (left ids, right ids) of pairs that never take a slot, in caller ids.  Tables must be encoded with
    ``partition=False``.  ``stats``: a list that receives [pairs visited, pairs past the category predicate and the
    length bound, pairs past the histogram bound, pairs that got an exact level score].  ``metric``: another string metric
    (``check_metric``: ``nsm_edit_levels_top_k``)."""
    k = check_k(k)
    entry, head = _edit_entry("nsm_indel_levels_top_k", metric)
    return _levels_top_k(entry, (left, left_strings, right, right_strings), left, right, left.first.device,
                         k, threshold, category_mode, prune, banned, stats, head)


def jaccard_levels_top_k(left: SetTable, right: SetTable, k: int, threshold: float, category_mode: int = _lib.CAT_NONE,
                         prune: bool = True, banned=None, stats: Optional[list] = None, measure: str = "union") -> Hits:
    """``intersection_vs_union`` counterpart of ``indel_levels_top_k`` (tables from ``SetTable.from_levels`` /
    ``from_nested_arrays`` with ``partition=False``); stats[2] counts the pairs past the signature bound.  ``measure``:
    another token-set measure (``check_measure``: ``nsm_set_levels_top_k``)."""
    k = check_k(k)
    entry, head = _set_entry("nsm_jaccard_levels_top_k", measure)
    if left.nlev is None or right.nlev is None:
        raise ValueError("levels top-k needs tables built with SetTable.from_levels")
    if left.side != "left" or right.side != "right":
        raise ValueError("tables must be encoded with side='left' and side='right' (distinct padding)")
    return _levels_top_k(entry, (left, right), left, right, left.ids.device, k, threshold, category_mode, prune, banned, stats,
                         head)


# ------------------------------------------------------------------------------- threshold profiles
PROFILE_MAX_THRESHOLDS = 64  # one threshold per lane of the tally (csrc/score_tally.hpp)


def check_thresholds(thresholds) -> np.ndarray:
    """The ladder of a profile as float64: 1 .. 64 numbers, strictly ascending, no NaN -- else ``ValueError``, before any
    device work."""
    t = np.array(list(thresholds), dtype=np.float64).reshape(-1)
    if not 1 <= len(t) <= PROFILE_MAX_THRESHOLDS:
        raise ValueError(f"a profile takes 1 .. {PROFILE_MAX_THRESHOLDS} thresholds, got {len(t)}")
    if np.isnan(t).any():
        raise ValueError("thresholds must not be NaN")
    if (np.diff(t) <= 0).any():
        raise ValueError("thresholds must be strictly ascending")
    return t


@dataclass
class ThresholdProfile:
    """What a ladder of thresholds would do to one grid, without the hits.  With the grid's hit list at ``thresholds[0]``:
    ``pairs[k]`` = the number of hits scoring ``>= thresholds[k]`` (the length of the grid's hit list at that threshold),
    ``left_best[i]`` / ``right_best[j]`` = the item's largest score among the hits, ``-1.0`` for an item without one."""

    thresholds: np.ndarray  # float64, ascending
    pairs: np.ndarray       # uint64, one per threshold
    left_best: np.ndarray   # float64, by the caller's left index
    right_best: np.ndarray  # float64, by the caller's right index

    def matched_left(self) -> np.ndarray:
        """Per threshold the number of left items with at least one hit at it."""
        return (self.left_best[None, :] >= self.thresholds[:, None]).sum(axis=1).astype(np.int64)

    def matched_right(self) -> np.ndarray:
        return (self.right_best[None, :] >= self.thresholds[:, None]).sum(axis=1).astype(np.int64)


def profile_of_hits(hits: Hits, thresholds, n_left: int, n_right: int) -> ThresholdProfile:
    """The definition of a profile, from the hits of a threshold grid run at (or below) ``thresholds[0]``: hits below
    ``thresholds[0]`` do not count."""
    t = check_thresholds(thresholds)
    keep = hits.score >= t[0]
    score, i, j = hits.score[keep], hits.i[keep], hits.j[keep]
    # (ascending scores: searchsorted left = number of scores < t[k])
    pairs = (len(score) - np.searchsorted(np.sort(score), t, side="left")).astype(np.uint64)
    left_best, right_best = np.full(int(n_left), -1.0), np.full(int(n_right), -1.0)
    np.maximum.at(left_best, i, score)
    np.maximum.at(right_best, j, score)
    return ThresholdProfile(t, pairs, left_best, right_best)


def merge_profiles(parts, thresholds, n_left: int, n_right: int) -> ThresholdProfile:
    """``parts``: (profile of a sub-grid, its left indices, its right indices), the sub-grids disjoint in pairs and all at
    the same ladder.  Counts add, bests take the maximum."""
    t = check_thresholds(thresholds)
    out = ThresholdProfile(t, np.zeros(len(t), np.uint64), np.full(int(n_left), -1.0), np.full(int(n_right), -1.0))
    for prof, li, ri in parts:
        if not np.array_equal(prof.thresholds, t):
            raise ValueError("profiles of different ladders cannot be merged")
        out.pairs += prof.pairs
        np.maximum.at(out.left_best, np.asarray(li, dtype=np.int64), prof.left_best)
        np.maximum.at(out.right_best, np.asarray(ri, dtype=np.int64), prof.right_best)
    return out


def _profile(launch: Callable, t: np.ndarray, left_orig: torch.Tensor, n_left: int, right_orig: torch.Tensor, n_right: int,
             device, what: str, stats: Optional[list]) -> ThresholdProfile:
    """Run a profile launch ``launch(thresholds, T, pairs, left_best, right_best, stats, stream)``.  The best arrays go by
    the tables' caller ids and reach to the largest one; the entry initialises what its tables name, the rest is -1.0."""
    import ctypes

    dev = _require_gpu(device)
    ids_l, ids_r = _id_count(left_orig, n_left, what), _id_count(right_orig, n_right, what)
    pairs = torch.zeros(len(t), dtype=torch.int64, device=dev)
    left_best = torch.full((max(1, ids_l),), -1.0, dtype=torch.float64, device=dev)
    right_best = torch.full((max(1, ids_r),), -1.0, dtype=torch.float64, device=dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    ladder = (ctypes.c_double * len(t))(*t.tolist())
    _lib.check(launch(ladder, len(t), pairs.data_ptr(), left_best.data_ptr(), right_best.data_ptr(), st.data_ptr(),
                      torch.cuda.current_stream(dev).cuda_stream), what)
    if stats is not None:
        stats[:] = [int(v) for v in st.tolist()]
    return ThresholdProfile(t, pairs.cpu().numpy().view(np.uint64), left_best[:ids_l].cpu().numpy(),
                            right_best[:ids_r].cpu().numpy())


def indel_raw_profile(left: StrTable, right: StrTable, thresholds, prune: bool = True,
                      stats: Optional[list] = None, metric: str = "indel") -> ThresholdProfile:
    """``profile_of_hits(indel_raw_grid(left, right, thresholds[0]), thresholds, ...)`` without the hits, in one sweep of
    ``nsm_indel_raw_profile`` (the top-k kernel with a tally in place of its lists).  ``stats`` as for ``indel_raw_top_k``.
    ``metric``: another string metric (``check_metric``: ``nsm_edit_raw_profile``)."""
    t = check_thresholds(thresholds)
    entry, head = _edit_entry("nsm_indel_raw_profile", metric)
    fn = getattr(_lib.load(), entry)
    ls, rs = left.struct(), right.struct()
    flags = _lib.FLAG_PRUNE if prune else 0
    return _profile(lambda lad, n, pairs, lb, rb, st, stream: fn(ls, rs, *head, lad, n, flags, pairs, lb, rb, st, stream),
                    t, left.orig, left.n, right.orig, right.n, left.codes.device, entry, stats)


def jaccard_raw_profile(left: SetTable, right: SetTable, thresholds, prune: bool = True,
                        stats: Optional[list] = None, measure: str = "union") -> ThresholdProfile:
    """``intersection_vs_union`` counterpart of ``indel_raw_profile``; preconditions as for ``jaccard_raw_top_k``.
    ``measure``: another token-set measure (``check_measure``: ``nsm_set_raw_profile``)."""
    t = check_thresholds(thresholds)
    entry, head = _set_entry("nsm_jaccard_raw_profile", measure)
    _check_set_sides(left, right, measure)  # score_functions.py:13, as for the grid
    fn = getattr(_lib.load(), entry)
    ls, rs = left.struct(), right.struct()
    flags = _lib.FLAG_PRUNE if prune else 0
    return _profile(lambda lad, n, pairs, lb, rb, st, stream: fn(ls, rs, *head, lad, n, flags, pairs, lb, rb, st, stream),
                    t, left.orig, left.n, right.orig, right.n, left.ids.device, entry, stats)


def _levels_profile(entry: str, tables: tuple, left, right, device, t: np.ndarray, category_mode: int, prune: bool, banned,
                    stats: Optional[list], head: tuple = ()) -> ThresholdProfile:
    fn = getattr(_lib.load(), entry)
    if left.category_mode is not None:  # the encoder may have dropped the predicate (no categories given)
        category_mode = left.category_mode
    structs = [tab.struct() for tab in tables]
    flags = _lib.FLAG_PRUNE if prune else 0
    bs, bj = banned_csr(banned, _id_count(left.orig, left.n, "banned") if banned is not None else 0, device)
    ptr = lambda x: 0 if x is None else x.data_ptr()
    return _profile(lambda lad, n, pairs, lb, rb, st, stream: fn(*structs, *head, lad, n, int(category_mode), flags, ptr(bs), ptr(bj),
                                                                 pairs, lb, rb, st, stream),
                    t, left.orig, left.n, right.orig, right.n, device, entry, stats)


def indel_levels_profile(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, thresholds,
                         category_mode: int = _lib.CAT_NONE, prune: bool = True, banned=None,
                         stats: Optional[list] = None, metric: str = "indel") -> ThresholdProfile:
    """The profile of ``indel_levels_grid(...)`` without the ``banned`` pairs (``indel_levels_top_k``'s arguments and
    preconditions: tables encoded with ``partition=False``; ``metric``: ``nsm_edit_levels_profile``)."""
    t = check_thresholds(thresholds)
    entry, head = _edit_entry("nsm_indel_levels_profile", metric)
    return _levels_profile(entry, (left, left_strings, right, right_strings), left, right,
                           left.first.device, t, category_mode, prune, banned, stats, head)


def jaccard_levels_profile(left: SetTable, right: SetTable, thresholds, category_mode: int = _lib.CAT_NONE, prune: bool = True,
                           banned=None, stats: Optional[list] = None, measure: str = "union") -> ThresholdProfile:
    """``intersection_vs_union`` counterpart of ``indel_levels_profile`` (``jaccard_levels_top_k``'s preconditions and
    ``measure``: ``nsm_set_levels_profile``)."""
    t = check_thresholds(thresholds)
    entry, head = _set_entry("nsm_jaccard_levels_profile", measure)
    if left.nlev is None or right.nlev is None:
        raise ValueError("levels profile needs tables built with SetTable.from_levels")
    if left.side != "left" or right.side != "right":
        raise ValueError("tables must be encoded with side='left' and side='right' (distinct padding)")
    return _levels_profile(entry, (left, right), left, right, left.ids.device, t, category_mode, prune, banned, stats, head)


# ------------------------------------------------------------------------------- floor grids and best matches
def check_margin(margin) -> float:
    """``margin`` of a best-match query: a finite number ``>= 0`` (not a bool), else ``ValueError`` -- before any device
    work."""
    if isinstance(margin, bool) or not isinstance(margin, (int, float, np.integer, np.floating)):
        raise ValueError(f"margin must be a finite number >= 0, got {margin!r}")
    m = float(margin)
    if not np.isfinite(m) or m < 0.0:
        raise ValueError(f"margin must be a finite number >= 0, got {margin!r}")
    return m


def _best_scores(hits: Hits, n_left: Optional[int], n_right: Optional[int]):
    """(left_best, right_best) of a hit list: every item's largest score, ``-inf`` for an item without a hit."""
    nl = max(int(n_left or 0), int(hits.i.max()) + 1 if len(hits) else 0)
    nr = max(int(n_right or 0), int(hits.j.max()) + 1 if len(hits) else 0)
    lb, rb = np.full(nl, -np.inf), np.full(nr, -np.inf)
    np.maximum.at(lb, hits.i, hits.score)
    np.maximum.at(rb, hits.j, hits.score)
    return lb, rb


def _canonical(score: np.ndarray, i: np.ndarray, j: np.ndarray) -> Hits:
    order = np.lexsort((j, i, -score))
    return Hits(score[order], i[order], j[order])


def filter_by_floors(hits: Hits, left_floor=None, right_floor=None) -> Hits:
    """The records of ``hits`` with ``score >= left_floor[i]`` and ``score >= right_floor[j]`` (each array float64 by
    caller id, or None for no floor on that side), in canonical order: the definition of a floor grid in terms of the
    threshold grid's hits, and the host-side gate for hits that come from the general kernels.  The comparisons are exact;
    a NaN floor admits nothing."""
    keep = np.ones(len(hits), dtype=bool)
    if left_floor is not None:
        keep &= hits.score >= np.asarray(left_floor, dtype=np.float64)[hits.i]
    if right_floor is not None:
        keep &= hits.score >= np.asarray(right_floor, dtype=np.float64)[hits.j]
    return _canonical(hits.score[keep], hits.i[keep], hits.j[keep])


def best_of_hits(hits: Hits, margin: float = 0.0, mutual: bool = False, n_left: Optional[int] = None,
                 n_right: Optional[int] = None) -> Hits:
    """The definition of a best-match query on a threshold grid's hit list: the records with ``score >= lb[i] - margin``,
    ``lb[i]`` the left item's largest score in ``hits``; with ``mutual`` also ``score >= rb[j] - margin`` for the right
    item's.  One float64 subtraction, exact comparisons.  ``margin=0`` is every item's best match with all its ties, a
    margin at least as large as the largest score gives ``hits`` back.  Canonical order."""
    m = check_margin(margin)
    lb, rb = _best_scores(hits, n_left, n_right)
    return filter_by_floors(hits, lb - m, rb - m if mutual else None)


def _floor_column(floor, ids: int, device, what: str) -> Optional[torch.Tensor]:
    """A floor array as the float64 device column the C entries read: one entry per caller id, reaching at least to the
    table's largest (``ids`` = that id + 1) -- the kernels index it with the table's ``orig`` values."""
    if floor is None:
        return None
    if isinstance(floor, torch.Tensor):
        if floor.dim() != 1 or floor.dtype != torch.float64:
            raise ValueError(f"{what}: floors must be a one-dimensional float64 tensor")
        col = floor.to(device).contiguous()
    else:
        arr = np.ascontiguousarray(floor, dtype=np.float64)
        if arr.ndim != 1:
            raise ValueError(f"{what}: floors must be a one-dimensional float64 array")
        col = torch.from_numpy(arr).to(device)
    if int(col.shape[0]) < ids:
        raise ValueError(f"{what}: {int(col.shape[0])} floors for caller ids up to {ids - 1}")
    return col


def _floor_grid(entry: str, structs: list, middle: tuple, left, right, device, threshold: float, left_floor, right_floor,
                stats: Optional[list], capacity: Optional[int], defer: bool = False):
    """A floor grid through the C entry ``entry``: ``structs`` the tables in the entry's argument order (and what it takes
    right behind them), ``middle`` what it takes between the floors and the hit buffer, ``left`` / ``right`` the two tables
    whose caller ids the floors go by.  ``defer``: as for ``run_grid``."""
    dev = _require_gpu(device)
    fn = getattr(_lib.load(), entry)
    ids_l, ids_r = _left_id_limit(left.orig, left.n), _left_id_limit(right.orig, right.n)
    if left_floor is not None:  # (the kernels index a floor array by caller id)
        _id_count(left.orig, left.n, entry + ": left_floor")
    if right_floor is not None:
        _id_count(right.orig, right.n, entry + ": right_floor")
    lf = _floor_column(left_floor, ids_l, dev, entry + ": left_floor")
    rf = _floor_column(right_floor, ids_r, dev, entry + ": right_floor")
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    ptr = lambda t: 0 if t is None or t.numel() == 0 else t.data_ptr()

    def launch(buf: HitBuffer, stream: int) -> int:
        st.zero_()  # (a retry at a larger capacity sweeps again)
        return fn(*structs, float(threshold), ptr(lf), ptr(rf), *middle, buf.records.data_ptr(), buf.capacity,
                  buf.count.data_ptr(), st.data_ptr(), stream)

    # (every reported id is below the larger limit: the sort's key width; an empty side reports nothing)
    hits = run_grid(launch, dev, capacity, entry, id_limit=max(ids_l, ids_r) if ids_l and ids_r else 0, defer=defer)
    if stats is not None:
        stats[:] = [int(v) for v in st.tolist()]
    return hits


def indel_raw_floor_grid(left: StrTable, right: StrTable, threshold: float, left_floor=None, right_floor=None,
                         prune: bool = True, stats: Optional[list] = None, capacity: Optional[int] = None,
                         defer: bool = False, metric: str = "indel") -> Hits:
    """``filter_by_floors(indel_raw_grid(left, right, threshold), left_floor, right_floor)`` in one sweep of
    ``nsm_indel_raw_floor_grid`` (the top-k kernel with a gate in place of its lists): a threshold grid whose threshold is
    per item.  Floors: numpy float64 arrays or float64 tensors indexed by caller id, or None.  ``stats`` as for
    ``indel_raw_top_k``.  ``metric``: another string metric (``check_metric``: ``nsm_edit_raw_floor_grid``); ``defer`` as
    for the grids."""
    entry, head = _edit_entry("nsm_indel_raw_floor_grid", metric)
    flags = _lib.FLAG_PRUNE if prune else 0
    return _floor_grid(entry, [left.struct(), right.struct(), *head], (flags,), left, right, left.codes.device,
                       threshold, left_floor, right_floor, stats, capacity, defer)


def jaccard_raw_floor_grid(left: SetTable, right: SetTable, threshold: float, left_floor=None, right_floor=None,
                           prune: bool = True, stats: Optional[list] = None, capacity: Optional[int] = None,
                           defer: bool = False, measure: str = "union") -> Hits:
    """``intersection_vs_union`` counterpart of ``indel_raw_floor_grid``; preconditions as for ``jaccard_raw_top_k``.
    ``measure``: another token-set measure (``check_measure``: ``nsm_set_raw_floor_grid``); ``defer`` as for the grids."""
    entry, head = _set_entry("nsm_jaccard_raw_floor_grid", measure)
    _check_set_sides(left, right, measure)  # score_functions.py:13, as for the grid
    flags = _lib.FLAG_PRUNE if prune else 0
    return _floor_grid(entry, [left.struct(), right.struct(), *head], (flags,), left, right, left.ids.device,
                       threshold, left_floor, right_floor, stats, capacity, defer)


def _levels_floor_grid(entry: str, tables: tuple, left, right, device, threshold: float, left_floor, right_floor,
                       category_mode: int, prune: bool, banned, stats: Optional[list], capacity: Optional[int],
                       head: tuple = (), defer: bool = False) -> Hits:
    if left.category_mode is not None:  # the encoder may have dropped the predicate (no categories given)
        category_mode = left.category_mode
    bs, bj = banned_csr(banned, _id_count(left.orig, left.n, "banned") if banned is not None else 0, device)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    middle = (int(category_mode), _lib.FLAG_PRUNE if prune else 0, ptr(bs), ptr(bj))
    return _floor_grid(entry, [*(t.struct() for t in tables), *head], middle, left, right, device, threshold, left_floor,
                       right_floor, stats, capacity, defer)


def indel_levels_floor_grid(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable,
                            threshold: float, left_floor=None, right_floor=None, category_mode: int = _lib.CAT_NONE,
                            prune: bool = True, banned=None, stats: Optional[list] = None,
                            capacity: Optional[int] = None, defer: bool = False, metric: str = "indel") -> Hits:
    """``filter_by_floors`` of ``indel_levels_grid(...)`` without the ``banned`` pairs, in one sweep of
    ``nsm_indel_levels_floor_grid`` (``indel_levels_top_k``'s arguments and preconditions: tables encoded with
    ``partition=False``; ``metric``: ``nsm_edit_levels_floor_grid``; ``defer`` as for the grids)."""
    entry, head = _edit_entry("nsm_indel_levels_floor_grid", metric)
    return _levels_floor_grid(entry, (left, left_strings, right, right_strings), left, right,
                              left.first.device, threshold, left_floor, right_floor, category_mode, prune, banned, stats, capacity,
                              head, defer)


def jaccard_levels_floor_grid(left: SetTable, right: SetTable, threshold: float, left_floor=None, right_floor=None,
                              category_mode: int = _lib.CAT_NONE, prune: bool = True, banned=None,
                              stats: Optional[list] = None, capacity: Optional[int] = None, defer: bool = False,
                              measure: str = "union") -> Hits:
    """``intersection_vs_union`` counterpart of ``indel_levels_floor_grid`` (``jaccard_levels_top_k``'s preconditions and
    ``measure``: ``nsm_set_levels_floor_grid``; ``defer`` as for the grids)."""
    entry, head = _set_entry("nsm_jaccard_levels_floor_grid", measure)
    if left.nlev is None or right.nlev is None:
        raise ValueError("levels floor grid needs tables built with SetTable.from_levels")
    if left.side != "left" or right.side != "right":
        raise ValueError("tables must be encoded with side='left' and side='right' (distinct padding)")
    return _levels_floor_grid(entry, (left, right), left, right, left.ids.device, threshold, left_floor, right_floor,
                              category_mode, prune, banned, stats, capacity, head, defer)


def floors_of_profile(prof: ThresholdProfile, margin: float, mutual: bool):
    """(left_floor, right_floor) of a best-match query from the profile at its threshold: ``best - margin``, one float64
    subtraction per item; no right floor unless ``mutual``.  An item without a hit (best -1.0) has nothing to admit."""
    m = check_margin(margin)
    return prof.left_best - m, (prof.right_best - m if mutual else None)


def _best(profile: Callable, floor_grid: Callable, margin: float, threshold: float, mutual: bool, stats: Optional[list]) -> Hits:
    """Best matches in two sweeps: ``profile([threshold], stats)`` for every item's best score, then
    ``floor_grid(left_floor, right_floor, stats)`` with ``floor = best - margin``.  ``stats`` receives both sweeps'
    counters: [the profile's four, the floor grid's four]."""
    m = check_margin(margin)
    t = check_thresholds([threshold])
    st1, st2 = [], []
    lf, rf = floors_of_profile(profile(t, st1), m, mutual)
    hits = floor_grid(lf, rf, st2)
    if stats is not None:
        stats[:] = [st1, st2]
    return hits


def indel_raw_best(left: StrTable, right: StrTable, margin: float = 0.0, threshold: float = 0.0, mutual: bool = False,
                   prune: bool = True, stats: Optional[list] = None, metric: str = "indel") -> Hits:
    """``best_of_hits(indel_raw_grid(left, right, threshold), margin, mutual)`` without the grid's hits: every left item's
    best match with everything within ``margin`` of it (``margin=0``: all its ties), with ``mutual`` only the pairs that
    are also within ``margin`` of the right item's best.  A profile sweep at ``[threshold]``, then a floor grid.
    ``metric`` as for ``indel_raw_top_k``."""
    return _best(lambda t, st: indel_raw_profile(left, right, t, prune=prune, stats=st, metric=metric),
                 lambda lf, rf, st: indel_raw_floor_grid(left, right, threshold, lf, rf, prune=prune, stats=st, metric=metric),
                 margin, threshold, mutual, stats)


def jaccard_raw_best(left: SetTable, right: SetTable, margin: float = 0.0, threshold: float = 0.0, mutual: bool = False,
                     prune: bool = True, stats: Optional[list] = None, measure: str = "union") -> Hits:
    """``intersection_vs_union`` counterpart of ``indel_raw_best``; preconditions and ``measure`` as for ``jaccard_raw_top_k``."""
    return _best(lambda t, st: jaccard_raw_profile(left, right, t, prune=prune, stats=st, measure=measure),
                 lambda lf, rf, st: jaccard_raw_floor_grid(left, right, threshold, lf, rf, prune=prune, stats=st, measure=measure),
                 margin, threshold, mutual, stats)


def indel_levels_best(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable,
                      margin: float = 0.0, threshold: float = 0.0, mutual: bool = False, category_mode: int = _lib.CAT_NONE,
                      prune: bool = True, banned=None, stats: Optional[list] = None, metric: str = "indel") -> Hits:
    """Best matches of ``indel_levels_grid(...)`` without the ``banned`` pairs (``indel_levels_top_k``'s preconditions and
    ``metric``)."""
    tabs = (left, left_strings, right, right_strings)
    return _best(lambda t, st: indel_levels_profile(*tabs, t, category_mode=category_mode, prune=prune, banned=banned, stats=st,
                                                    metric=metric),
                 lambda lf, rf, st: indel_levels_floor_grid(*tabs, threshold, lf, rf, category_mode=category_mode, prune=prune,
                                                            banned=banned, stats=st, metric=metric),
                 margin, threshold, mutual, stats)


def jaccard_levels_best(left: SetTable, right: SetTable, margin: float = 0.0, threshold: float = 0.0, mutual: bool = False,
                        category_mode: int = _lib.CAT_NONE, prune: bool = True, banned=None,
                        stats: Optional[list] = None, measure: str = "union") -> Hits:
    """``intersection_vs_union`` counterpart of ``indel_levels_best`` (``jaccard_levels_top_k``'s preconditions and ``measure``)."""
    return _best(lambda t, st: jaccard_levels_profile(left, right, t, category_mode=category_mode, prune=prune, banned=banned,
                                                      stats=st, measure=measure),
                 lambda lf, rf, st: jaccard_levels_floor_grid(left, right, threshold, lf, rf, category_mode=category_mode,
                                                              prune=prune, banned=banned, stats=st, measure=measure),
                 margin, threshold, mutual, stats)


# ------------------------------------------------------------------------------- listed pairs
NO_SCORE = -1.0  # what a listed pair without a score gets (the profiles' "none")


def check_pair_ids(i, j):
    """The two id columns of a pair list as int64 arrays: one-dimensional integer arrays of equal length, else
    ``ValueError`` -- before any device work."""
    i, j = np.asarray(i), np.asarray(j)
    for name, a in (("i", i), ("j", j)):
        if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
            raise ValueError(f"pairs: {name} must be a one-dimensional integer array")
    if i.shape != j.shape:
        raise ValueError(f"pairs: {len(i)} left ids for {len(j)} right ids")
    return i.astype(np.int64), j.astype(np.int64)


def _pair_keys(i: np.ndarray, j: np.ndarray) -> np.ndarray:
    return (i.astype(np.int64) << 32) | (j.astype(np.int64) & 0xFFFFFFFF)


def lookup_pairs(hits, i, j) -> np.ndarray:
    """The definition of a pairs query in terms of a grid's hits: for every listed pair ``(i[p], j[p])`` its score in
    ``hits`` (a ``Hits``, or a sequence of ``(score, i, j)`` records), ``-1.0`` when the pair is not among them.  The order
    is the caller's, duplicates get equal scores."""
    i, j = check_pair_ids(i, j)
    if not isinstance(hits, Hits):
        rec = list(hits)
        hits = Hits(np.array([r[0] for r in rec], dtype=np.float64), np.array([r[1] for r in rec], dtype=np.int32),
                    np.array([r[2] for r in rec], dtype=np.int32))
    out = np.full(len(i), NO_SCORE, dtype=np.float64)
    if len(hits) == 0 or len(i) == 0:
        return out
    keys = _pair_keys(hits.i, hits.j)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    int32 = lambda a: (a >= -(1 << 31)) & (a < (1 << 31))
    fits = int32(i) & int32(j)  # (an id beyond int32 is in no hit list)
    want = _pair_keys(np.where(fits, i, 0), np.where(fits, j, 0))
    at = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    found = fits & (keys[at] == want)
    out[found] = hits.score[order[at[found]]]
    return out


def _row_map(orig: torch.Tensor, n: int, device) -> torch.Tensor:
    """The inverse of a table's ``orig`` column as the entries read it: row_map[id] = the row of caller id ``id``, -1 for
    an id no row carries -- one scatter of ``arange`` by ``orig``."""
    ids = _id_count(orig, n, "pairs")
    rows = torch.full((max(1, ids),), -1, dtype=torch.int32, device=device)
    if n:
        rows[orig[:n].long()] = torch.arange(n, dtype=torch.int32, device=device)
    return rows[:ids] if ids else rows[:0]


def _pairs(entry: str, tables: tuple, left, right, device, i, j, head: tuple = ()) -> np.ndarray:
    """A pairs query through the C entry ``entry``: ``tables`` in the entry's argument order, ``left`` / ``right`` the two
    tables among them whose rows the caller ids name."""
    i, j = check_pair_ids(i, j)
    dev = _require_gpu(device)
    fn = getattr(_lib.load(), entry)
    n = len(i)
    if n == 0:
        return np.zeros(0, dtype=np.float64)
    fits = lambda a: np.where((a >= 0) & (a < (1 << 31)), a, -1).astype(np.int32)  # (no such id: -1.0 either way)
    host = np.zeros((n, 2), dtype=np.float64)
    ij = host.view(np.int32).reshape(n, 4)
    ij[:, 2], ij[:, 3] = fits(i), fits(j)
    records = torch.from_numpy(host).to(dev)
    lmap, rmap = _row_map(left.orig, left.n, dev), _row_map(right.orig, right.n, dev)
    structs = [t.struct() for t in tables]
    ptr = lambda t: t.data_ptr() if t.numel() else 0
    _lib.check(fn(*structs, *head, ptr(lmap), int(lmap.numel()), ptr(rmap), int(rmap.numel()), records.data_ptr(), n,
                  torch.cuda.current_stream(dev).cuda_stream), entry)
    return records[:, 0].cpu().numpy()


def indel_raw_pairs(left: StrTable, right: StrTable, i, j, metric: str = "indel") -> np.ndarray:
    """The ``fuzzy_match`` score of every listed pair: ``i`` / ``j`` are integer arrays of equal length holding caller ids
    (the tables' ``orig`` values).  Returns float64 scores in the caller's order -- ``lookup_pairs(indel_raw_grid(left,
    right, -inf), i, j)`` bit for bit, ``-1.0`` for an id the table does not hold -- in O(P), by ``nsm_indel_raw_pairs``.
    ``metric``: another string metric (``check_metric``: ``nsm_edit_raw_pairs``)."""
    i, j = check_pair_ids(i, j)
    entry, head = _edit_entry("nsm_indel_raw_pairs", metric)
    return _pairs(entry, (left, right), left, right, left.codes.device, i, j, head)


def jaccard_raw_pairs(left: SetTable, right: SetTable, i, j, measure: str = "union") -> np.ndarray:
    """``intersection_vs_union`` counterpart of ``indel_raw_pairs``; a pair of two empty sets gets ``-1.0`` (the plugin
    raises ``ZeroDivisionError`` for it).  ``measure``: another token-set measure (``check_measure``:
    ``nsm_set_raw_pairs``), ``-1.0`` wherever its denominator is zero."""
    i, j = check_pair_ids(i, j)
    entry, head = _set_entry("nsm_jaccard_raw_pairs", measure)
    if left.side != "left" or right.side != "right":
        raise ValueError("tables must be encoded with side='left' and side='right' (distinct padding)")
    return _pairs(entry, (left, right), left, right, left.ids.device, i, j, head)


def indel_levels_pairs(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, i, j,
                       metric: str = "indel") -> np.ndarray:
    """The ``compare_terms`` x ``fuzzy_match`` score of every listed pair of items, as ``indel_levels_grid`` computes it --
    without category predicate or blacklist.  ``-1.0`` also for a pair with an item without levels.  Tables must be encoded
    with ``partition=False``.  ``metric``: another string metric (``check_metric``: ``nsm_edit_levels_pairs``)."""
    i, j = check_pair_ids(i, j)
    entry, head = _edit_entry("nsm_indel_levels_pairs", metric)
    return _pairs(entry, (left, left_strings, right, right_strings), left, right, left.first.device, i, j, head)


def jaccard_levels_pairs(left: SetTable, right: SetTable, i, j, measure: str = "union") -> np.ndarray:
    """``intersection_vs_union`` counterpart of ``indel_levels_pairs`` (tables from ``SetTable.from_levels`` /
    ``from_nested_arrays`` with ``partition=False``); ``-1.0`` also for a pair that compares two empty levels.
    ``measure``: another token-set measure (``nsm_set_levels_pairs``), ``-1.0`` for a pair with a step that divides by zero."""
    i, j = check_pair_ids(i, j)
    entry, head = _set_entry("nsm_jaccard_levels_pairs", measure)
    if left.nlev is None or right.nlev is None:
        raise ValueError("levels pairs need tables built with SetTable.from_levels")
    if left.side != "left" or right.side != "right":
        raise ValueError("tables must be encoded with side='left' and side='right' (distinct padding)")
    return _pairs(entry, (left, right), left, right, left.ids.device, i, j, head)


# ------------------------------------------------------------------------------- levels grids
def jaccard_levels_grid(
    left: SetTable, right: SetTable, threshold: float, category_mode: int = _lib.CAT_NONE, prune: bool = True,
    capacity: Optional[int] = None, index: Optional[bool] = None, defer: bool = False, measure: str = "union", banned=None,
) -> Hits:
    """``compare_terms`` with ``intersection_vs_union`` over suffix-nested levels.
    ``index``: None = the library decides (candidates from the right table's global inverted index where its posting
    statistics say they are few, from a per-tile index at low thresholds, else the filter kernel over all pairs);
    True = force an index (the global one when the right table carries it), "tile" = force the per-tile index,
    False = never an index.
    ``measure``: another token-set measure (``check_measure``) -- its threshold grid is the floor grid without floors
    (``nsm_set_levels_floor_grid``: tables encoded with ``partition=False``, and ``banned`` as ``jaccard_levels_top_k``
    takes it; ``index`` does not apply)."""
    if check_measure(measure) != _lib.MEASURE_UNION:
        return jaccard_levels_floor_grid(left, right, threshold, category_mode=category_mode, prune=prune, banned=banned,
                                         capacity=capacity, defer=defer, measure=measure)
    if banned is not None:
        raise ValueError("banned: the Jaccard threshold grid takes no blacklist (jaccard_levels_floor_grid does)")
    if left.nlev is None or right.nlev is None:
        raise ValueError("levels grid needs tables built with SetTable.from_levels")
    lib = _lib.load()
    ls, rs = left.struct(), right.struct()
    flags = (_lib.FLAG_PRUNE if prune else 0) | (0 if index is None else (_lib.FLAG_INDEX if index else _lib.FLAG_NO_INDEX))
    if index == "tile":
        flags |= _lib.FLAG_TILE_INDEX
    if (left.seg is None) != (right.seg is None) or left.category_mode != right.category_mode:
        raise ValueError("both sides must be encoded alike: same category_mode and partition (tables.partition_allowed)")
    if left.category_mode is not None:  # the encoder may have rewritten the predicate (partition)
        category_mode = left.category_mode

    def launch(buf: HitBuffer, stream: int) -> int:
        return lib.nsm_jaccard_levels_grid(
            ls, rs, float(threshold), int(category_mode), flags, buf.records.data_ptr(), buf.capacity,
            buf.count.data_ptr(), stream,
        )

    return run_grid(launch, left.ids.device, capacity, "nsm_jaccard_levels_grid", defer=defer)


PROBE_MIN_PAIRS = 1 << 27      # grids of at least this many pairs are probed before they are routed (11 600 x 11 600)
PROBE_LEFT_ROWS = 8192          # left rows of the probe's sample
SPLIT_MAX_SURVIVAL = 0.10       # of the pairs a grid visits: up to here the split path, beyond it the shared-tile kernel


def _visited_pairs(left: LevelItems, right: LevelItems) -> float:
    """Pairs the one-word kernels score step 1 for: all of them, or -- partitioned tables -- the same-category ones."""
    if left.seg_start is None or right.seg_start is None:
        return float(left.n) * float(right.n)
    a = left.seg_start.cpu().numpy().astype(np.float64)
    b = right.seg_start.cpu().numpy().astype(np.float64)
    return float(((a[1:] - a[:-1]) * (b[1:] - b[:-1])).sum())


def probe_survival(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, threshold: float,
                   category_mode: int):
    """MEASURE, on a sample of the left rows, how many pairs outlive step 1 of ``compare_terms`` x ``fuzzy_match`` on this
    grid (one-word level strings): every k-th row of the left items table (the rows stay grouped by category and ordered by
    depth) against the whole right side through the scan kernel alone (``NSM_FLAG_PROBE``), the survivors read from the
    workspace's queue counters.  Returns (expected survivors of the full grid, pairs the full grid visits), or None when
    the grid is not one the split path could take.  Which path is fastest depends on that rate and nothing else that a
    threshold could tell: word-like text at 0.55 lets 2.8 % of the same-category pairs through, digit strings at 0.65
    about 60 %."""
    lib = _lib.load()
    dev = left.first.device
    k = max(1, left.n // PROBE_LEFT_ROWS)
    idx = torch.arange(0, left.n, k, device=dev)
    seg = seg_start = None
    if left.seg is not None:
        seg = left.seg[idx].contiguous()
        seg_start = torch.zeros(65, dtype=torch.int32, device=dev)
        seg_start[1:] = torch.cumsum(torch.bincount(seg, minlength=64)[:64], 0).to(torch.int32)
    sample = LevelItems(first=left.first[idx].contiguous(), nlev=left.nlev[idx].contiguous(), orig=left.orig[idx].contiguous(),
                        cat=None if left.cat is None else left.cat[idx].contiguous(), n=int(idx.numel()), seg=seg,
                        seg_start=seg_start, category_mode=left.category_mode)
    flags = _lib.FLAG_PRUNE | _lib.FLAG_SPLIT | _lib.FLAG_PROBE
    si, ls, ri, rs = sample.struct(), left_strings.struct(), right.struct(), right_strings.struct()
    if int(lib.nsm_indel_levels_workspace_bytes(si, ls, ri, rs, float(threshold), flags, 0.0)) == 0:
        return None
    ws = torch.zeros(64 + 2 * (1 << 16), dtype=torch.int64, device=dev)  # control words + two small queue halves
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.nsm_indel_levels_grid(si, ls, ri, rs, float(threshold), int(category_mode), flags, 0, 0, count.data_ptr(),
                                         ws.data_ptr(), ws.numel() * 8, 1.0, stream), "nsm_indel_levels_grid (probe)")
    # (expected survivors 1: ONE round over the sample whatever the queue holds -- only the counters matter)
    survivors = float(ws[2:64].sum().item())  # (synchronises; the counters keep counting past the queue's capacity)
    visited_sample = _visited_pairs(sample, right)
    visited = _visited_pairs(left, right)
    if visited_sample <= 0:
        return 0.0, visited
    return survivors / visited_sample * visited, visited


def route_one_word(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, threshold: float,
                   category_mode: int):
    """(extra flags, expected survivors, what was measured) for a large grid of one-word level strings: probe, then the split
    path when few pairs outlive step 1, the shared-tile kernel when many do.  (0, 0.0, None): leave it to the library."""
    got = probe_survival(left, left_strings, right, right_strings, threshold, category_mode)
    if got is None:
        return 0, 0.0, None
    expected, visited = got
    rate = expected / visited if visited > 0 else 0.0
    if rate <= SPLIT_MAX_SURVIVAL:
        # (sampling error: a quarter more queue than the estimate)
        return _lib.FLAG_SPLIT, max(1.0, 1.25 * expected), {"survival_rate": rate, "path": "split", "pairs_visited": visited}
    return _lib.FLAG_TILE, 0.0, {"survival_rate": rate, "path": "tile", "pairs_visited": visited}


def indel_levels_grid(
    left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, threshold: float,
    category_mode: int = _lib.CAT_NONE, prune: bool = True, capacity: Optional[int] = None, wave_wide: bool = False,
    park: bool = False, workspace: Optional[int] = None, return_overflow: Optional[list] = None, defer: bool = False,
    probe: Optional[bool] = None, route: Optional[list] = None, metric: str = "indel", banned=None,
) -> Hits:
    """``compare_terms`` with ``fuzzy_match`` over per-level strings.  ``wave_wide`` selects the kernel
    without block-cooperative parking, ``park`` the round-2 kernel for multi-word strings (same hits; A/B runs
    and tests).  ``workspace``: bytes of split-path scratch to hand to the library (None = what it asks for, 0 = none:
    the single-kernel path); ``return_overflow``: a list that receives the workspace's overflow word (tests).
    ``probe``: measure the survival rate of step 1 on a sample first and route by it (None = for large grids of one-word
    strings; ``route`` receives what was decided).
    ``metric``: another string metric (``check_metric``) -- its threshold grid is the floor grid without floors
    (``nsm_edit_levels_floor_grid``: tables encoded with ``partition=False``, and ``banned`` as ``indel_levels_top_k``
    takes it; the kernel switches, the workspace and the probe do not apply)."""
    if check_metric(metric) != _lib.METRIC_INDEL:
        return indel_levels_floor_grid(left, left_strings, right, right_strings, threshold, category_mode=category_mode,
                                       prune=prune, banned=banned, capacity=capacity, defer=defer, metric=metric)
    if banned is not None:
        raise ValueError("banned: the Indel threshold grid takes no blacklist (indel_levels_floor_grid does)")
    lib = _lib.load()
    li, ls, ri, rs = left.struct(), left_strings.struct(), right.struct(), right_strings.struct()
    flags = (_lib.FLAG_PRUNE if prune else 0) | (_lib.FLAG_WAVE_WIDE if wave_wide else 0) | (_lib.FLAG_PARK if park else 0)
    if (left.seg is None) != (right.seg is None) or left.category_mode != right.category_mode:
        raise ValueError("both sides must be encoded alike: same category_mode and partition (tables.partition_allowed)")
    if left.category_mode is not None:  # the encoder may have rewritten the predicate (partition)
        category_mode = left.category_mode

    dev = left.first.device
    expected = 0.0
    if probe is None:
        probe = (workspace is None and prune and not wave_wide and not park and left_strings.stride == 64 and threshold > 0 and
                 float(left.n) * float(right.n) >= PROBE_MIN_PAIRS)
    if probe:
        extra, expected, measured = route_one_word(left, left_strings, right, right_strings, threshold, category_mode)
        flags |= extra
        if route is not None and measured is not None:
            route.append(dict(measured, expected_survivors=expected))
    # the split path's survivor queue (scan kernel -> queue -> finish kernel; one-word strings at thresholds >= 0.7, or
    # wherever the probe found few survivors) is CALLER-owned scratch: a torch tensor, so torch's allocator owns it and it
    # goes back to the cache with this call
    want = int(lib.nsm_indel_levels_workspace_bytes(li, ls, ri, rs, float(threshold), flags, float(expected))) if workspace is None \
        else int(workspace)
    ws = split_workspace(want, dev) if want > 0 else None

    def launch(buf: HitBuffer, stream: int) -> int:
        return lib.nsm_indel_levels_grid(
            li, ls, ri, rs, float(threshold), int(category_mode), flags, buf.records.data_ptr(), buf.capacity,
            buf.count.data_ptr(), ws.data_ptr() if ws is not None else 0, ws.numel() * 8 if ws is not None else 0, float(expected),
            stream,
        )

    hits = run_grid(launch, dev, capacity, "nsm_indel_levels_grid", defer=defer)  # (returns after the stream has been synchronised)
    if ws is not None and return_overflow is not None:
        return_overflow.append(int(ws[1].item()) & 0xFFFFFFFF)
    return hits


def split_workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    """Scratch for ``nsm_indel_levels_grid`` (include/nsm_hip.h): ``nbytes`` rounded down to 8-byte words, at most what
    the device can spare -- less than the library asks for only means more rounds.  None when memory is too tight for a
    useful queue: the grid then runs its single-kernel path."""
    words = int(nbytes) // 8
    try:
        free, _total = torch.cuda.mem_get_info(device)
        words = min(words, int(free * 0.5) // 8)
    except RuntimeError:
        pass
    if words < 128:
        return None
    try:
        return torch.empty(words, dtype=torch.int64, device=device)
    except torch.cuda.OutOfMemoryError:
        return None


# ------------------------------------------------------------------------------- one-to-one assignment
ASSIGN_ROUTES = {None: 0, "rounds": _lib.ASSIGN_ROUNDS_ONLY, "stream": _lib.ASSIGN_STREAM_ONLY}


def assign_of_hits(hits: Hits) -> Hits:
    """The definition of a one-to-one assignment on a hit list: walk the records in canonical order, take a record iff
    neither its ``i`` nor its ``j`` has been taken, and mark both.  The taken records, in canonical order.  A record that
    repeats an ``(i, j)`` is a record like any other: the second one is never taken.  The result is one-to-one and maximal
    (no record of ``hits`` has both items free), and a prefix in the score: assigning the records ``>= t`` gives the
    records ``>= t`` of the assignment."""
    h = _canonical(np.asarray(hits.score, np.float64), np.asarray(hits.i, np.int32), np.asarray(hits.j, np.int32))
    left, right, keep = set(), set(), []
    for r, (a, b) in enumerate(zip(h.i.tolist(), h.j.tolist())):
        if a not in left and b not in right:
            left.add(a)
            right.add(b)
            keep.append(r)
    keep = np.asarray(keep, dtype=np.int64)
    return Hits(h.score[keep], h.i[keep], h.j[keep])


def _assign_flags(route) -> int:
    if route not in ASSIGN_ROUTES:
        raise ValueError(f"route must be None, 'rounds' or 'stream', got {route!r}")
    return ASSIGN_ROUTES[route]


def assign_hits_device(buf: HitBuffer, n: int, n_left: int, n_right: int, id_limit: int = 0, route=None,
                       stats: Optional[list] = None) -> Hits:
    """``assign_of_hits`` of the ``n`` records in ``buf`` without the list leaving the device: canonical order
    (``nsm_sort_hits``, in place), ``nsm_assign_hits``, the order again for the at most min(n, n_left, n_right) records of
    the assignment, and one D2H copy of those.  ``n_left`` / ``n_right``: exclusive bounds of the records' ids."""
    flags = _assign_flags(route)
    if n == 0:
        if stats is not None:
            stats[:] = [0, 0, 0, 0]
        return Hits(np.zeros(0, np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32))
    fn = _lib.entry("nsm_assign_hits")
    lib = _lib.load()
    dev = buf.records.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    limit = max(0, min(int(id_limit), 0x7FFFFFFF))
    scratch_ptr = 0
    if n > SMALL_SORT_MAX:
        if buf.scratch is None or buf.scratch.shape[0] < n:
            buf.scratch = torch.empty((n, 2), dtype=torch.float64, device=dev)
        scratch_ptr = buf.scratch.data_ptr()
    _lib.check(lib.nsm_sort_hits(buf.records.data_ptr(), scratch_ptr, buf.capacity, buf.count.data_ptr(), n, limit, stream),
               "nsm_sort_hits")
    out = HitBuffer(max(1, min(n, int(n_left), int(n_right))), dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.check(fn(buf.records.data_ptr(), n, int(n_left), int(n_right), flags, out.records.data_ptr(), out.count.data_ptr(),
                  st.data_ptr(), stream), "nsm_assign_hits")
    if stats is not None:
        stats[:] = [int(v) for v in st.tolist()]
    return sort_hits_device(out, int(out.count.item()), limit)


def assign_hits(hits: Hits, n_left: Optional[int] = None, n_right: Optional[int] = None, device=None, route=None,
                stats: Optional[list] = None) -> Hits:
    """``assign_of_hits(hits)`` on the device for any host hit list: canonical order, upload, ``nsm_assign_hits``,
    ``nsm_sort_hits`` on the result, and a copy back of at most min(N, M) records.  ``n_left`` / ``n_right``: exclusive
    bounds of the ids (None = the largest id in ``hits`` + 1); ids must be ``>= 0``.  ``route``: None = the library routes
    (parallel rounds while they pay, then the one-workgroup stream stage), "rounds" / "stream" = one stage only (same
    records).  ``stats`` receives [rounds run, records live when the stream stage started, matches made by rounds, matches
    made by the stream stage]."""
    _assign_flags(route)
    dev = _require_gpu("cuda" if device is None else device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    h = _canonical(np.asarray(hits.score, np.float64), np.asarray(hits.i, np.int32), np.asarray(hits.j, np.int32))
    n = len(h)
    nl = max(int(n_left or 0), int(h.i.max()) + 1 if n else 0)
    nr = max(int(n_right or 0), int(h.j.max()) + 1 if n else 0)
    if n and (int(h.i.min()) < 0 or int(h.j.min()) < 0):
        raise ValueError("assign_hits: ids must be >= 0")
    buf = HitBuffer(n, dev)
    if n:
        host = np.empty((n, 2), dtype=np.float64)
        host[:, 0] = h.score
        ij = host.view(np.int32).reshape(n, 4)
        ij[:, 2], ij[:, 3] = h.i, h.j
        buf.records[:n] = torch.from_numpy(host).to(dev)
        buf.count.fill_(n)
    return assign_hits_device(buf, n, nl, nr, max(nl, nr), route, stats)


def _assign_pending(pending: PendingHits, left, right, route, stats: Optional[list]) -> Hits:
    # (nsm_assign_hits marks taken items in arrays indexed by caller id)
    ids_l, ids_r = _id_count(left.orig, left.n, "assign"), _id_count(right.orig, right.n, "assign")
    return assign_hits_device(pending.buf, pending.n, ids_l, ids_r, max(ids_l, ids_r) if ids_l and ids_r else 0, route, stats)


def indel_raw_assign(left: StrTable, right: StrTable, threshold: float, prune: bool = True, capacity: Optional[int] = None,
                     two_stage: bool = True, pack: Optional[bool] = None, route=None, stats: Optional[list] = None,
                     metric: str = "indel") -> Hits:
    """``assign_of_hits(indel_raw_grid(left, right, threshold, ...))``: the grid's hits stay in their device buffer, are
    ordered and assigned there, and only the assignment (at most min(N, M) records) crosses to the host."""
    pending = indel_raw_grid(left, right, threshold, prune=prune, capacity=capacity, two_stage=two_stage, pack=pack, defer=True,
                             metric=metric)
    return _assign_pending(pending, left, right, route, stats)


def jaccard_raw_assign(left: SetTable, right: SetTable, threshold: float, prune: bool = True, capacity: Optional[int] = None,
                       index: Optional[bool] = None, route=None, stats: Optional[list] = None, measure: str = "union") -> Hits:
    """``intersection_vs_union`` counterpart of ``indel_raw_assign`` (``measure`` as for ``jaccard_raw_grid``)."""
    pending = jaccard_raw_grid(left, right, threshold, prune=prune, capacity=capacity, index=index, defer=True, measure=measure)
    return _assign_pending(pending, left, right, route, stats)


def indel_levels_assign(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, threshold: float,
                        category_mode: int = _lib.CAT_NONE, prune: bool = True, capacity: Optional[int] = None, route=None,
                        stats: Optional[list] = None, **grid_options) -> Hits:
    """``assign_of_hits(indel_levels_grid(...))`` without the grid's hits leaving the device (``grid_options``: the grid's
    other keywords)."""
    pending = indel_levels_grid(left, left_strings, right, right_strings, threshold, category_mode=category_mode, prune=prune,
                                capacity=capacity, defer=True, **grid_options)
    return _assign_pending(pending, left, right, route, stats)


def jaccard_levels_assign(left: SetTable, right: SetTable, threshold: float, category_mode: int = _lib.CAT_NONE,
                          prune: bool = True, capacity: Optional[int] = None, index: Optional[bool] = None, route=None,
                          stats: Optional[list] = None, measure: str = "union", banned=None) -> Hits:
    """``intersection_vs_union`` counterpart of ``indel_levels_assign`` (``measure``, ``banned`` as for ``jaccard_levels_grid``)."""
    pending = jaccard_levels_grid(left, right, threshold, category_mode=category_mode, prune=prune, capacity=capacity,
                                  index=index, defer=True, measure=measure, banned=banned)
    return _assign_pending(pending, left, right, route, stats)


# ------------------------------------------------------------------------------- match groups
def _check_forest(start, nodes: int) -> np.ndarray:
    forest = np.asarray(start)
    if forest.shape != (nodes,) or not np.issubdtype(forest.dtype, np.integer):
        raise ValueError(f"start must be an integer array of {nodes} labels")
    if nodes and ((forest < 0).any() or (forest > np.arange(nodes)).any()):
        raise ValueError("start: every label[v] must lie in [0, v]")
    return forest.astype(np.int32)


def _list_nodes(hits: Hits, left_base: int, right_base: int, nodes: int, what: str):
    """The two node columns of a list (int64), range-checked: ALL records, whatever their score."""
    i, j = np.asarray(hits.i, dtype=np.int64), np.asarray(hits.j, dtype=np.int64)
    left_base, right_base = int(left_base), int(right_base)
    if left_base < 0 or right_base < 0 or left_base > nodes or right_base > nodes:
        raise ValueError(f"{what}: a list's bases must lie in [0, nodes]")
    if len(i) and (int(i.min()) < 0 or int(j.min()) < 0):
        raise ValueError(f"{what}: ids must be >= 0")
    if len(i) and (int(i.max()) + left_base >= nodes or int(j.max()) + right_base >= nodes):
        raise ValueError(f"{what}: a record reaches beyond the {nodes} nodes")
    return i + left_base, j + right_base


def groups_of_hits(lists, nodes: int, min_score: float = 0.0, start=None) -> np.ndarray:
    """The definition of match groups.  ``lists = [(Hits, left_base, right_base), ...]``: record ``(score, i, j)`` is an edge
    between node ``left_base + i`` and node ``right_base + j`` if ``score >= min_score`` (a NaN links nothing).  Returns
    int32 ``label[nodes]``: the smallest node of every node's connected component over all lists together; a node no
    record touches is its own label.  ``start``: a forest to link into (``0 <= start[v] <= v``, e.g. an earlier result).
    Plain union-find on the host; the order of records and lists does not matter."""
    nodes = int(nodes)
    if nodes < 0:
        raise ValueError("groups_of_hits: nodes must be >= 0")
    parent = list(range(nodes)) if start is None else _check_forest(start, nodes).tolist()

    def find(v: int) -> int:
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for hits, left_base, right_base in lists:
        u, v = _list_nodes(hits, left_base, right_base, nodes, "groups_of_hits")
        keep = np.asarray(hits.score, dtype=np.float64) >= min_score
        for a, b in zip(u[keep].tolist(), v[keep].tolist()):
            a, b = find(a), find(b)
            if a != b:
                parent[max(a, b)] = min(a, b)  # (the smaller root stays: the last root is the component's minimum)
    return np.fromiter((find(v) for v in range(nodes)), dtype=np.int32, count=nodes)


def _records_to_device(hits: Hits, dev) -> Optional[torch.Tensor]:
    """A host list as device records (16 bytes each: score, i, j), in the order given."""
    n = len(hits)
    if n == 0:
        return None
    host = np.empty((n, 2), dtype=np.float64)
    host[:, 0] = hits.score
    ij = host.view(np.int32).reshape(n, 4)
    ij[:, 2], ij[:, 3] = hits.i, hits.j
    return torch.from_numpy(host).to(dev)


def group_lists_device(entries, nodes: int, min_score: float, dev, start=None, stats: Optional[list] = None) -> np.ndarray:
    """One ``nsm_group_hits`` call over device lists and one D2H copy of the ``nodes`` labels.  ``entries``: per list
    ``(records pointer, n, left_base, left_ids, right_base, right_ids)``."""
    fn = _lib.entry("nsm_group_hits")
    nodes = int(nodes)
    if nodes == 0:
        if stats is not None:
            stats[:] = [0, 0]
        return np.zeros(0, dtype=np.int32)
    flags = 0
    if start is None:
        label = torch.empty(nodes, dtype=torch.int32, device=dev)
    else:
        label = torch.from_numpy(_check_forest(start, nodes)).to(dev)
        flags = _lib.GROUP_CONTINUE
    lists = (_lib.NsmHitList * max(1, len(entries)))()
    for slot, (ptr, n, left_base, left_ids, right_base, right_ids) in zip(lists, entries):
        slot.hits, slot.n = (ptr if n else None), int(n)
        slot.left_base, slot.left_ids, slot.right_base, slot.right_ids = int(left_base), int(left_ids), int(right_base), int(right_ids)
    st = torch.zeros(2, dtype=torch.int64, device=dev) if stats is not None else None
    status = fn(lists, len(entries), nodes, float(min_score), flags, label.data_ptr(), st.data_ptr() if st is not None else None,
                torch.cuda.current_stream(dev).cuda_stream)
    if status == 10001:
        raise ValueError("nsm_group_hits: " + _lib.load().nsm_last_error().decode("utf-8", "replace"))
    _lib.check(status, "nsm_group_hits")
    if stats is not None:
        stats[:] = [int(v) for v in st.tolist()]
    return label.cpu().numpy()


def group_hits(lists, nodes: int, min_score: float = 0.0, start=None, device=None, stats: Optional[list] = None,
               min_support=0) -> np.ndarray:
    """``groups_of_hits(lists, nodes, min_score, start)`` on the device for host hit lists: upload (in any order), one
    ``nsm_group_hits`` call over all lists, one D2H copy of ``nodes`` words.  Ids must be ``>= 0`` and every record must
    stay inside the nodes (``ValueError``).  ``stats`` receives [records with score >= min_score, hooks made].

    ``min_support > 0``: the groups are the connected components of the ``(min_support + 2)``-truss of the records
    ``>= min_score`` -- ``groups_of_hits`` over the records whose ``truss_of_hits`` word is ``>= 0`` -- so a chain
    a-b, b-c without a-c no longer makes one group, and a larger ``min_support`` refines the groups.  ``nsm_support_hits``
    runs on the device lists, the alive records are compacted there and linked by ``nsm_group_hits`` as always.  Meant for
    self-joins, overlapping node ranges and three or more cohorts: two disjoint cohorts are a bipartite graph, where every
    support is 0 and every group dissolves."""
    min_support = check_min_support(min_support)
    dev = _require_gpu("cuda" if device is None else device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    nodes = int(nodes)
    if nodes < 0:
        raise ValueError("group_hits: nodes must be >= 0")
    entries, keep = _upload_lists(lists, nodes, dev, "group_hits")
    if min_support:
        entries, keep = _truss_entries(entries, keep, nodes, min_score, min_support, dev)
    return group_lists_device(entries, nodes, min_score, dev, start, stats)


@dataclass
class MatchGroups:
    """Match groups over one or more cohorts that share a node space: cohort ``c``'s item ``k`` is node ``bases[c] + k``."""

    label: np.ndarray  # int32 [nodes]: the smallest node of every node's group
    bases: tuple  # per cohort: its first node
    cohort_sizes: tuple  # per cohort: its number of items (ids)

    def of(self, c: int) -> np.ndarray:
        """The labels of cohort ``c``'s items."""
        return self.label[self.bases[c]: self.bases[c] + self.cohort_sizes[c]]

    def sizes(self) -> np.ndarray:
        """Per node the number of nodes it labels: the group's size at its smallest node, 0 elsewhere."""
        return np.bincount(self.label, minlength=len(self.label))

    def members(self, min_size: int = 2):
        """The groups of at least ``min_size`` nodes, ordered by label, each as a tuple of per-cohort item-index arrays."""
        order = np.argsort(self.label, kind="stable")  # (within a group: nodes ascending)
        sorted_label = self.label[order]
        starts = np.r_[0, np.flatnonzero(sorted_label[1:] != sorted_label[:-1]) + 1, len(order)] if len(order) else np.zeros(1, int)
        out = []
        for a, b in zip(starts[:-1].tolist(), starts[1:].tolist()):
            if b - a < min_size:
                continue
            nodes = order[a:b]
            out.append(tuple((nodes[(nodes >= base) & (nodes < base + size)] - base).astype(np.int64)
                             for base, size in zip(self.bases, self.cohort_sizes)))
        return out


def _groups_pending(pending: PendingHits, left, right, same: bool, min_score, stats: Optional[list],
                    min_support=0) -> MatchGroups:
    min_support = check_min_support(min_support)
    # (nsm_group_hits indexes the labels by caller id)
    ids_l, ids_r = _id_count(left.orig, left.n, "groups"), _id_count(right.orig, right.n, "groups")
    if same:  # one node space: left item k and right item k are the same node
        nodes, bases, sizes = max(ids_l, ids_r), (0,), (max(ids_l, ids_r),)
    else:
        nodes, bases, sizes = ids_l + ids_r, (0, ids_l), (ids_l, ids_r)
    floor = float("-inf") if min_score is None else float(min_score)
    # the buffer goes in UNSORTED: components need no order
    entries, dev = [(pending.buf.records.data_ptr(), pending.n, 0, ids_l, bases[-1], ids_r)], pending.buf.records.device
    if min_support:  # only the records of the (min_support + 2)-truss link (group_hits has the meaning)
        entries, _keep = _truss_entries(entries, [pending.buf.records], nodes, floor, min_support, dev)
    label = group_lists_device(entries, nodes, floor, dev, None, stats)
    return MatchGroups(label, bases, sizes)


def indel_raw_groups(left: StrTable, right: StrTable, threshold: float, prune: bool = True, capacity: Optional[int] = None,
                     two_stage: bool = True, pack: Optional[bool] = None, same: bool = False, min_score: Optional[float] = None,
                     stats: Optional[list] = None, metric: str = "indel", min_support=0) -> MatchGroups:
    """``groups_of_hits([(indel_raw_grid(left, right, threshold, ...), 0, right's base)], ...)``: the grid's hits stay in
    their device buffer, unsorted, are linked there, and only the labels cross to the host.  ``same``: both tables
    describe the same items (a self-join), numbered in ONE node space -- near-duplicate clusters.  ``min_score``: only
    records scoring at least that link (None: every hit of the grid).  ``min_support > 0``: only the records of the
    ``(min_support + 2)``-truss link (``group_hits`` has the meaning; for ``same=True`` -- two disjoint cohorts are
    bipartite and dissolve): ``nsm_support_hits`` on the buffer, the alive records compacted on the device."""
    check_min_support(min_support)  # (before any device work)
    pending = indel_raw_grid(left, right, threshold, prune=prune, capacity=capacity, two_stage=two_stage, pack=pack, defer=True,
                             metric=metric)
    return _groups_pending(pending, left, right, same, min_score, stats, min_support)


def jaccard_raw_groups(left: SetTable, right: SetTable, threshold: float, prune: bool = True, capacity: Optional[int] = None,
                       index: Optional[bool] = None, same: bool = False, min_score: Optional[float] = None,
                       stats: Optional[list] = None, measure: str = "union", min_support=0) -> MatchGroups:
    """``intersection_vs_union`` counterpart of ``indel_raw_groups`` (``measure`` as for ``jaccard_raw_grid``)."""
    check_min_support(min_support)  # (before any device work)
    pending = jaccard_raw_grid(left, right, threshold, prune=prune, capacity=capacity, index=index, defer=True, measure=measure)
    return _groups_pending(pending, left, right, same, min_score, stats, min_support)


def indel_levels_groups(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, threshold: float,
                        category_mode: int = _lib.CAT_NONE, prune: bool = True, capacity: Optional[int] = None, same: bool = False,
                        min_score: Optional[float] = None, stats: Optional[list] = None, min_support=0, **grid_options) -> MatchGroups:
    """``groups_of_hits`` of ``indel_levels_grid(...)``'s hits without them leaving the device (``grid_options``: the grid's
    other keywords)."""
    check_min_support(min_support)  # (before any device work)
    pending = indel_levels_grid(left, left_strings, right, right_strings, threshold, category_mode=category_mode, prune=prune,
                                capacity=capacity, defer=True, **grid_options)
    return _groups_pending(pending, left, right, same, min_score, stats, min_support)


def jaccard_levels_groups(left: SetTable, right: SetTable, threshold: float, category_mode: int = _lib.CAT_NONE,
                          prune: bool = True, capacity: Optional[int] = None, index: Optional[bool] = None, same: bool = False,
                          min_score: Optional[float] = None, stats: Optional[list] = None, measure: str = "union",
                          banned=None, min_support=0) -> MatchGroups:
    """``intersection_vs_union`` counterpart of ``indel_levels_groups`` (``measure``, ``banned`` as for ``jaccard_levels_grid``)."""
    check_min_support(min_support)  # (before any device work)
    pending = jaccard_levels_grid(left, right, threshold, category_mode=category_mode, prune=prune, capacity=capacity,
                                  index=index, defer=True, measure=measure, banned=banned)
    return _groups_pending(pending, left, right, same, min_score, stats, min_support)


# ------------------------------------------------------------------------------- edge support and truss groups
def check_min_support(min_support) -> int:
    """``min_support`` as an int: an integer ``>= 0`` (``ValueError`` otherwise -- 1.5 and "1" are not integers)."""
    if isinstance(min_support, (bool, np.bool_)) or not isinstance(min_support, (int, np.integer)):
        raise ValueError(f"min_support must be an integer >= 0, not {min_support!r}")
    if int(min_support) < 0 or int(min_support) > 0x7FFFFFFF:
        raise ValueError(f"min_support must be an integer >= 0, not {min_support!r}")
    return int(min_support)


def _edge_keys(lists, nodes: int, min_score: float, what: str):
    """Per list the key ``min(u, v) * nodes + max(u, v)`` of every record (int64) and which records are edge records."""
    out = []
    for hits, left_base, right_base in lists:
        u, v = _list_nodes(hits, left_base, right_base, nodes, what)
        edge = (np.asarray(hits.score, dtype=np.float64) >= min_score) & (u != v)  # (a NaN compares false)
        out.append((np.minimum(u, v) * max(nodes, 1) + np.maximum(u, v), edge))
    return out


def truss_of_hits(lists, nodes: int, min_support, min_score: float = 0.0):
    """The definition of edge support and of the truss.  ``lists = [(Hits, left_base, right_base), ...]`` in the node space
    of ``groups_of_hits``.  Record ``(score, i, j)`` is an EDGE RECORD iff ``score >= min_score`` (a NaN never is) and
    ``u = left_base + i != v = right_base + j``; ``E`` is the set of unordered pairs ``{u, v}`` of all edge records of all
    lists together (duplicates and the two orientations of a self-join collapse), ``N(u) = {w : {u, w} in E}``.

    Peeling is synchronous: a round counts every alive edge's support ``|N(u) & N(v)|`` among the alive edges, then removes
    ALL alive edges with support ``< min_support`` at once; it stops after the first round that removes nothing.  Returns
    ``([int32 array per list], rounds)``: per record its edge's support in the final graph (``>= min_support``), ``-2`` for
    an edge record whose edge was removed, ``-1`` for any other record; ``rounds`` counts the counting passes, the last one
    included.  What is left is the ``(min_support + 2)``-truss (``networkx.k_truss(G, min_support + 2)``): the fixpoint is
    unique, so the order of removal -- and of records and lists -- does not matter.  Python sets on the host."""
    nodes, min_support = int(nodes), check_min_support(min_support)
    if nodes < 0:
        raise ValueError("truss_of_hits: nodes must be >= 0")
    keyed = _edge_keys(lists, nodes, min_score, "truss_of_hits")
    edges = np.unique(np.concatenate([key[edge] for key, edge in keyed])) if keyed else np.zeros(0, dtype=np.int64)
    ends = [(int(k) // max(nodes, 1), int(k) % max(nodes, 1)) for k in edges.tolist()]
    alive = np.ones(len(ends), dtype=bool)
    support = np.zeros(len(ends), dtype=np.int32)
    rounds = 0
    while True:
        rounds += 1
        near = {}
        for e, (a, b) in enumerate(ends):
            if alive[e]:
                near.setdefault(a, set()).add(b)
                near.setdefault(b, set()).add(a)
        for e, (a, b) in enumerate(ends):
            support[e] = len(near[a] & near[b]) if alive[e] else 0
        drop = alive & (support < min_support)
        if not drop.any():
            break
        alive &= ~drop
    words = []
    for key, edge in keyed:
        out = np.full(len(key), -1, dtype=np.int32)
        at = np.searchsorted(edges, key[edge])
        out[edge] = np.where(alive[at], support[at], -2)
        words.append(out)
    return words, rounds


def support_of_hits(lists, nodes: int, min_score: float = 0.0):
    """Per list an int32 array aligned with its records: ``|N(u) & N(v)|``, the number of common neighbours of the record's
    two ends, for an edge record and ``-1`` for any other (``truss_of_hits`` has the definitions; this is its
    ``min_support = 0``).  Independent of record order, list order and duplicates."""
    return truss_of_hits(lists, nodes, 0, min_score)[0]


def support_lists_device(entries, nodes: int, min_score: float, min_support: int, dev, stats: Optional[list] = None):
    """One ``nsm_support_hits`` call (include/nsm_hip_support.h) over device lists; the words stay on the device: per list
    an int32 tensor aligned with its records (``truss_of_hits``).  ``entries`` as for ``group_lists_device``.  ``stats``
    receives [edge records, distinct edges, distinct edges alive at the end, rounds, sum of the final supports]."""
    min_support = check_min_support(min_support)
    fn = _lib.entry("nsm_support_hits")
    nodes = int(nodes)
    words = [torch.empty(int(n), dtype=torch.int32, device=dev) for _ptr, n, *_rest in entries]
    lists = (_lib.NsmHitList * max(1, len(entries)))()
    out = (ctypes.c_void_p * max(1, len(entries)))()
    for k, (slot, (ptr, n, left_base, left_ids, right_base, right_ids)) in enumerate(zip(lists, entries)):
        slot.hits, slot.n = (ptr if n else None), int(n)
        slot.left_base, slot.left_ids, slot.right_base, slot.right_ids = int(left_base), int(left_ids), int(right_base), int(right_ids)
        out[k] = words[k].data_ptr() if n else None
    st = torch.zeros(5, dtype=torch.int64, device=dev) if stats is not None else None
    status = fn(lists, len(entries), nodes, float(min_score), min_support, out, st.data_ptr() if st is not None else None,
                torch.cuda.current_stream(dev).cuda_stream)
    if status == 10001:
        raise ValueError("nsm_support_hits: " + _lib.load().nsm_last_error().decode("utf-8", "replace"))
    _lib.check(status, "nsm_support_hits")
    if stats is not None:
        stats[:] = [int(v) for v in st.tolist()]
    return words


def _upload_lists(lists, nodes: int, dev, what: str):
    """Host lists as device records and the entries ``group_lists_device`` / ``support_lists_device`` take."""
    entries, keep = [], []
    for hits, left_base, right_base in lists:
        _list_nodes(hits, left_base, right_base, nodes, what)
        recs = _records_to_device(hits, dev)
        keep.append(recs)
        # (any id that stays inside the nodes is a node: the id counts reach to the end of the node space)
        entries.append((recs.data_ptr() if recs is not None else 0, len(hits), int(left_base), nodes - int(left_base),
                        int(right_base), nodes - int(right_base)))
    return entries, keep


def support_hits(lists, nodes: int, min_score: float = 0.0, min_support=0, device=None, stats: Optional[list] = None):
    """``truss_of_hits(lists, nodes, min_support, min_score)[0]`` on the device for host hit lists (``min_support = 0``:
    ``support_of_hits``): upload (in any order), one ``nsm_support_hits`` call over all lists, one D2H copy of the words.
    ``stats`` as for ``support_lists_device``; ``stats[3]`` is the definition's ``rounds`` wherever there is a record."""
    min_support = check_min_support(min_support)
    dev = _require_gpu("cuda" if device is None else device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    nodes = int(nodes)
    if nodes < 0:
        raise ValueError("support_hits: nodes must be >= 0")
    entries, _keep = _upload_lists(lists, nodes, dev, "support_hits")
    words = support_lists_device(entries, nodes, min_score, min_support, dev, stats)
    return [w.cpu().numpy() for w in words]


def _truss_entries(entries, records, nodes: int, min_score: float, min_support: int, dev):
    """The entries of the records that survive the ``(min_support + 2)``-truss: ``nsm_support_hits`` on the device lists,
    then the alive records (word ``>= 0``) compacted on the device.  ``records``: per list its ``[n, 2]`` float64 tensor
    (None for an empty list).  Returns the new entries and the tensors they point into."""
    words = support_lists_device(entries, nodes, min_score, min_support, dev)
    out, keep = [], []
    for (_ptr, n, left_base, left_ids, right_base, right_ids), recs, word in zip(entries, records, words):
        alive = recs[: int(n)][word >= 0] if n else None
        keep.append(alive)
        count = 0 if alive is None else int(alive.shape[0])
        out.append((alive.data_ptr() if count else 0, count, left_base, left_ids, right_base, right_ids))
    return out, keep


# ------------------------------------------------------------------------------- merge forests
def _score_key(score: np.ndarray) -> np.ndarray:
    """``nsm_sort_hits``'s K(score): ascending in this uint64 is descending in the score, by its bits (+0.0 before -0.0)."""
    bits = np.ascontiguousarray(score, dtype=np.float64).view(np.uint64)
    flip = np.where(bits >> np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1) << np.uint64(63))
    return ~(bits ^ flip)


def _check_cut(threshold, min_score: float, what: str) -> float:
    t = float(threshold)
    if not t >= min_score:
        raise ValueError(f"{what}: threshold {threshold!r} is not >= the forest's min_score {min_score!r}; "
                         "the forest does not know what links below it")
    return t


@dataclass
class MergeForest:
    """The merge forest of hit lists over one node space: the maximum spanning forest under the canonical record order,
    i.e. the single-linkage hierarchy.  Record ``k`` joined the groups of nodes ``u[k] < v[k]`` at ``score[k]``; cut at any
    threshold ``>= min_score`` it gives the match groups at that threshold.  Cohort ``c``'s item ``k`` is node
    ``bases[c] + k``, as in ``MatchGroups``."""

    score: np.ndarray  # float64, canonical order (score descending by its bits, then u, then v)
    u: np.ndarray  # int32, the smaller node
    v: np.ndarray  # int32, the larger node
    nodes: int
    bases: tuple
    cohort_sizes: tuple
    min_score: float

    def __len__(self) -> int:
        return int(self.score.shape[0])

    def as_tuples(self):
        return list(zip(self.score.tolist(), self.u.tolist(), self.v.tolist()))

    def hits(self) -> Hits:
        """The records as a hit list over the whole node space (``left_base = right_base = 0``): what
        ``forest(forest(A) u B)`` feeds back."""
        return Hits(self.score, self.u, self.v)

    def cut(self, threshold: float) -> MatchGroups:
        """The match groups at ``threshold``: ``groups_of_hits`` of the lists the forest was built from, label for label.
        ``ValueError`` below ``min_score``, where the forest does not know."""
        t = _check_cut(threshold, self.min_score, "MergeForest.cut")
        return MatchGroups(groups_of_hits([(self.hits(), 0, 0)], self.nodes, t), self.bases, self.cohort_sizes)

    def ladder(self, thresholds) -> dict:
        """Per threshold (any order, each ``>= min_score``): ``components`` (groups of any size), ``groups`` (of at least
        two nodes), ``grouped`` (nodes in such groups) and ``largest`` (the largest group's size) -- the statistics of
        ``cut(t)``, for the whole ladder in ONE pass over the records, int64 arrays in the thresholds' order."""
        ts = np.asarray([_check_cut(t, self.min_score, "MergeForest.ladder") for t in np.asarray(thresholds, dtype=np.float64).ravel()])
        out = {name: np.zeros(len(ts), dtype=np.int64) for name in ("components", "groups", "grouped", "largest")}
        parent, size = list(range(self.nodes)), [1] * self.nodes

        def find(x: int) -> int:
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        score, u, v = self.score.tolist(), self.u.tolist(), self.v.tolist()
        k, groups, grouped, largest = 0, 0, 0, min(self.nodes, 1)
        for slot in np.argsort(-ts, kind="stable").tolist():  # thresholds descending: the records >= t are a growing prefix
            while k < len(score) and score[k] >= ts[slot]:
                a, b = find(u[k]), find(v[k])
                sa, sb = size[a], size[b]
                groups += 1 - (sa >= 2) - (sb >= 2)
                grouped += (sa if sa < 2 else 0) + (sb if sb < 2 else 0)
                parent[b], size[a] = a, sa + sb
                largest = max(largest, sa + sb)
                k += 1
            out["components"][slot], out["groups"][slot] = self.nodes - k, groups
            out["grouped"][slot], out["largest"][slot] = grouped, largest
        return out

    def merge_score(self, a, b) -> np.ndarray:
        """Per pair of nodes ``(a[q], b[q])`` the largest threshold at which they share a group: the score of the record
        that joined their groups; ``-1.0`` if none did (the profiles' "none"), ``+inf`` for ``a == b``."""
        a, b = np.asarray(a, dtype=np.int64).ravel(), np.asarray(b, dtype=np.int64).ravel()
        if a.shape != b.shape:
            raise ValueError("merge_score: a and b must have the same length")
        if len(a) and (min(int(a.min()), int(b.min())) < 0 or max(int(a.max()), int(b.max())) >= self.nodes):
            raise ValueError(f"merge_score: nodes must lie in [0, {self.nodes})")
        out = np.full(len(a), -1.0)
        out[a == b] = np.inf
        # offline: every component carries the open queries with one end in it; the smaller set is merged into the larger
        parent = list(range(self.nodes))
        open_at: dict = {}
        for q, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
            if x != y:
                open_at.setdefault(x, set()).add(q)
                open_at.setdefault(y, set()).add(q)

        def find(x: int) -> int:
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for s, x, y in zip(self.score.tolist(), self.u.tolist(), self.v.tolist()):
            x, y = find(x), find(y)
            qx, qy = open_at.pop(x, set()), open_at.pop(y, set())
            if len(qx) < len(qy):
                qx, qy = qy, qx
            for q in qy:
                if q in qx:
                    qx.discard(q)
                    out[q] = s
                else:
                    qx.add(q)
            parent[y] = x
            if qx:
                open_at[x] = qx
        return out


def _forest_layout(nodes: int, bases, cohort_sizes):
    return ((0,), (nodes,)) if bases is None else (tuple(bases), tuple(cohort_sizes))


def forest_of_hits(lists, nodes: int, min_score: float = 0.0, bases=None, cohort_sizes=None) -> MergeForest:
    """The definition of a merge forest.  ``lists = [(Hits, left_base, right_base), ...]`` as for ``groups_of_hits``: record
    ``(score, i, j)`` joins ``u = left_base + i`` and ``v = right_base + j`` and is an edge iff ``score >= min_score`` and
    ``u != v`` (a NaN links nothing); its value is ``(score, lo, hi)``.  All edges are walked in canonical order -- the
    order of ``nsm_sort_hits``'s key: score descending by its bits (``+0.0`` before ``-0.0``), then lo, then hi -- and an
    edge is taken iff its ends are not yet connected by taken edges (Kruskal).  The taken values, in that order."""
    nodes = int(nodes)
    if nodes < 0:
        raise ValueError("forest_of_hits: nodes must be >= 0")
    min_score = float(min_score)
    parts = []
    for hits, left_base, right_base in lists:
        a, b = _list_nodes(hits, left_base, right_base, nodes, "forest_of_hits")
        s = np.asarray(hits.score, dtype=np.float64)
        keep = (s >= min_score) & (a != b)
        parts.append((s[keep], np.minimum(a, b)[keep], np.maximum(a, b)[keep]))
    score = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.float64)
    lo = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, np.int64)
    hi = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, np.int64)
    order = np.lexsort((hi, lo, _score_key(score)))
    parent = list(range(nodes))

    def find(x: int) -> int:
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    taken = []
    for r, a, b in zip(order.tolist(), lo[order].tolist(), hi[order].tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
            taken.append(r)
    taken = np.asarray(taken, dtype=np.int64)
    return MergeForest(score[taken], lo[taken].astype(np.int32), hi[taken].astype(np.int32), nodes,
                       *_forest_layout(nodes, bases, cohort_sizes), min_score)


def span_lists_device(entries, nodes: int, min_score: float, dev, stats: Optional[list] = None, bases=None,
                      cohort_sizes=None) -> MergeForest:
    """One ``nsm_span_hits`` call over device lists, the forest ordered on the device (``nsm_sort_hits``), and one D2H copy
    of its at most ``nodes - 1`` records.  ``entries``: per list ``(records pointer, n, left_base, left_ids, right_base,
    right_ids)``."""
    fn = _lib.entry("nsm_span_hits")
    nodes = int(nodes)
    layout = _forest_layout(nodes, bases, cohort_sizes)
    if nodes == 0:
        if stats is not None:
            stats[:] = [0, 0, 0, 0]
        return MergeForest(np.zeros(0, np.float64), np.zeros(0, np.int32), np.zeros(0, np.int32), 0, *layout, float(min_score))
    lists = (_lib.NsmHitList * max(1, len(entries)))()
    for slot, (ptr, n, left_base, left_ids, right_base, right_ids) in zip(lists, entries):
        slot.hits, slot.n = (ptr if n else None), int(n)
        slot.left_base, slot.left_ids, slot.right_base, slot.right_ids = int(left_base), int(left_ids), int(right_base), int(right_ids)
    out = HitBuffer(max(1, nodes - 1), dev)
    st = torch.zeros(4, dtype=torch.int64, device=dev) if stats is not None else None
    status = fn(lists, len(entries), nodes, float(min_score), 0, out.records.data_ptr(),
                out.count.data_ptr(), None, st.data_ptr() if st is not None else None, torch.cuda.current_stream(dev).cuda_stream)
    if status == 10001:
        raise ValueError("nsm_span_hits: " + _lib.load().nsm_last_error().decode("utf-8", "replace"))
    _lib.check(status, "nsm_span_hits")
    if stats is not None:
        stats[:] = [int(v) for v in st.tolist()]
    taken = sort_hits_device(out, int(out.count.item()), nodes)
    return MergeForest(taken.score, taken.i, taken.j, nodes, *layout, float(min_score))


def span_hits(lists, nodes: int, min_score: float = 0.0, device=None, stats: Optional[list] = None, bases=None,
              cohort_sizes=None) -> MergeForest:
    """``forest_of_hits(lists, nodes, min_score)`` on the device for host hit lists: upload (in any order), one
    ``nsm_span_hits`` call over all lists, the forest ordered on the device, one D2H copy of at most ``nodes - 1`` records.
    Ids must be ``>= 0`` and every record must stay inside the nodes (``ValueError``).  ``stats`` receives [records with
    score >= min_score, forest records, rounds run, edge visits summed over the rounds]."""
    dev = _require_gpu("cuda" if device is None else device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    nodes = int(nodes)
    if nodes < 0:
        raise ValueError("span_hits: nodes must be >= 0")
    entries, keep = [], []
    for hits, left_base, right_base in lists:
        _list_nodes(hits, left_base, right_base, nodes, "span_hits")
        recs = _records_to_device(hits, dev)
        keep.append(recs)
        entries.append((recs.data_ptr() if recs is not None else 0, len(hits), int(left_base), nodes - int(left_base),
                        int(right_base), nodes - int(right_base)))
    return span_lists_device(entries, nodes, min_score, dev, stats, bases, cohort_sizes)


def _forest_pending(pending: PendingHits, left, right, threshold: float, same: bool, min_score,
                    stats: Optional[list]) -> MergeForest:
    # (nsm_span_hits numbers the nodes by caller id, as nsm_group_hits does)
    ids_l, ids_r = _id_count(left.orig, left.n, "forest"), _id_count(right.orig, right.n, "forest")
    if same:  # one node space: left item k and right item k are the same node
        nodes, bases, sizes = max(ids_l, ids_r), (0,), (max(ids_l, ids_r),)
    else:
        nodes, bases, sizes = ids_l + ids_r, (0, ids_l), (ids_l, ids_r)
    floor = float("-inf") if min_score is None else float(min_score)
    # the buffer goes in UNSORTED and is only read: the call orders its own copy of the edges
    forest = span_lists_device([(pending.buf.records.data_ptr(), pending.n, 0, ids_l, bases[-1], ids_r)], nodes, floor,
                               pending.buf.records.device, stats, bases, sizes)
    forest.min_score = max(floor, float(threshold))  # (the grid knows nothing below its threshold either)
    return forest


def indel_raw_forest(left: StrTable, right: StrTable, threshold: float, prune: bool = True, capacity: Optional[int] = None,
                     two_stage: bool = True, pack: Optional[bool] = None, same: bool = False, min_score: Optional[float] = None,
                     stats: Optional[list] = None, metric: str = "indel") -> MergeForest:
    """``forest_of_hits([(indel_raw_grid(left, right, threshold, ...), 0, right's base)], ...)``: the grid's hits stay in
    their device buffer, are spanned there, and only the forest (fewer records than there are items) crosses to the host.
    ``same``: both tables describe the same items (a self-join), numbered in ONE node space.  ``min_score``: only records
    scoring at least that are edges (None: every hit of the grid; the forest then knows every threshold the grid does)."""
    pending = indel_raw_grid(left, right, threshold, prune=prune, capacity=capacity, two_stage=two_stage, pack=pack, defer=True,
                             metric=metric)
    return _forest_pending(pending, left, right, threshold, same, min_score, stats)


def jaccard_raw_forest(left: SetTable, right: SetTable, threshold: float, prune: bool = True, capacity: Optional[int] = None,
                       index: Optional[bool] = None, same: bool = False, min_score: Optional[float] = None,
                       stats: Optional[list] = None, measure: str = "union") -> MergeForest:
    """``intersection_vs_union`` counterpart of ``indel_raw_forest`` (``measure`` as for ``jaccard_raw_grid``)."""
    pending = jaccard_raw_grid(left, right, threshold, prune=prune, capacity=capacity, index=index, defer=True, measure=measure)
    return _forest_pending(pending, left, right, threshold, same, min_score, stats)


def indel_levels_forest(left: LevelItems, left_strings: StrTable, right: LevelItems, right_strings: StrTable, threshold: float,
                        category_mode: int = _lib.CAT_NONE, prune: bool = True, capacity: Optional[int] = None, same: bool = False,
                        min_score: Optional[float] = None, stats: Optional[list] = None, **grid_options) -> MergeForest:
    """``forest_of_hits`` of ``indel_levels_grid(...)``'s hits without them leaving the device (``grid_options``: the grid's
    other keywords)."""
    pending = indel_levels_grid(left, left_strings, right, right_strings, threshold, category_mode=category_mode, prune=prune,
                                capacity=capacity, defer=True, **grid_options)
    return _forest_pending(pending, left, right, threshold, same, min_score, stats)


def jaccard_levels_forest(left: SetTable, right: SetTable, threshold: float, category_mode: int = _lib.CAT_NONE,
                          prune: bool = True, capacity: Optional[int] = None, index: Optional[bool] = None, same: bool = False,
                          min_score: Optional[float] = None, stats: Optional[list] = None, measure: str = "union",
                          banned=None) -> MergeForest:
    """``intersection_vs_union`` counterpart of ``indel_levels_forest`` (``measure``, ``banned`` as for ``jaccard_levels_grid``)."""
    pending = jaccard_levels_grid(left, right, threshold, category_mode=category_mode, prune=prune, capacity=capacity,
                                  index=index, defer=True, measure=measure, banned=banned)
    return _forest_pending(pending, left, right, threshold, same, min_score, stats)
