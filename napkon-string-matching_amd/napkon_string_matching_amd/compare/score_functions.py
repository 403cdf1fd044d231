"""The score_func plugin module, MI355X edition.

Same names, call convention and error behaviour as the reference's
``napkon_string_matching/compare/score_functions.py`` (:6-27): callables
``(left, right) -> float`` looked up BY NAME (types/comparable_data.py:150), plus
``join_sorted``.  Each plugin has two faces:

* calling it scores ONE pair -- as a 1 x 1 grid on the GPU, through the same kernels as the
  batched path (there is no CPU implementation of the arithmetic in this package);
* ``plugin.raw_grid(left_items, right_items, threshold)`` / the levels builders used by
  ``ComparableData.gen_comparable`` score N x M pairs in one launch;
* ``plugin.top_k(left_items, right_items, k, threshold)`` keeps the ``k`` best right items of every left item
  (score descending, right index ascending among equals) -- rapidfuzz's ``process.extract(query, choices, scorer,
  limit, score_cutoff)`` for all queries at once; the output is bounded by N k records whatever the data.  With
  ``groups=`` (one hashable per right item) it keeps the best item of every group and of those the ``k`` best: the
  ``k`` best distinct candidates when the right side lists a candidate under several spellings.

* ``plugin.pairs(left_items, right_items, pairs)`` scores a LIST of ``(i, j)`` pairs in O(P) -- rapidfuzz's
  ``process.cpdist``: what do these particular pairs score?

* ``plugin.profile(left_items, right_items, thresholds)`` answers what a whole ladder of thresholds would do -- hit counts
  per threshold and every item's best score -- without the hits (``grid.ThresholdProfile``).

* ``plugin.best(left_items, right_items, margin, threshold, mutual)`` keeps every left item's best match together with
  everything within ``margin`` of it -- all its ties at ``margin=0``, which no fixed ``k`` returns -- and with
  ``mutual=True`` only the pairs that are best from both sides (reciprocal best hits).

* ``plugin.assign(left_items, right_items, threshold)`` turns the match list into a one-to-one mapping: the best pair, both
  its items removed, and again (``grid.assign_of_hits``), assigned on the device.

* ``plugin.groups(left_items, right_items, threshold)`` closes the match list transitively: the connected components of
  the pairs scoring ``>= threshold`` (``grid.groups_of_hits``), linked on the device; ``plugin.clusters(items, threshold)``
  is the self-join -- near-duplicate clusters inside one list.

* ``plugin.forest(left_items, right_items, threshold)`` is the groups at EVERY threshold ``>= threshold`` from one run: the
  merge forest (``grid.forest_of_hits``), spanned on the device -- ``cut(t)``, ``ladder(thresholds)``, ``merge_score(a, b)``;
  ``plugin.cluster_tree(items, threshold)`` is the self-join.

Beside the reference's two functions the module holds three more token-set measures with the same faces --
``intersection_vs_mean`` (Sorensen-Dice), ``intersection_vs_smaller`` (overlap coefficient) and ``intersection_vs_left``
(containment of left in right): ``intersection_vs_union``'s class with another ``measure``.

On the string side ``levenshtein_match`` (normalised Levenshtein similarity) and ``levenshtein_within`` (best approximate
occurrence of the left string inside the right one) stand beside ``fuzzy_match`` in the same way: ``fuzzy_match``'s class
with another ``metric``.

``default_process`` / ``join_sorted`` are per-item string preparation and stay on the host; the
reference re-does them for every pair (score_functions.py:24-25 inside the hot loop).
"""
from __future__ import annotations

import re
from typing import Iterable, List, Sequence, Union

import numpy as np
import torch

from .. import grid, tables

_NON_WORD = re.compile(r"\W", re.UNICODE)        # keeps "_": what rapidfuzz 2.1's pure-Python fallback does
_NON_ALNUM = re.compile(r"[\W_]", re.UNICODE)    # blanks "_" too: "non alphanumeric", the compiled implementation

# How ``default_process`` treats "_" -- the one point where rapidfuzz 2.1's two implementations of it differ:
# the C++ one (what a pip-installed wheel runs, and what its documentation describes: "removing all non
# alphanumeric characters") blanks it, the pure-Python fallback (``re.sub(r"(?ui)\W", " ", s)``) keeps it.
# rapidfuzz is not installable offline, so this cannot be pinned against the pinned version; the switch is
# explicit instead of buried in a regex.  Synthetic corpora only use ``[a-z0-9 ]``, a fixed point of both.
UNDERSCORE_POLICIES = ("blank", "keep")
UNDERSCORE_POLICY = "blank"

Operand = Union[str, List[str]]


def _device():
    if not torch.cuda.is_available():
        from .._lib import NsmLibraryError

        raise NsmLibraryError("score functions run on an MI355X (HIP device); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def join_sorted(value: Sequence[str]) -> str:
    """score_functions.py:16-17."""
    return " ".join(sorted(value, key=str.lower))


def default_process(text: str, underscore: str = None) -> str:
    """rapidfuzz 2.x ``utils.default_process`` (applied by ``fuzz.QRatio`` by default in the
    pinned 2.1 line): non-alphanumeric code points -> blank, strip, lower-case.  ``underscore``:
    "blank" or "keep" (default: the module's ``UNDERSCORE_POLICY``)."""
    policy = UNDERSCORE_POLICY if underscore is None else underscore
    if policy not in UNDERSCORE_POLICIES:
        raise ValueError(f"underscore policy must be one of {UNDERSCORE_POLICIES}")
    return (_NON_ALNUM if policy == "blank" else _NON_WORD).sub(" ", text).strip().lower()


def fuzzy_operand(value: Operand) -> str:
    """What ``fuzzy_match`` feeds to the Indel ratio for one operand (score_functions.py:24-25
    followed by QRatio's default processor)."""
    return default_process(join_sorted(value) if isinstance(value, list) else value)


def factorise_groups(groups, n_right: int):
    """``groups`` of a grouped ``top_k`` (any sequence of hashables, one per right item) as an int32 array of dense ids;
    ``None`` stays ``None``.  A wrong length is a ``ValueError``, before any device work."""
    if groups is None:
        return None
    groups = list(groups)
    if len(groups) != n_right:
        raise ValueError(f"{len(groups)} groups for {n_right} right items")
    ids = {}
    return np.fromiter((ids.setdefault(g, len(ids)) for g in groups), dtype=np.int32, count=len(groups))


def set_operand(value: Operand) -> Iterable[str]:
    """What ``intersection_vs_union`` turns one operand into (score_functions.py:10-11)."""
    return value if isinstance(value, list) else value.split()


def _padded_ids(rows, vocab, width: int) -> np.ndarray:
    """Token rows as the int array ``SetTable.from_padded`` takes: distinct ids first, -1 behind them."""
    ids = np.full((len(rows), width), -1, dtype=np.int32)
    for k, row in enumerate(rows):
        uniq = list(dict.fromkeys(vocab.id(tok) for tok in row))
        ids[k, : len(uniq)] = uniq
    return ids


def _best(profile, split, n_left: int, n_right: int, margin: float, threshold: float, mutual: bool, fast, general) -> grid.Hits:
    """Best matches of a plugin grid in two passes.  Pass 1: ``profile([threshold])``, the plugin's own profile routing --
    it merges the wide parts, so the bests are global.  Pass 2: the grid cut as ``wide.split_grid`` cuts it (``split``:
    (wide_l, wide_r) or None); ``fast(li, ri, left_floor, right_floor)`` is the floor grid of a sub-grid with the floors
    gathered to its sub-tables, ``general(li, ri)`` the general kernel's hits at ``threshold``, gated on the host."""
    from .. import wide

    if not n_left or not n_right:
        return wide.merge([])
    lf, rf = grid.floors_of_profile(profile([threshold]), margin, mutual)
    take = lambda floor, idx: None if floor is None else floor[np.asarray(idx, dtype=np.int64)]
    fast_part = lambda li, ri: fast(li, ri, take(lf, li), take(rf, ri))
    general_part = lambda li, ri: grid.filter_by_floors(general(li, ri), take(lf, li), take(rf, ri))
    if split is None:
        return fast_part(range(n_left), range(n_right))
    return wide.split_grid(split[0], split[1], fast_part, general_part)


class _IntersectionVsUnion:
    """``len(A & B) / len(A | B)`` of the two token sets (Jaccard; score_functions.py:6-13).  The token-set measures below
    are this class with another ``measure``: every method here hands ``self.measure`` to the ``grid.jaccard_*`` wrapper it
    uses (``"union"`` keeps each wrapper's own route) and takes its ``ZeroDivisionError`` rule from ``divides_by_zero``."""
    __name__ = "intersection_vs_union"
    kind = "sets"
    measure = "union"  # grid.check_measure: which quotient the device computes

    def __call__(self, left: Operand, right: Operand) -> float:
        hits = self.raw_grid([left], [right], float("-inf"))
        return float(hits.score[0])

    def divides_by_zero(self, a, b) -> bool:
        """Does the score of a left set ``a`` and a right set ``b`` (sets, or their sizes) divide by zero?"""
        size = lambda x: x if isinstance(x, (int, np.integer)) else len(x)
        return grid.measure_divides_by_zero(self.measure, size(a), size(b))

    def _rows(self, left_items, right_items):
        """Both sides as token lists.  A measure beside Jaccard checks here what it cannot score, before the device is asked
        for: the whole grid's ``ZeroDivisionError`` (``grid.check_measure_grid``) and items beyond the fast kernels."""
        l_rows = [list(set_operand(v)) for v in left_items]
        r_rows = [list(set_operand(v)) for v in right_items]
        if self.measure != "union":
            grid.check_measure_grid(self.measure, any(not r for r in l_rows), len(l_rows), any(not r for r in r_rows), len(r_rows))
            self._check_narrow(l_rows, r_rows)
        return l_rows, r_rows

    def _check_narrow(self, *sides) -> None:
        from .. import wide

        if self.measure != "union" and any(len(set(r)) > wide.FAST_TOKENS for rows in sides for r in rows):
            raise NotImplementedError(f"{self.__name__}: an item of more than {wide.FAST_TOKENS} distinct tokens (measure "
                                      f"{self.measure!r} has no general kernel)")

    def raw_grid(self, left_items: Sequence[Operand], right_items: Sequence[Operand], threshold: float, device=None,
                 prune: bool = True) -> grid.Hits:
        from .. import wide

        l_rows, r_rows = self._rows(left_items, right_items)
        dev = device or _device()

        def fast(li, ri):
            vocab = tables.Vocabulary()
            ls, rs = [l_rows[k] for k in li], [r_rows[k] for k in ri]
            width = tables.pick_width(max((len(set(r)) for r in ls), default=1), max((len(set(r)) for r in rs), default=1))
            lt = tables.SetTable.from_rows(ls, "left", dev, vocab, width=width)
            rt = tables.SetTable.from_rows(rs, "right", dev, vocab, width=width)
            return grid.jaccard_raw_grid(lt, rt, threshold, prune=prune, measure=self.measure)

        split = wide.wide_set_items([[r] for r in l_rows], [[r] for r in r_rows])
        if split is None:
            return fast(range(len(l_rows)), range(len(r_rows)))
        # items of more than 64 distinct tokens (the reference's set(...) has no size limit, score_functions.py:10-13)
        if any(not r for r in l_rows) and any(not r for r in r_rows):
            raise ZeroDivisionError("division by zero")  # (:13, checked on the whole grid before it is split)
        general = lambda li, ri: wide.jaccard_any_grid([[l_rows[k]] for k in li], [[r_rows[k]] for k in ri], threshold,
                                                       raw=True, device=dev)
        return wide.split_grid(split[0], split[1], fast, general)

    def top_k(self, left_items: Sequence[Operand], right_items: Sequence[Operand], k: int, threshold: float = 0.0, device=None,
              prune: bool = True, groups=None) -> grid.Hits:
        """Per left item the first ``k`` records of ``raw_grid(left_items, right_items, threshold)`` (score descending,
        right index ascending), all of them in canonical order.  ``groups`` (hashables, one per right item): right items
        of one group are spellings of one candidate -- per left item only the best record of every group is kept, and of
        those the first ``k``: the ``k`` best DISTINCT candidates."""
        from .. import wide

        k = grid.check_k(k)
        gids = factorise_groups(groups, len(right_items))
        l_rows, r_rows = self._rows(left_items, right_items)
        dev = device or _device()
        if any(not r for r in l_rows) and any(not r for r in r_rows):
            raise ZeroDivisionError("division by zero")  # (:13)

        sub = lambda ri: None if gids is None else gids[np.asarray(ri, dtype=np.int64)]

        def fast(li, ri):
            vocab = tables.Vocabulary()
            ls, rs = [l_rows[k_] for k_ in li], [r_rows[k_] for k_ in ri]
            width = tables.pick_width(max((len(set(r)) for r in ls), default=1), max((len(set(r)) for r in rs), default=1))
            lt = tables.SetTable.from_rows(ls, "left", dev, vocab, width=width)
            rt = tables.SetTable.from_rows(rs, "right", dev, vocab, width=width)
            return grid.jaccard_raw_top_k(lt, rt, k, threshold, prune=prune, groups=sub(ri), measure=self.measure)

        split = wide.wide_set_items([[r] for r in l_rows], [[r] for r in r_rows])
        if split is None:
            return fast(range(len(l_rows)), range(len(r_rows)))
        # items of more than 64 distinct tokens: the general kernel at `threshold`; the parts are disjoint in j for every
        # i, so the union of their per-row selections holds the answer (grouped: a representative among the first k of
        # the whole row is the best of its group in its own part, and fewer than k groups beat it there)
        general = lambda li, ri: grid.select_top_k(
            wide.jaccard_any_grid([[l_rows[k_]] for k_ in li], [[r_rows[k_]] for k_ in ri], threshold, raw=True, device=dev), k,
            sub(ri))
        return grid.select_top_k(wide.split_grid(split[0], split[1], fast, general), k, gids)


    def pairs(self, left_items: Sequence[Operand], right_items: Sequence[Operand], pairs, device=None) -> np.ndarray:
        """The score of every listed pair: ``pairs`` is a sequence of ``(i, j)`` positions in the two item lists, or a
        P x 2 integer array; the result is ``[plugin(left_items[i], right_items[j]) for i, j in pairs]`` as a float64 array,
        in O(P) (``nsm_jaccard_raw_pairs``: tables of the listed items only, one launch).  A listed pair of two empty sets
        raises ``ZeroDivisionError`` as the plugin does (:13) -- a per-pair check here, not the whole-grid one.  A pair
        with an item of more than 64 distinct tokens goes through the general grid, one call per distinct left item of
        such pairs over its listed partners: slow, and meant for the rare item that needs it."""
        from .. import wide

        i, j = wide.check_pair_positions(pairs, len(left_items), len(right_items))
        l_rows = {int(k): list(set_operand(left_items[k])) for k in np.unique(i)}
        r_rows = {int(k): list(set_operand(right_items[k])) for k in np.unique(j)}
        if any(self.divides_by_zero(set(l_rows[int(a)]), set(r_rows[int(b)])) for a, b in zip(i, j)):
            raise ZeroDivisionError("division by zero")  # (:13)
        self._check_narrow(l_rows.values(), r_rows.values())
        if len(i) == 0:
            return np.zeros(0, dtype=np.float64)
        dev = device or _device()

        def fast(li, ri, pi, pj):
            vocab = tables.Vocabulary()
            ls, rs = [l_rows[int(k)] for k in li], [r_rows[int(k)] for k in ri]
            width = tables.pick_width(max((len(set(r)) for r in ls), default=1), max((len(set(r)) for r in rs), default=1))
            lt = tables.SetTable.from_padded(_padded_ids(ls, vocab, width), "left", dev, width=width, validate=False, index=False)
            rt = tables.SetTable.from_padded(_padded_ids(rs, vocab, width), "right", dev, width=width, validate=False, index=False)
            return grid.jaccard_raw_pairs(lt, rt, pi, pj, measure=self.measure)

        general = lambda li, ri: wide.jaccard_any_grid([[l_rows[int(k)]] for k in li], [[r_rows[int(k)]] for k in ri],
                                                       float("-inf"), raw=True, device=dev)
        n_l, n_r = len(left_items), len(right_items)
        big = lambda rows, n: np.fromiter((len(set(rows.get(k, ()))) > wide.FAST_TOKENS for k in range(n)), dtype=bool, count=n)
        wide_l, wide_r = big(l_rows, n_l), big(r_rows, n_r)
        split = (wide_l, wide_r) if wide_l.any() or wide_r.any() else None
        return wide.split_pairs(split, i, j, fast, general)

    def profile(self, left_items: Sequence[Operand], right_items: Sequence[Operand], thresholds, device=None,
                prune: bool = True) -> grid.ThresholdProfile:
        """``grid.profile_of_hits(raw_grid(left_items, right_items, thresholds[0]), thresholds, ...)`` without the hits:
        per threshold the number of pairs scoring at least that, per item its best score (``-1.0``: none at
        ``thresholds[0]``).  Wide items are routed as ``top_k`` routes them."""
        from .. import wide

        t = grid.check_thresholds(thresholds)
        l_rows, r_rows = self._rows(left_items, right_items)
        dev = device or _device()
        if any(not r for r in l_rows) and any(not r for r in r_rows):
            raise ZeroDivisionError("division by zero")  # (:13)

        def fast(li, ri):
            vocab = tables.Vocabulary()
            ls, rs = [l_rows[k_] for k_ in li], [r_rows[k_] for k_ in ri]
            width = tables.pick_width(max((len(set(r)) for r in ls), default=1), max((len(set(r)) for r in rs), default=1))
            lt = tables.SetTable.from_rows(ls, "left", dev, vocab, width=width)
            rt = tables.SetTable.from_rows(rs, "right", dev, vocab, width=width)
            return grid.jaccard_raw_profile(lt, rt, t, prune=prune, measure=self.measure)

        general = lambda li, ri: grid.profile_of_hits(
            wide.jaccard_any_grid([[l_rows[k_]] for k_ in li], [[r_rows[k_]] for k_ in ri], float(t[0]), raw=True, device=dev),
            t, len(li), len(ri))
        return wide.split_profile(wide.wide_set_items([[r] for r in l_rows], [[r] for r in r_rows]), len(l_rows), len(r_rows),
                                  t, fast, general)

    def best(self, left_items: Sequence[Operand], right_items: Sequence[Operand], margin: float = 0.0, threshold: float = 0.0,
             mutual: bool = False, device=None, prune: bool = True) -> grid.Hits:
        """``grid.best_of_hits(raw_grid(left_items, right_items, threshold), margin, mutual)`` without the grid's hits:
        every left item's best match with everything within ``margin`` of it (``margin=0``: all its ties); ``mutual``: only
        the pairs also within ``margin`` of the right item's best.  Wide items are routed as ``profile`` routes them."""
        from .. import wide

        margin = grid.check_margin(margin)
        grid.check_thresholds([threshold])
        l_rows, r_rows = self._rows(left_items, right_items)
        dev = device or _device()
        if any(not r for r in l_rows) and any(not r for r in r_rows):
            raise ZeroDivisionError("division by zero")  # (:13)

        def fast(li, ri, lf, rf):
            vocab = tables.Vocabulary()
            ls, rs = [l_rows[k_] for k_ in li], [r_rows[k_] for k_ in ri]
            width = tables.pick_width(max((len(set(r)) for r in ls), default=1), max((len(set(r)) for r in rs), default=1))
            lt = tables.SetTable.from_rows(ls, "left", dev, vocab, width=width)
            rt = tables.SetTable.from_rows(rs, "right", dev, vocab, width=width)
            return grid.jaccard_raw_floor_grid(lt, rt, threshold, lf, rf, prune=prune, measure=self.measure)

        general = lambda li, ri: wide.jaccard_any_grid([[l_rows[k_]] for k_ in li], [[r_rows[k_]] for k_ in ri], threshold,
                                                       raw=True, device=dev)
        return _best(lambda t: self.profile(left_items, right_items, t, device=dev, prune=prune),
                     wide.wide_set_items([[r] for r in l_rows], [[r] for r in r_rows]), len(l_rows), len(r_rows), margin,
                     threshold, mutual, fast, general)

    def assign(self, left_items: Sequence[Operand], right_items: Sequence[Operand], threshold: float, device=None,
               prune: bool = True) -> grid.Hits:
        """``grid.assign_of_hits(raw_grid(left_items, right_items, threshold))``: a one-to-one mapping between the two lists
        -- the best pair, both its items removed, and again (ties by left then right index) -- of the pairs scoring
        ``>= threshold``.  ``threshold`` is required: at 0 the hit list is the whole N x M grid.  The hits are ordered and
        assigned on the device and only the assignment (at most min(N, M) records) comes back; where wide items send part
        of the grid through the general kernels the merged host list goes through ``grid.assign_hits``."""
        from .. import wide

        grid.check_thresholds([threshold])
        l_rows, r_rows = self._rows(left_items, right_items)
        dev = device or _device()
        if not l_rows or not r_rows:
            return wide.merge([])
        if wide.wide_set_items([[r] for r in l_rows], [[r] for r in r_rows]) is not None:
            return grid.assign_hits(self.raw_grid(left_items, right_items, threshold, device=dev, prune=prune), len(l_rows),
                                    len(r_rows), device=dev)
        vocab = tables.Vocabulary()
        width = tables.pick_width(max((len(set(r)) for r in l_rows), default=1), max((len(set(r)) for r in r_rows), default=1))
        lt = tables.SetTable.from_rows(l_rows, "left", dev, vocab, width=width)
        rt = tables.SetTable.from_rows(r_rows, "right", dev, vocab, width=width)
        return grid.jaccard_raw_assign(lt, rt, threshold, prune=prune, measure=self.measure)

    def groups(self, left_items: Sequence[Operand], right_items: Sequence[Operand], threshold: float, device=None,
               prune: bool = True, same: bool = False, min_support=0) -> grid.MatchGroups:
        """``grid.groups_of_hits`` of ``raw_grid(left_items, right_items, threshold)``: the items of both lists grouped by
        the pairs scoring ``>= threshold``, closed transitively (left item k is node k, right item k node N + k; with
        ``same`` both lists are the same items in one node space).  The hits are linked on the device, unsorted, and only
        the labels come back; where wide items send part of the grid through the general kernels the merged host list goes
        through ``grid.group_hits``.  ``min_support > 0``: only the pairs of the ``(min_support + 2)``-truss link (every
        linking pair has that many common neighbours among the linking pairs; ``grid.group_hits`` has the definition), so
        chains fall apart -- for ``same=True``: two separate lists are a bipartite graph without common neighbours."""
        from .. import wide

        grid.check_thresholds([threshold])
        min_support = grid.check_min_support(min_support)
        l_rows, r_rows = self._rows(left_items, right_items)
        dev = device or _device()
        n_l, n_r = len(l_rows), len(r_rows)
        layout = ((0,), (max(n_l, n_r),)) if same else ((0, n_l), (n_l, n_r))
        if not l_rows or not r_rows:
            return grid.MatchGroups(np.arange(sum(layout[1]), dtype=np.int32), *layout)
        if wide.wide_set_items([[r] for r in l_rows], [[r] for r in r_rows]) is not None:
            hits = self.raw_grid(left_items, right_items, threshold, device=dev, prune=prune)
            return grid.MatchGroups(grid.group_hits([(hits, 0, layout[0][-1])], sum(layout[1]), float("-inf"), device=dev,
                                                    min_support=min_support), *layout)
        vocab = tables.Vocabulary()
        width = tables.pick_width(max((len(set(r)) for r in l_rows), default=1), max((len(set(r)) for r in r_rows), default=1))
        lt = tables.SetTable.from_rows(l_rows, "left", dev, vocab, width=width)
        rt = tables.SetTable.from_rows(r_rows, "right", dev, vocab, width=width)
        return grid.jaccard_raw_groups(lt, rt, threshold, prune=prune, same=same, measure=self.measure, min_support=min_support)

    def clusters(self, items: Sequence[Operand], threshold: float, device=None, prune: bool = True,
                 min_support=0) -> List[np.ndarray]:
        """Near-duplicate clusters inside ONE list (dedupe): the self-join's groups of at least two items, each an
        ascending array of positions in ``items``, ordered by their smallest member.  ``min_support``: as for ``groups`` -- with 1 a chain of
        near-duplicates no longer swallows the list, every linking pair needs a third item close to both."""
        groups = self.groups(items, items, threshold, device=device, prune=prune, same=True, min_support=min_support)
        return [members[0] for members in groups.members(2)]

    def forest(self, left_items: Sequence[Operand], right_items: Sequence[Operand], threshold: float, device=None,
               prune: bool = True, same: bool = False) -> grid.MergeForest:
        """``grid.forest_of_hits`` of ``raw_grid(left_items, right_items, threshold)``: the merge forest of the pairs scoring
        ``>= threshold`` -- ``groups`` at every threshold from there up in one run (``cut(t)``), with the score that joined
        two items (``merge_score``) and the group statistics of a whole ladder (``ladder``).  Nodes as in ``groups``.  The
        hits are spanned on the device and only the forest comes back; where wide items send part of the grid through the
        general kernels the merged host list goes through ``grid.span_hits``."""
        from .. import wide

        grid.check_thresholds([threshold])
        l_rows, r_rows = self._rows(left_items, right_items)
        dev = device or _device()
        n_l, n_r = len(l_rows), len(r_rows)
        layout = ((0,), (max(n_l, n_r),)) if same else ((0, n_l), (n_l, n_r))
        if not l_rows or not r_rows:
            return grid.forest_of_hits([], sum(layout[1]), float(threshold), *layout)
        if wide.wide_set_items([[r] for r in l_rows], [[r] for r in r_rows]) is not None:
            hits = self.raw_grid(left_items, right_items, threshold, device=dev, prune=prune)
            return grid.span_hits([(hits, 0, layout[0][-1])], sum(layout[1]), float(threshold), device=dev, bases=layout[0],
                                  cohort_sizes=layout[1])
        vocab = tables.Vocabulary()
        width = tables.pick_width(max((len(set(r)) for r in l_rows), default=1), max((len(set(r)) for r in r_rows), default=1))
        lt = tables.SetTable.from_rows(l_rows, "left", dev, vocab, width=width)
        rt = tables.SetTable.from_rows(r_rows, "right", dev, vocab, width=width)
        return grid.jaccard_raw_forest(lt, rt, threshold, prune=prune, same=same, measure=self.measure)

    def cluster_tree(self, items: Sequence[Operand], threshold: float, device=None, prune: bool = True) -> grid.MergeForest:
        """The single-linkage tree of ONE list: the self-join's merge forest (node k is ``items[k]``); ``cut(t).members(2)``
        are ``clusters(items, t)`` for every ``t >= threshold``."""
        return self.forest(items, items, threshold, device=device, prune=prune, same=True)


class _FuzzyMatch:
    """The Indel ratio ``2 LCS / (la + lb)`` of the two prepared strings (QRatio / 100; score_functions.py:20-27).  The
    Levenshtein score functions below are this class with another ``metric``: every method here hands ``self.metric`` to
    the ``grid.indel_*`` wrapper it uses (``"indel"`` keeps each wrapper's own route)."""
    __name__ = "fuzzy_match"
    kind = "strings"
    metric = "indel"  # grid.check_metric: which score the device computes

    def __call__(self, left: Operand, right: Operand) -> float:
        hits = self.raw_grid([left], [right], float("-inf"))
        return float(hits.score[0])

    def _split(self, items_l, items_r):
        """``wide.wide_string_items``: which items lie beyond the fast kernels (None: none).  The general kernels are
        Indel-only, so another metric raises here, before the device is asked."""
        from .. import wide

        split = wide.wide_string_items(items_l, items_r)
        if split is not None and self.metric != "indel":
            raise NotImplementedError(f"{self.__name__}: a string beyond the fast kernels (more than {wide.FAST_LEN} code "
                                      f"units, or more than 255 distinct code units in the grid; metric {self.metric!r} has "
                                      "no general kernel)")
        return split

    def raw_grid(self, left_items: Sequence[Operand], right_items: Sequence[Operand], threshold: float, device=None,
                 prune: bool = True) -> grid.Hits:
        from .. import wide

        l_ops, r_ops = [fuzzy_operand(v) for v in left_items], [fuzzy_operand(v) for v in right_items]
        split = self._split([[s] for s in l_ops], [[s] for s in r_ops])  # (before the device is asked for)
        dev = device or _device()

        def fast(li, ri):
            lt, rt = tables.encode_strings([l_ops[k] for k in li], [r_ops[k] for k in ri], dev)
            return grid.indel_raw_grid(lt, rt, threshold, prune=prune, metric=self.metric)

        if split is None:
            return fast(range(len(l_ops)), range(len(r_ops)))
        # strings of more than 512 code units / more than 255 distinct code units (rapidfuzz has no such limit, :27)
        general = lambda li, ri: wide.indel_any_grid([[l_ops[k]] for k in li], [[r_ops[k]] for k in ri], threshold, raw=True,
                                                     device=dev)
        return wide.split_grid(split[0], split[1], fast, general)

    def top_k(self, left_items: Sequence[Operand], right_items: Sequence[Operand], k: int, threshold: float = 0.0, device=None,
              prune: bool = True, groups=None) -> grid.Hits:
        """Per left item the first ``k`` records of ``raw_grid(left_items, right_items, threshold)`` (score descending,
        right index ascending), all of them in canonical order.  ``groups`` (hashables, one per right item): right items
        of one group are spellings of one candidate -- per left item only the best record of every group is kept, and of
        those the first ``k``: the ``k`` best DISTINCT candidates (``MeshProvider.get_matches``' one row per Id)."""
        from .. import wide

        k = grid.check_k(k)
        gids = factorise_groups(groups, len(right_items))
        l_ops, r_ops = [fuzzy_operand(v) for v in left_items], [fuzzy_operand(v) for v in right_items]
        split = self._split([[s] for s in l_ops], [[s] for s in r_ops])  # (before the device is asked for)
        dev = device or _device()
        sub = lambda ri: None if gids is None else gids[np.asarray(ri, dtype=np.int64)]

        def fast(li, ri):
            lt, rt = tables.encode_strings([l_ops[k_] for k_ in li], [r_ops[k_] for k_ in ri], dev)
            return grid.indel_raw_top_k(lt, rt, k, threshold, prune=prune, groups=sub(ri), metric=self.metric)

        if split is None:
            return fast(range(len(l_ops)), range(len(r_ops)))
        # strings beyond the fast kernels: the general kernel at `threshold`; the parts are disjoint in j for every i, so
        # the union of their per-row selections holds the answer (grouped: as for intersection_vs_union.top_k)
        general = lambda li, ri: grid.select_top_k(
            wide.indel_any_grid([[l_ops[k_]] for k_ in li], [[r_ops[k_]] for k_ in ri], threshold, raw=True, device=dev), k,
            sub(ri))
        return grid.select_top_k(wide.split_grid(split[0], split[1], fast, general), k, gids)


    def pairs(self, left_items: Sequence[Operand], right_items: Sequence[Operand], pairs, device=None) -> np.ndarray:
        """The score of every listed pair: ``pairs`` is a sequence of ``(i, j)`` positions in the two item lists, or a
        P x 2 integer array; the result is ``[plugin(left_items[i], right_items[j]) for i, j in pairs]`` as a float64 array,
        in O(P) -- rapidfuzz's ``process.cpdist`` (``nsm_indel_raw_pairs``: tables of the listed items only, one launch).
        A pair with a string beyond the fast kernels (more than 512 code units, a code unit outside the 255 most frequent)
        goes through the general grid, one call per distinct left item of such pairs over its listed partners: slow, and
        meant for the rare item that needs it."""
        from .. import wide

        i, j = wide.check_pair_positions(pairs, len(left_items), len(right_items))
        if len(i) == 0:
            return np.zeros(0, dtype=np.float64)
        l_ops = {int(k): fuzzy_operand(left_items[k]) for k in np.unique(i)}
        r_ops = {int(k): fuzzy_operand(right_items[k]) for k in np.unique(j)}
        n_l, n_r = len(left_items), len(right_items)
        split = self._split([[l_ops.get(k, "")] for k in range(n_l)], [[r_ops.get(k, "")] for k in range(n_r)])  # (before the device)
        dev = device or _device()

        def fast(li, ri, pi, pj):
            lt, rt = tables.encode_strings([l_ops[int(k)] for k in li], [r_ops[int(k)] for k in ri], dev)
            return grid.indel_raw_pairs(lt, rt, pi, pj, metric=self.metric)

        general = lambda li, ri: wide.indel_any_grid([[l_ops[int(k)]] for k in li], [[r_ops[int(k)]] for k in ri], float("-inf"),
                                                     raw=True, device=dev)
        return wide.split_pairs(split, i, j, fast, general)

    def profile(self, left_items: Sequence[Operand], right_items: Sequence[Operand], thresholds, device=None,
                prune: bool = True) -> grid.ThresholdProfile:
        """``grid.profile_of_hits(raw_grid(left_items, right_items, thresholds[0]), thresholds, ...)`` without the hits:
        per threshold the number of pairs scoring at least that, per item its best score (``-1.0``: none at
        ``thresholds[0]``) -- at 0.0 every pair counts, which no hit list could hold.  Wide items are routed as ``top_k``
        routes them."""
        from .. import wide

        t = grid.check_thresholds(thresholds)
        l_ops, r_ops = [fuzzy_operand(v) for v in left_items], [fuzzy_operand(v) for v in right_items]
        split = self._split([[s] for s in l_ops], [[s] for s in r_ops])  # (before the device is asked for)
        dev = device or _device()

        def fast(li, ri):
            lt, rt = tables.encode_strings([l_ops[k_] for k_ in li], [r_ops[k_] for k_ in ri], dev)
            return grid.indel_raw_profile(lt, rt, t, prune=prune, metric=self.metric)

        general = lambda li, ri: grid.profile_of_hits(
            wide.indel_any_grid([[l_ops[k_]] for k_ in li], [[r_ops[k_]] for k_ in ri], float(t[0]), raw=True, device=dev),
            t, len(li), len(ri))
        return wide.split_profile(split, len(l_ops), len(r_ops),
                                  t, fast, general)

    def best(self, left_items: Sequence[Operand], right_items: Sequence[Operand], margin: float = 0.0, threshold: float = 0.0,
             mutual: bool = False, device=None, prune: bool = True) -> grid.Hits:
        """``grid.best_of_hits(raw_grid(left_items, right_items, threshold), margin, mutual)`` without the grid's hits --
        at threshold 0.0 that grid is N M records: every left item's best match with everything within ``margin`` of it
        (``margin=0``: all its ties, which ``top_k(k=1)`` cuts in ``j`` order); ``mutual``: only the pairs also within
        ``margin`` of the right item's best (reciprocal best hits).  Wide items are routed as ``profile`` routes them."""
        from .. import wide

        margin = grid.check_margin(margin)
        grid.check_thresholds([threshold])
        l_ops, r_ops = [fuzzy_operand(v) for v in left_items], [fuzzy_operand(v) for v in right_items]
        split = self._split([[s] for s in l_ops], [[s] for s in r_ops])  # (before the device is asked for)
        dev = device or _device()

        def fast(li, ri, lf, rf):
            lt, rt = tables.encode_strings([l_ops[k_] for k_ in li], [r_ops[k_] for k_ in ri], dev)
            return grid.indel_raw_floor_grid(lt, rt, threshold, lf, rf, prune=prune, metric=self.metric)

        general = lambda li, ri: wide.indel_any_grid([[l_ops[k_]] for k_ in li], [[r_ops[k_]] for k_ in ri], threshold, raw=True,
                                                     device=dev)
        return _best(lambda t: self.profile(left_items, right_items, t, device=dev, prune=prune),
                     split, len(l_ops), len(r_ops), margin,
                     threshold, mutual, fast, general)

    def assign(self, left_items: Sequence[Operand], right_items: Sequence[Operand], threshold: float, device=None,
               prune: bool = True) -> grid.Hits:
        """``grid.assign_of_hits(raw_grid(left_items, right_items, threshold))``: a one-to-one mapping between the two lists
        -- the best pair, both its items removed, and again (ties by left then right index) -- of the pairs scoring
        ``>= threshold``.  ``threshold`` is required: at 0 the hit list is the whole N x M grid.  The hits are ordered and
        assigned on the device and only the assignment (at most min(N, M) records) comes back; where wide items send part
        of the grid through the general kernels the merged host list goes through ``grid.assign_hits``."""
        from .. import wide

        grid.check_thresholds([threshold])
        l_ops, r_ops = [fuzzy_operand(v) for v in left_items], [fuzzy_operand(v) for v in right_items]
        split = self._split([[s] for s in l_ops], [[s] for s in r_ops])  # (before the device is asked for)
        dev = device or _device()
        if not l_ops or not r_ops:
            return wide.merge([])
        if split is not None:
            return grid.assign_hits(self.raw_grid(left_items, right_items, threshold, device=dev, prune=prune), len(l_ops),
                                    len(r_ops), device=dev)
        lt, rt = tables.encode_strings(l_ops, r_ops, dev)
        return grid.indel_raw_assign(lt, rt, threshold, prune=prune, metric=self.metric)

    def groups(self, left_items: Sequence[Operand], right_items: Sequence[Operand], threshold: float, device=None,
               prune: bool = True, same: bool = False, min_support=0) -> grid.MatchGroups:
        """``grid.groups_of_hits`` of ``raw_grid(left_items, right_items, threshold)``: the items of both lists grouped by
        the pairs scoring ``>= threshold``, closed transitively (left item k is node k, right item k node N + k; with
        ``same`` both lists are the same items in one node space).  The hits are linked on the device, unsorted, and only
        the labels come back; where wide items send part of the grid through the general kernels the merged host list goes
        through ``grid.group_hits``.  ``min_support > 0``: only the pairs of the ``(min_support + 2)``-truss link (every
        linking pair has that many common neighbours among the linking pairs; ``grid.group_hits`` has the definition), so
        chains fall apart -- for ``same=True``: two separate lists are a bipartite graph without common neighbours."""
        from .. import wide

        grid.check_thresholds([threshold])
        min_support = grid.check_min_support(min_support)
        l_ops, r_ops = [fuzzy_operand(v) for v in left_items], [fuzzy_operand(v) for v in right_items]
        split = self._split([[s] for s in l_ops], [[s] for s in r_ops])  # (before the device is asked for)
        dev = device or _device()
        n_l, n_r = len(l_ops), len(r_ops)
        layout = ((0,), (max(n_l, n_r),)) if same else ((0, n_l), (n_l, n_r))
        if not l_ops or not r_ops:
            return grid.MatchGroups(np.arange(sum(layout[1]), dtype=np.int32), *layout)
        if split is not None:
            hits = self.raw_grid(left_items, right_items, threshold, device=dev, prune=prune)
            return grid.MatchGroups(grid.group_hits([(hits, 0, layout[0][-1])], sum(layout[1]), float("-inf"), device=dev,
                                                    min_support=min_support), *layout)
        lt, rt = tables.encode_strings(l_ops, r_ops, dev)
        return grid.indel_raw_groups(lt, rt, threshold, prune=prune, same=same, metric=self.metric, min_support=min_support)

    def clusters(self, items: Sequence[Operand], threshold: float, device=None, prune: bool = True,
                 min_support=0) -> List[np.ndarray]:
        """Near-duplicate clusters inside ONE list (rapidfuzz users' dedupe): the self-join's groups of at least two items,
        each an ascending array of positions in ``items``, ordered by their smallest member.  ``min_support``: as for ``groups`` -- with 1 a chain of
        near-duplicates no longer swallows the list, every linking pair needs a third item close to both."""
        groups = self.groups(items, items, threshold, device=device, prune=prune, same=True, min_support=min_support)
        return [members[0] for members in groups.members(2)]

    def forest(self, left_items: Sequence[Operand], right_items: Sequence[Operand], threshold: float, device=None,
               prune: bool = True, same: bool = False) -> grid.MergeForest:
        """``grid.forest_of_hits`` of ``raw_grid(left_items, right_items, threshold)``: the merge forest of the pairs scoring
        ``>= threshold`` -- ``groups`` at every threshold from there up in one run (``cut(t)``), with the score that joined
        two items (``merge_score``) and the group statistics of a whole ladder (``ladder``).  Nodes as in ``groups``.  The
        hits are spanned on the device and only the forest comes back; where wide items send part of the grid through the
        general kernels the merged host list goes through ``grid.span_hits``."""
        from .. import wide

        grid.check_thresholds([threshold])
        l_ops, r_ops = [fuzzy_operand(v) for v in left_items], [fuzzy_operand(v) for v in right_items]
        split = self._split([[s] for s in l_ops], [[s] for s in r_ops])  # (before the device is asked for)
        dev = device or _device()
        n_l, n_r = len(l_ops), len(r_ops)
        layout = ((0,), (max(n_l, n_r),)) if same else ((0, n_l), (n_l, n_r))
        if not l_ops or not r_ops:
            return grid.forest_of_hits([], sum(layout[1]), float(threshold), *layout)
        if split is not None:
            hits = self.raw_grid(left_items, right_items, threshold, device=dev, prune=prune)
            return grid.span_hits([(hits, 0, layout[0][-1])], sum(layout[1]), float(threshold), device=dev, bases=layout[0],
                                  cohort_sizes=layout[1])
        lt, rt = tables.encode_strings(l_ops, r_ops, dev)
        return grid.indel_raw_forest(lt, rt, threshold, prune=prune, same=same, metric=self.metric)

    def cluster_tree(self, items: Sequence[Operand], threshold: float, device=None, prune: bool = True) -> grid.MergeForest:
        """The single-linkage tree of ONE list: the self-join's merge forest (node k is ``items[k]``); ``cut(t).members(2)``
        are ``clusters(items, t)`` for every ``t >= threshold``."""
        return self.forest(items, items, threshold, device=device, prune=prune, same=True)


class _IntersectionVsMean(_IntersectionVsUnion):
    """``2 * len(A & B) / (len(A) + len(B))``: the Sorensen-Dice coefficient.  ``ZeroDivisionError`` when both sets are
    empty."""
    __name__ = "intersection_vs_mean"
    measure = "mean"


class _IntersectionVsSmaller(_IntersectionVsUnion):
    """``len(A & B) / min(len(A), len(B))``: the overlap (Szymkiewicz-Simpson) coefficient -- 1.0 whenever one set holds the
    other.  ``ZeroDivisionError`` when either set is empty."""
    __name__ = "intersection_vs_smaller"
    measure = "smaller"


class _IntersectionVsLeft(_IntersectionVsUnion):
    """``len(A & B) / len(A)``: the containment of the LEFT set in the right one (asymmetric) -- a short definition against
    a long item that holds all its tokens scores 1.0.  ``ZeroDivisionError`` when the left set is empty."""
    __name__ = "intersection_vs_left"
    measure = "left"


class _LevenshteinMatch(_FuzzyMatch):
    """``1 - d(a, b) / max(la, lb)`` of the two prepared strings, d the unit-cost Levenshtein distance: the normalised
    Levenshtein similarity.  0.0 when either prepared string is empty, as ``fuzzy_match``."""
    __name__ = "levenshtein_match"
    metric = "edit"


class _LevenshteinWithin(_FuzzyMatch):
    """``1 - w(a, b) / la`` with w the least Levenshtein distance of the LEFT prepared string to any substring of the right
    one (asymmetric): a short definition that occurs verbatim in a long item scores 1.0 -- the string counterpart of
    ``intersection_vs_left``.  0.0 when either prepared string is empty."""
    __name__ = "levenshtein_within"
    metric = "edit_within"


intersection_vs_union = _IntersectionVsUnion()
intersection_vs_mean = _IntersectionVsMean()
intersection_vs_smaller = _IntersectionVsSmaller()
intersection_vs_left = _IntersectionVsLeft()
fuzzy_match = _FuzzyMatch()
levenshtein_match = _LevenshteinMatch()
levenshtein_within = _LevenshteinWithin()
PLUGINS = (intersection_vs_union, intersection_vs_mean, intersection_vs_smaller, intersection_vs_left, fuzzy_match,
           levenshtein_match, levenshtein_within)
