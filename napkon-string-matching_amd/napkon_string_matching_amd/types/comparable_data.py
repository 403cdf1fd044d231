"""``ComparableData``: the cross-cohort N x M match loop with the reference's surface.

Mirrors ``napkon_string_matching/types/comparable_data.py`` (:69-299, :452-574): same method names,
keyword arguments, output columns, thresholds (``>=`` on doubles), exceptions and pair labels
(``i*M + j`` after dropna / whitelist removal).  What differs is WHERE the work runs:

* per ITEM (host, O(N + M)): dropna, whitelist removal, ``gen_comp_value`` levels, token -> id /
  string encoding, category bit masks;
* per PAIR (MI355X, one launch): the ``compare_terms`` sum over levels with the chosen score
  function, the category predicate and the threshold (csrc/jaccard_levels_impl.hpp,
  csrc/indel_levels.hip).  The reference's N*M-row ``merge(how="cross")`` frame (:191) is never built;
* per HIT (host): the blacklist -- dropping a blacklisted pair before scoring (:195-204) equals
  dropping it from the hit list -- and the output frame.

The reference's per-pair exceptions only depend on per-item properties (a zero-level item ->
``IndexError`` at :262, two empty level sets -> ``ZeroDivisionError`` at score_functions.py:13), so
they are resolved on the host, in pair order, against the same blacklist / category filters.
"""
from __future__ import annotations

import itertools
import json
import logging
from contextlib import contextmanager
from hashlib import md5
from pathlib import Path
from types import SimpleNamespace
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from .. import _lib, distributed, grid, tables
from ..compare import score_functions
from .comparable import COLUMN_NAMES, IDENTIFIER, MATCH_SCORE, QUESTION_OUTPUT, Comparable
from .mapping import Mapping

logger = logging.getLogger(__name__)

PREPARE_REMOVE_SYMBOLS = "!?,.()[]:;*"  # comparable_data.py:24
CACHE_FILE_PATTERN = "compared__score_{}.json"  # comparable_data.py:25
COMP_COLUMN = "Compare"
TERM = "Term"
_INF = 1 << 30


# =============================================================================== per item
def flatten_list(list_) -> List[str]:
    """One level of flattening (:567-574); a ``str`` is walked character by character."""
    out: List[str] = []
    for part in list_:
        if isinstance(part, list):
            out += part
        else:
            out.append(part)
    return out


class Tokenizer:
    """The word tokenizer + stop-word list of ``tokenize`` (:287-299).

    Upstream uses nltk punkt and nltk's German stop words; neither ships with this package (no
    network at build time), so both are injectable.  The default (``str.split``, no stop words)
    equals punkt on text made of plain alphanumeric words that are not stop words.
    """

    def __init__(self, word_tokenize: Callable[[str], Iterable[str]] = str.split, stop_words: Iterable[str] = ()):
        self.word_tokenize = word_tokenize
        self.stop_words = frozenset(stop_words)

    @classmethod
    def from_nltk(cls, language: str = "german") -> "Tokenizer":
        from nltk.corpus import stopwords  # optional dependency
        from nltk.tokenize import word_tokenize

        return cls(word_tokenize, stopwords.words(language))

    def __call__(self, parts) -> List[str]:
        words = self.word_tokenize(" ".join(flatten_list(parts)))
        kept = {w for w in words if w.casefold() not in self.stop_words and w not in PREPARE_REMOVE_SYMBOLS}
        return sorted(kept, key=str.casefold)

    @property
    def compositional(self) -> bool:
        """True when tokenising a blank-joined sequence equals concatenating the parts' tokens
        (whitespace splitting): the suffix levels can then be built incrementally."""
        return self.word_tokenize is str.split

    def levels(self, items) -> List[List[str]]:
        """``[tokenize(items[-k:]) for k in 1..len(items)]`` (gen_comp_value, :283-285).  For a
        compositional tokenizer each entry is tokenised once and the suffix sets grow by union --
        the same lists, without the O(L^2) re-tokenisation."""
        if not self.compositional or isinstance(items, str):
            return [self(items[-k:]) for k in range(1, len(items) + 1)]
        out: List[List[str]] = []
        acc: set = set()
        stop = self.stop_words
        for entry in reversed(items):
            parts = entry if isinstance(entry, list) else [entry]
            for part in parts:
                for w in part.split():
                    if w not in PREPARE_REMOVE_SYMBOLS and (not stop or w.casefold() not in stop):
                        acc.add(w)
            out.append(sorted(acc, key=str.casefold))
        return out


# =============================================================================== mappings
def get_identifiers_from_mapping(mappings: Mapping, group: str) -> List[str]:
    out: List[str] = []
    for entry in mappings.values():
        out += entry[group]
    return out


def flatten_mapping(left_group: str, right_group: str, mapping: Mapping) -> List[Tuple[str, str]]:
    """Cartesian identifier pairs of every entry that lists both cohorts (:555-564)."""
    return [(a, b) for lefts, rights in mapping.get_all_mapping_for_groups(left_group, right_group)
            for a in lefts for b in rights]


def _as_mapping(value) -> Mapping:
    if value is None:
        return Mapping()
    if isinstance(value, Mapping):
        return value
    if isinstance(value, dict):
        return Mapping(value)
    if hasattr(value, "dict"):
        return Mapping(value.dict())
    raise TypeError("mappings must be a Mapping or a {uuid: {cohort: [identifiers]}} dict")


# =============================================================================== categories
class _Categories:
    """Category columns of both sides as <= 64-bit masks + the device predicate mode."""

    def __init__(self, left: Sequence, right: Sequence, first_left, first_right) -> None:
        l_list, r_list = isinstance(first_left, list), isinstance(first_right, list)
        if l_list and not r_list:
            # :471 evaluates `x in set(y)` with x a list: hashing a list raises
            raise TypeError("unhashable type: 'list'")
        self.mode = _lib.CAT_INTERSECT_OR_BOTH_EMPTY if (l_list and r_list) else _lib.CAT_INTERSECT
        self.scalar_scalar = not l_list and not r_list
        # inside item_memo() the label -> bit assignment is shared by the run's grids, which makes the
        # per-cell result reusable (a cohort's cells are looked at once per grid it takes part in)
        memo = ComparableData._item_memo
        bits: Dict[object, int] = {} if memo is None else memo.setdefault(("category bits",), {})

        def mask_of(value, as_list: bool) -> Tuple[int, frozenset]:
            if memo is None:
                return mask(value, as_list)
            key = ("category", as_list, id(value))
            got = memo.get(key)
            if got is None or got[0] is not value:
                got = (value, mask(value, as_list))
                memo[key] = got
            return got[1]

        def mask(value, as_list: bool) -> Tuple[int, frozenset]:
            labels = value if as_list else [value]
            if as_list and not isinstance(value, list):
                raise NotImplementedError("Category column mixes lists and scalars")
            if not as_list and isinstance(value, list):
                raise NotImplementedError("Category column mixes lists and scalars")
            m = 0
            keys = []
            for lab in labels:
                if isinstance(lab, float) and lab != lab:
                    continue  # NaN never equals anything
                keys.append(lab)
                m |= 1 << bits.setdefault(lab, len(bits))
            return m, frozenset(keys)

        lm = [mask_of(v, l_list) for v in left]
        rm = [mask_of(v, r_list) for v in right]
        self.left_sets = [s for _, s in lm]
        self.right_sets = [s for _, s in rm]
        self.on_device = len(bits) <= 64
        if self.on_device:
            self.left_mask = np.array([m for m, _ in lm], dtype=np.uint64)
            self.right_mask = np.array([m for m, _ in rm], dtype=np.uint64)

    def match(self, i: int, j: int) -> bool:
        a, b = self.left_sets[i], self.right_sets[j]
        if a & b:
            return True
        return self.mode == _lib.CAT_INTERSECT_OR_BOTH_EMPTY and not a and not b


# =============================================================================== the class
def _agree_on_rank0(flag: bool) -> bool:
    """Rank 0's verdict on every rank (one tiny broadcast; a no-op without a process group)."""
    rank, size = distributed.world()
    if size == 1:
        return bool(flag)
    return bool(distributed.broadcast_object(bool(flag) if rank == 0 else None))


def _read_cache_collectively(cache_file: Path) -> Comparable:
    """The cached ``Comparable``: read by rank 0 and handed to the other ranks (their ``cache_dir`` need not
    be the same file system)."""
    rank, size = distributed.world()
    if size == 1:
        return Comparable.read_json(cache_file)
    # rank 0 may fail (unreadable or corrupt file): it must still take part in the broadcast, or the other ranks wait
    # for it forever -- the failure travels as the payload and every rank raises it (round-3 advice)
    box = None
    if rank == 0:
        try:
            text = cache_file.read_text(encoding="utf-8")
            json.loads(text)
            box = (True, text)
        except Exception as exc:  # noqa: BLE001 -- re-raised on every rank below
            box = (False, f"{type(exc).__name__}: {exc}")
    ok, payload = distributed.broadcast_object(box)
    if not ok:
        raise RuntimeError(f"compare cache {cache_file} could not be read on rank 0: {payload}")
    return Comparable(data=json.loads(payload))


class ComparableData:
    """A cohort's items as a pandas frame plus the ``compare`` machinery.

    Needs the columns ``Identifier``, ``Term`` and the compare column; ``Variable``, ``Sheet`` are
    copied to the result when present; ``Category`` when ``filter_categories`` is on.
    """

    __column_mapping__: Dict[str, str] = {}
    __category_column__ = "Category"
    tokenizer: Tokenizer = Tokenizer()
    _item_memo: Optional[Dict[int, tuple]] = None  # see item_memo()

    @classmethod
    @contextmanager
    def item_memo(cls):
        """Per-ITEM results (levels, fuzzy operands) are remembered by the identity of the cell object
        while the context is open: with k cohorts every item takes part in k - 1 grids
        (Matcher.match_questionnaires), and dropna / rename hand the same cell objects on.  The cells
        must not be modified in place inside the context."""
        outer = ComparableData._item_memo
        ComparableData._item_memo = {} if outer is None else outer
        try:
            yield
        finally:
            ComparableData._item_memo = outer

    @staticmethod
    def _memoised(tag, values, func) -> list:
        memo = ComparableData._item_memo
        if memo is None:
            return [func(v) for v in values]
        out = []
        for v in values:
            key = (tag, id(v))
            got = memo.get(key)
            if got is None or got[0] is not v:  # the memo keeps `v` alive, so its id cannot be reused
                got = (v, func(v))
                memo[key] = got
            out.append(got[1])
        return out

    def __init__(self, data=None) -> None:
        if isinstance(data, ComparableData):
            data = data._data
        self.__dict__["_data"] = data if isinstance(data, pd.DataFrame) else pd.DataFrame(data)

    # ---- thin frame wrapper (reference: types/data.py)
    def __getattr__(self, name: str):
        return getattr(self._data, name)

    def __getitem__(self, item):
        got = self._data[item]
        return self.__class__(got) if isinstance(got, pd.DataFrame) else got

    def __setitem__(self, item, value) -> None:
        self._data[item] = value

    def __len__(self) -> int:
        return len(self._data)

    def __repr__(self) -> str:
        return repr(self._data)

    def dataframe(self) -> pd.DataFrame:
        return self._data

    def dropna(self, *args, **kwargs) -> "ComparableData":
        return self.__class__(self._data.dropna(*args, **kwargs))

    def to_csv(self) -> str:
        return self._data.to_csv(index=False)

    def map_for_comparable(self) -> pd.DataFrame:
        return self._data.rename(columns=self.__column_mapping__)

    # ---- per item
    @classmethod
    def tokenize(cls, parts, language: str = "german") -> List[str]:
        return cls.tokenizer(parts)

    @classmethod
    def gen_comp_value(cls, items) -> List[List[str]]:
        """Level l = tokens of the last l+1 entries (:283-285)."""
        return cls.tokenizer.levels(items)

    @staticmethod
    def gen_term(*items: str) -> List[str]:
        return [item for item in items if item]

    def get_existing_mapping_ids(self, group_name: str, mappings: Mapping) -> List[str]:
        per_group = mappings.filter_by_group(group_name)
        identifiers = list(self._data[IDENTIFIER])
        return list({key for key, members in per_group.items() for ident in identifiers if ident in members})

    def remove_existing_mappings(self, existing_mappings) -> None:
        drop = set(existing_mappings)
        self.__dict__["_data"] = self._data[[v not in drop for v in self._data[IDENTIFIER]]]

    # ---- per pair (single): compare_terms as a 1 x 1 levels grid on the GPU
    @classmethod
    def compare_terms(cls, left: Sequence, right: Sequence, score_func) -> float:
        """:248-265 for ONE pair.  ``score_func`` is one of this package's plugins (or its name)."""
        plugin = _resolve_plugin(score_func)
        if len(left) == 0 and len(right) == 0:
            return 0
        if len(left) == 0 or len(right) == 0:
            raise IndexError("list index out of range")
        if plugin.kind == "sets":
            sets = lambda levels: [list(score_functions.set_operand(lv)) for lv in levels]
            sl, sr = sets(left), sets(right)
            if _divides_by_zero(sl, _empty_levels(sl), sr, _empty_levels(sr), plugin.divides_by_zero):
                raise ZeroDivisionError("division by zero")  # a step the plugin divides by zero at is visited
        hits = _levels_grid(plugin, [list(left)], [list(right)], float("-inf"), None, None)
        return float(hits.score[0])

    # ---- the grid
    def compare(
        self,
        other,
        existing_mappings_whitelist=None,
        existing_mappings_blacklist=None,
        compare_column: str = None,
        score_threshold: float = 0.1,
        cached: bool = True,
        cache_threshold: Optional[float] = None,
        cache_dir=None,
        identifier_column_left: Optional[str] = None,
        identifier_column_right: Optional[str] = None,
        *args,
        top_k: Optional[int] = None,
        best_margin: Optional[float] = None,
        mutual_best: bool = False,
        one_to_one: bool = False,
        **kwargs,
    ) -> Comparable:
        """:69-128.  Scores at ``cache_threshold or score_threshold``, keeps ``>= score_threshold``,
        orders by score descending.

        ``top_k``: keep only the first ``top_k`` pairs of every left item in the order (score descending, right item
        ascending) -- the frame ``compare()`` returns without it, restricted to those pair labels (rapidfuzz's
        ``process.extract(limit=)`` over ``compare_terms``).  Each item's pairs are cut in score order, so cutting at
        ``cache_threshold`` and then filtering at ``score_threshold`` keeps the meaning of both.

        ``best_margin`` (a finite number >= 0): keep only the pairs within ``best_margin`` of their left item's best score --
        the frame ``compare()`` returns without it (after ``dropna``, whitelist removal, blacklist and categories; zero-level
        pairs, which score 0, count as rows like any other), restricted to ``score >= best[left item] - best_margin``.  0.0
        is every item's best match with all its ties, which no ``top_k`` returns.  ``mutual_best=True``: a pair must also be
        within ``best_margin`` of its RIGHT item's best (reciprocal best hits).  The bests are taken at ``cache_threshold``
        and the rows filtered at ``score_threshold`` afterwards, which keeps the meaning: an item whose best is below
        ``score_threshold`` has no rows either way, and one whose best is above it has the same best at both thresholds.
        Restrictions as for ``top_k`` (at most 64 category labels; one rank); not together with ``top_k``.

        ``one_to_one=True``: a mapping instead of a match list -- of the frame ``compare()`` returns without it (after
        ``dropna``, whitelist removal, blacklist and categories, zero-level pairs included) the rows that
        ``grid.assign_of_hits`` takes: the best pair, both its items removed, and again; equal scores in the order (left
        position, right position).  Every item appears in at most one row, and no row of the plain frame has both its
        items unused.  Assigned at ``cache_threshold`` and filtered at ``score_threshold`` afterwards, which keeps the
        meaning: rows below a threshold are walked after all rows at or above it.  Not together with ``top_k`` or
        ``best_margin``; one rank.

        Compare cache: the reference keys ``compared__score_{md5}.json`` by a hash
        that embeds object addresses (``str(kwargs.items())`` of ``Mapping`` objects, :61-67), so it
        never hits, and it leaves ``score_func`` out of the key.  Here the key is a stable content
        hash (both frames, both mappings, compare column, cache threshold, score function, category
        filter, cohort names) and the cache is only used when ``cache_dir`` is given.  The file format
        is the reference's: ``{"left_name", "right_name", "data": [records]}`` (indent 4); like
        upstream, a frame read back from the cache carries a fresh RangeIndex instead of pair labels.
        """
        if top_k is not None:
            top_k = grid.check_k(top_k)
        best_margin = _check_best_args(best_margin, mutual_best, top_k)
        one_to_one = _check_one_to_one(one_to_one, top_k, best_margin)
        first = cache_threshold if cache_threshold else score_threshold
        cache_file = None
        if cached and cache_dir is not None:
            cache_file = Path(cache_dir) / CACHE_FILE_PATTERN.format(
                self._hash_compare_args(other, existing_mappings_whitelist, existing_mappings_blacklist,
                                        compare_column, first, kwargs, top_k, best_margin, mutual_best, one_to_one))
        # hit or miss is decided ONCE for all ranks of a sharded run (rank 0 looks, everybody follows): with a
        # rank-local exists() the ranks can disagree -- a cache_dir that is not shared between nodes, or a repeated
        # compare() where one rank looks before rank 0's rename has landed -- and the ranks that miss would then
        # wait in gen_comparable's collectives for a rank that never comes
        use_cache = cache_file is not None and _agree_on_rank0(cache_file.exists())
        if use_cache:
            logger.info("using cached result")
            result = _read_cache_collectively(cache_file)
        else:
            if cache_file is None:
                # the rows between `first` and `score_threshold` only ever fed the cache file: without
                # it, scoring at `first` and filtering at `score_threshold` equals scoring at the max
                first = max(first, score_threshold)
            result = self.gen_comparable(
                other,
                existing_mappings_whitelist,
                existing_mappings_blacklist,
                *args,
                score_threshold=first,
                compare_column=compare_column,
                identifier_column_left=identifier_column_left,
                identifier_column_right=identifier_column_right,
                top_k=top_k,
                best_margin=best_margin,
                mutual_best=mutual_best,
                one_to_one=one_to_one,
                **kwargs,
            )
            if cache_file is not None:
                # every rank of a sharded run holds the full result: rank 0 writes it (atomically, see write_json); its
                # verdict is broadcast, which also is the barrier: nobody returns (and calls compare again) before the
                # file is in place, and a failed write (disk full) raises on every rank instead of leaving them waiting
                error = None
                if distributed.world()[0] == 0:
                    try:
                        cache_file.parent.mkdir(parents=True, exist_ok=True)
                        logger.info("write cache to file")
                        result.write_json(cache_file)
                    except Exception as exc:  # noqa: BLE001 -- re-raised on every rank below
                        error = f"{type(exc).__name__}: {exc}"
                if distributed.world()[1] > 1:
                    error = distributed.broadcast_object(error)
                if error is not None:
                    raise RuntimeError(f"compare cache {cache_file} could not be written on rank 0: {error}")
        result = result[result.match_score >= score_threshold]
        logger.info("got %i filtered entries", len(result))
        result.sort_by_score()
        return result

    def compare_profile(self, other, thresholds, existing_mappings_whitelist=None, existing_mappings_blacklist=None,
                        compare_column: str = None, identifier_column_left: Optional[str] = None,
                        identifier_column_right: Optional[str] = None, **kwargs) -> grid.ThresholdProfile:
        """What ``compare(other, score_threshold=t, ...)`` would return for every ``t`` of ``thresholds`` (1 .. 64, strictly
        ascending), without the pairs: ``pairs[k] == len(compare(score_threshold=thresholds[k]))`` (no cache involved), and
        per item -- by position in the compared frames, i.e. after ``dropna`` on the compare column and the whitelist --
        its best score among the pairs at ``thresholds[0]`` (``-1.0``: none).  Takes the keyword arguments of ``compare``
        (``score_func``, ``left_name``, ``filter_categories``, ...; thresholds and cache arguments are ignored) and runs the
        same prelude: whitelist, blacklist, categories, the reference's exceptions in pair order, zero-level pairs scoring
        0.  Categories and blacklist run in the kernel (``nsm_*_levels_profile``), so more than 64 category labels are a
        ``NotImplementedError``, as for ``top_k``; so is a sharded run."""
        t = grid.check_thresholds(thresholds)
        if distributed.world()[1] > 1:
            raise NotImplementedError("compare_profile on more than one rank (sharded profiles are not implemented)")
        for name in ("score_threshold", "cached", "cache_threshold", "cache_dir", "top_k", "best_margin", "mutual_best",
                     "one_to_one"):
            kwargs.pop(name, None)
        pre = self._compare_prelude(
            other, existing_mappings_whitelist, existing_mappings_blacklist, kwargs.get("score_func"), compare_column,
            kwargs.get("category_column", "Category"), kwargs.get("left_name"), kwargs.get("right_name"),
            kwargs.get("filter_categories", False), identifier_column_left, identifier_column_right, per_item="a threshold profile")
        return _prelude_profile(pre, t)

    def score_pairs(self, other, pairs, compare_column: str = None, score_func: str = None,
                    identifier_column_left: Optional[str] = None, identifier_column_right: Optional[str] = None,
                    left_name: str = None, right_name: str = None, **kwargs) -> Comparable:
        """What do THESE pairs score?  ``pairs``: a sequence of (left identifier, right identifier), or a ``Mapping`` (a
        validated mapping, a whitelist, a blacklist), read with ``flatten_mapping(left_name, right_name, mapping)``.
        Returns a ``Comparable`` with ``compare``'s columns and one row per listed pair, in list order (a plain
        ``RangeIndex``); ``MatchScore`` is ``compare_terms`` of the two items, NaN where an identifier is not in the compared
        frame (the frame after ``dropna`` on the compare column; of several rows with one identifier the first counts).

        Takes ``compare``'s keyword arguments and runs its per-item prelude (dropna, the level builder).  No whitelist
        removal, blacklist, category filter or threshold is applied -- those arguments are ignored: the whitelist's own
        pairs are what a user scores here.  Two level-less items score 0 as in ``compare_terms``; the FIRST listed pair for
        which ``compare_terms`` would raise raises here too (``IndexError``: level-less against levels,
        ``ZeroDivisionError``: an empty-vs-empty level), before any device work.  One launch of ``nsm_*_levels_pairs`` for
        the whole list, O(P); pairs with a wide or irregular item go through the general grids, one call per distinct left
        item of such pairs (slow, rare).  On a sharded run every rank scores the whole list itself: no collective."""
        if isinstance(pairs, (Mapping, dict)) or (hasattr(pairs, "dict") and not isinstance(pairs, (list, tuple))):
            if not left_name or not right_name:
                raise ValueError("score_pairs: a Mapping needs left_name and right_name (the cohorts whose identifiers it lists)")
            pairs = flatten_mapping(left_name, right_name, _as_mapping(pairs))
        if isinstance(pairs, (str, bytes)):
            raise ValueError("score_pairs: pairs must be a sequence of (left identifier, right identifier)")
        pairs = list(pairs)
        for pair in pairs:
            if isinstance(pair, (str, bytes)) or not hasattr(pair, "__len__") or len(pair) != 2:
                raise ValueError(f"score_pairs: {pair!r} is not a (left identifier, right identifier) pair")
        pre = self._compare_prelude(other, None, None, score_func, compare_column, kwargs.get("category_column", "Category"),
                                    left_name or "left", right_name or "right", False, identifier_column_left,
                                    identifier_column_right, listed=True)
        first_row = lambda ids: {v: k for k, v in reversed(list(enumerate(ids)))}
        pos_l, pos_r = first_row(pre.id_l), first_row(pre.id_r)
        pi = np.array([pos_l.get(a, -1) for a, _ in pairs], dtype=np.int64)
        pj = np.array([pos_r.get(b, -1) for _, b in pairs], dtype=np.int64)
        known = (pi >= 0) & (pj >= 0)
        score = np.full(len(pairs), np.nan, dtype=np.float64)
        # ---- the reference's per-pair exceptions, in list order; level-less pairs score 0
        is_sets = pre.plugin.kind == "sets"
        empty = {}
        if is_sets:
            reach = lambda levels: _empty_levels([lv if isinstance(lv, list) else lv.split() for lv in levels])
            empty = {("l", k): reach(pre.levels_l[k]) for k in set(pi[known].tolist())}
            empty.update({("r", k): reach(pre.levels_r[k]) for k in set(pj[known].tolist())})
        todo = []
        for p in np.flatnonzero(known):
            a, b = pre.levels_l[pi[p]], pre.levels_r[pj[p]]
            if len(a) == 0 and len(b) == 0:
                score[p] = 0.0
            elif len(a) == 0 or len(b) == 0:
                raise IndexError("list index out of range")
            elif is_sets and (empty[("l", int(pi[p]))] or empty[("r", int(pj[p]))]) and \
                    _divides_by_zero(a, empty[("l", int(pi[p]))], b, empty[("r", int(pj[p]))], pre.plugin.divides_by_zero):
                raise ZeroDivisionError("division by zero")
            else:
                todo.append(p)
        if todo:
            todo = np.array(todo, dtype=np.int64)
            score[todo] = _levels_pairs(pre.plugin, pre.levels_l, pre.levels_r, pi[todo], pj[todo])
        # ---- output frame: compare's columns, one row per listed pair
        lf = pre.lf.assign(**{COMP_COLUMN: pre.levels_l, QUESTION_OUTPUT: pre.argument_l})
        rf = pre.rf.assign(**{COMP_COLUMN: pre.levels_r, QUESTION_OUTPUT: pre.argument_r})
        out = {}
        sides = ((lf, pre.lp, pi, identifier_column_left or IDENTIFIER, [a for a, _ in pairs]),
                 (rf, pre.rp, pj, identifier_column_right or IDENTIFIER, [b for _, b in pairs]))
        for frame, prefix, rows, id_col, given in sides:
            for col in frame.columns:
                if col in COLUMN_NAMES:
                    cells = np.empty(len(rows), dtype=object)
                    values = frame[col].to_numpy()
                    for k, r in enumerate(rows):
                        cells[k] = values[r] if r >= 0 else (given[k] if col == id_col else None)
                    out[prefix + col] = cells
        out[MATCH_SCORE] = score
        return Comparable(data=pd.DataFrame(out), left_name=pre.lp, right_name=pre.rp)

    def _hash_compare_args(self, other, whitelist, blacklist, compare_column, cache_threshold, kwargs, top_k=None,
                           best_margin=None, mutual_best=False, one_to_one=False) -> str:
        other_csv = other.to_csv() if hasattr(other, "to_csv") else pd.DataFrame(other).to_csv(index=False)
        parts = [
            self.to_csv(), other_csv,
            json.dumps(_as_mapping(whitelist).dict(), sort_keys=True),
            json.dumps(_as_mapping(blacklist).dict(), sort_keys=True),
            str(compare_column), repr(cache_threshold),
            json.dumps({k: kwargs.get(k) for k in ("score_func", "filter_categories", "category_column", "left_name",
                                                    "right_name")}, sort_keys=True, default=str),
        ]
        if top_k is not None:  # (absent from the key otherwise: the keys of plain calls stay what they were)
            parts.append(f"top_k={int(top_k)}")
        if best_margin is not None:
            parts.append(f"best_margin={float(best_margin)!r}")
            if mutual_best:
                parts.append("mutual_best=True")
        if one_to_one:
            parts.append("one_to_one=True")
        return md5("\x1f".join(parts).encode("utf-8"), usedforsecurity=False).hexdigest()

    def _compare_prelude(self, right, existing_mappings_whitelist, existing_mappings_blacklist, score_func, compare_column,
                         category_column, left_name, right_name, filter_categories, identifier_column_left,
                         identifier_column_right, per_item: Optional[str] = None, listed: bool = False) -> SimpleNamespace:
        """Everything of :133-222 that comes before the scores, shared by ``gen_comparable`` and ``compare_profile``:
        whitelist, levels, blacklist as position pairs, categories, the reference's per-pair exceptions in pair order, the
        zero-level pairs that score 0, and the items the device grid takes.  ``per_item``: the name of a query whose
        category predicate must run on the device (``NotImplementedError`` beyond 64 labels).  ``listed``
        (``score_pairs``): the per-item part only -- dropna, levels, identifiers; the caller names its pairs itself, so no
        whitelist removal, blacklist, category filter or scan of the whole grid for the reference's exceptions."""
        plugin = getattr(score_functions, score_func)  # AttributeError for an unknown name (:150)
        whitelist = _as_mapping(existing_mappings_whitelist)
        blacklist = _as_mapping(existing_mappings_blacklist)
        if not isinstance(right, ComparableData):
            right = ComparableData(right)

        left = self.dropna(subset=[compare_column])
        right = right.dropna(subset=[compare_column])
        logger.info(
            "comparing number of items %i left, %i right, potential %s comparisons",
            len(left), len(right), "{:,}".format(len(left) * len(right)),
        )
        if not listed:
            remove_existing_mappings(left, right, left_name, right_name, whitelist)
            logger.info("after removing existing whitelisted mappings: %i left, %i right", len(left), len(right))

        lf, rf = left.map_for_comparable(), right.map_for_comparable()
        lp, rp = left_name.title(), right_name.title()
        n_l, n_r = len(lf), len(rf)

        levels_l = self._memoised(("levels", id(self.tokenizer)), lf[compare_column], self.gen_comp_value)
        levels_r = self._memoised(("levels", id(self.tokenizer)), rf[compare_column], self.gen_comp_value)
        argument_l = [":".join(flatten_list(item)) for item in lf[TERM]]
        argument_r = [":".join(flatten_list(item)) for item in rf[TERM]]

        # ---- blacklist as position pairs
        id_l = list(lf[identifier_column_left or IDENTIFIER])
        id_r = list(rf[identifier_column_right or IDENTIFIER])
        if listed:
            return SimpleNamespace(plugin=plugin, lf=lf, rf=rf, lp=lp, rp=rp, n_l=n_l, n_r=n_r, levels_l=levels_l,
                                   levels_r=levels_r, argument_l=argument_l, argument_r=argument_r, id_l=id_l, id_r=id_r)
        banned = _banned_positions(flatten_mapping(left_name, right_name, blacklist), id_l, id_r)
        logger.info("remaining %s entries after removing blacklisted ones", "{:,}".format(n_l * n_r - len(banned)))

        # ---- categories
        cats: Optional[_Categories] = None
        if filter_categories:
            first = _first_surviving_pair(n_l, n_r, banned)
            if first is None:
                raise IndexError("single positional indexer is out-of-bounds")  # df.iloc[0] at :465
            cl, cr = list(lf[category_column]), list(rf[category_column])
            cats = _Categories(cl, cr, cl[first[0]], cr[first[1]])
            if per_item is None and (getattr(plugin, "measure", "union") != "union" or getattr(plugin, "metric", "indel") != "indel"):
                per_item = f"score_func {score_func}"  # (its grid is a per-item sweep: floors_levels.hip without floors)
            if per_item is not None and not cats.on_device:
                raise NotImplementedError(f"{per_item} with more than 64 distinct category labels (the predicate must run on "
                                          "the device, where each item keeps its list)")
        elif n_l == 0 or n_r == 0:
            # the reference's blacklist step indexes the cross join with a list of booleans (:549-552); for
            # an EMPTY cross join that list is empty, pandas reads it as "no columns", and :223-232 then
            # fails on the compare column
            raise KeyError(lp + COMP_COLUMN)

        def survives(i: int, j: int) -> bool:
            return (i, j) not in banned and (cats is None or cats.match(i, j))

        # ---- the reference's per-pair exceptions, in pair order
        nlev_l = np.array([len(v) for v in levels_l], dtype=np.int64)
        nlev_r = np.array([len(v) for v in levels_r], dtype=np.int64)
        extra_hits: List[Tuple[int, int]] = []  # zero-level x zero-level pairs score 0
        _raise_first_pair_error(
            plugin.kind == "sets", levels_l, levels_r, nlev_l, nlev_r, n_r, survives, extra_hits,
            getattr(plugin, "divides_by_zero", None)
        )

        # ---- device grid over the items that have at least one level
        keep_l = np.flatnonzero(nlev_l > 0)
        keep_r = np.flatnonzero(nlev_r > 0)
        return SimpleNamespace(plugin=plugin, lf=lf, rf=rf, lp=lp, rp=rp, n_l=n_l, n_r=n_r, levels_l=levels_l, levels_r=levels_r,
                               argument_l=argument_l, argument_r=argument_r, banned=banned, cats=cats, nlev_l=nlev_l,
                               nlev_r=nlev_r, extra_hits=extra_hits, keep_l=keep_l, keep_r=keep_r)

    def gen_comparable(
        self,
        right,
        existing_mappings_whitelist=None,
        existing_mappings_blacklist=None,
        score_func: str = None,
        compare_column: str = None,
        category_column: str = "Category",
        score_threshold: float = 0.1,
        left_name: str = None,
        right_name: str = None,
        filter_categories: bool = False,
        identifier_column_left: Optional[str] = None,
        identifier_column_right: Optional[str] = None,
        *args,
        top_k: Optional[int] = None,
        best_margin: Optional[float] = None,
        mutual_best: bool = False,
        one_to_one: bool = False,
        **kwargs,
    ) -> Comparable:
        """:133-246 (steps 1-12 of SURVEY.md 3.2), the per-pair part on the GPU.  ``top_k``: per left item only the
        first ``top_k`` pairs (score descending, right item ascending) of what would be returned (``compare``).
        ``best_margin`` / ``mutual_best``: only the pairs within ``best_margin`` of their left (and right) item's best score
        among what would be returned (``compare``): a profile sweep for the bests, then a floor grid.
        ``one_to_one``: ``grid.assign_of_hits`` of what would be returned, by position in the compared frames
        (``grid.assign_hits`` on the final host arrays: after the blacklist, the host-side category filter and the
        zero-level pairs)."""
        if top_k is not None:
            top_k = grid.check_k(top_k)
        best_margin = _check_best_args(best_margin, mutual_best, top_k)
        one_to_one = _check_one_to_one(one_to_one, top_k, best_margin)
        if one_to_one and distributed.world()[1] > 1:
            raise NotImplementedError("one_to_one on more than one rank (sharded assignment is not implemented)")
        if best_margin is not None and distributed.world()[1] > 1:
            raise NotImplementedError("best_margin on more than one rank (sharded best matches are not implemented)")
        pre = self._compare_prelude(right, existing_mappings_whitelist, existing_mappings_blacklist, score_func, compare_column,
                                    category_column, left_name, right_name, filter_categories, identifier_column_left,
                                    identifier_column_right,
                                    per_item="top_k" if top_k is not None else "best_margin" if best_margin is not None else None)
        plugin, lf, rf, lp, rp, n_l, n_r = pre.plugin, pre.lf, pre.rf, pre.lp, pre.rp, pre.n_l, pre.n_r
        levels_l, levels_r, argument_l, argument_r = pre.levels_l, pre.levels_r, pre.argument_l, pre.argument_r
        banned, cats, nlev_l, nlev_r, extra_hits, keep_l, keep_r = (pre.banned, pre.cats, pre.nlev_l, pre.nlev_r, pre.extra_hits,
                                                                     pre.keep_l, pre.keep_r)
        rank, world_size = distributed.world()
        if world_size > 1:  # left rows block-sharded over the ranks, right side replicated
            row_lo, row_hi = distributed.shard_bounds(n_l, rank, world_size)
            keep_l = keep_l[(keep_l >= row_lo) & (keep_l < row_hi)]
            extra_hits = [p for p in extra_hits if row_lo <= p[0] < row_hi]
        if top_k is not None and min(top_k, int(keep_r.size)) > grid.TOP_K_MAX:
            raise NotImplementedError(f"top_k = {min(top_k, int(keep_r.size))} (after clamping to the right side's "
                                      f"{int(keep_r.size)} items) exceeds the supported {grid.TOP_K_MAX}")
        logger.info("calculate score")
        host_filter = bool(banned) or (cats is not None and not cats.on_device)
        pending = None
        floors = None
        if best_margin is not None:
            # pass 1: every item's best score over the frame a plain call returns (zero-level pairs included); pass 2 below
            # emits what reaches floor = best - margin.  Categories and blacklist run in the kernel in both passes
            floors = grid.floors_of_profile(_prelude_profile(pre, grid.check_thresholds([score_threshold])), best_margin,
                                            mutual_best)
        if keep_l.size and keep_r.size and floors is not None:
            on_device = cats is not None
            hits = _levels_grid(
                plugin,
                [levels_l[k] for k in keep_l],
                [levels_r[k] for k in keep_r],
                score_threshold,
                cats.left_mask[keep_l] if on_device else None,
                cats.right_mask[keep_r] if on_device else None,
                cats.mode if on_device else _lib.CAT_NONE,
                banned=_local_banned(banned, keep_l, keep_r),
                floors=(floors[0][keep_l], None if floors[1] is None else floors[1][keep_r]),
            )
        elif keep_l.size and keep_r.size and top_k is not None:
            # per-item lists on the device: categories and blacklist go to the kernel, which keeps each item's best
            on_device = cats is not None
            hits = _levels_grid(
                plugin,
                [levels_l[k] for k in keep_l],
                [levels_r[k] for k in keep_r],
                score_threshold,
                cats.left_mask[keep_l] if on_device else None,
                cats.right_mask[keep_r] if on_device else None,
                cats.mode if on_device else _lib.CAT_NONE,
                top_k=top_k,
                banned=_local_banned(banned, keep_l, keep_r),
            )
        elif keep_l.size and keep_r.size:
            on_device = cats is not None and cats.on_device
            hits = _levels_grid(
                plugin,
                [levels_l[k] for k in keep_l],
                [levels_r[k] for k in keep_r],
                score_threshold,
                cats.left_mask[keep_l] if on_device else None,
                cats.right_mask[keep_r] if on_device else None,
                cats.mode if on_device else _lib.CAT_NONE,
                defer=world_size > 1 and not host_filter,
            )
            if isinstance(hits, grid.PendingHits):
                pending = hits
        extra = bool(extra_hits) and 0.0 >= score_threshold
        if world_size > 1:
            # The one exchange step: all-gatherv of the hits.  When every rank's hits sit in ONE device buffer and nothing
            # has to be filtered on the host (no blacklist, the category predicate ran in the kernel, no zero-level pairs)
            # the buffers go GPU -> all-gather -> GPU at a capacity agreed with one MAX all-reduce; otherwise the ranks
            # exchange what they have filtered on the host.  The choice is collective (one MIN all-reduce).
            nothing_to_score = not (keep_l.size and keep_r.size)  # (this rank's shard: it then contributes an empty buffer)
            direct = distributed.agree_all(top_k is None and (pending is not None or nothing_to_score) and not extra and
                                           not host_filter)
        else:
            direct = False
        if direct:
            hs, hi, hj = distributed.all_gather_pending(pending, n_l, nlev_l, nlev_r, world_size)
        else:
            if pending is not None:
                hits = pending.finish()
            if keep_l.size and keep_r.size:
                hi, hj, hs = keep_l[hits.i], keep_r[hits.j], hits.score
            else:
                hi, hj, hs = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
            if extra:
                ei = np.array([p[0] for p in extra_hits], dtype=np.int64)
                ej = np.array([p[1] for p in extra_hits], dtype=np.int64)
                if floors is not None:  # (a zero-level pair is a row like any other: it passes the same gate)
                    gated = grid.filter_by_floors(grid.Hits(np.zeros(len(ei)), ei, ej), floors[0], floors[1])
                    ei, ej = gated.i, gated.j
                hi, hj, hs = np.concatenate([hi, ei]), np.concatenate([hj, ej]), np.concatenate([hs, np.zeros(len(ei))])

            if top_k is not None:
                # (the kernel applied categories and blacklist; the zero-level pairs join the per-item selection)
                sel = grid.select_top_k(grid.Hits(hs, hi, hj), top_k)
                hi, hj, hs = sel.i, sel.j, sel.score
            # ---- per hit: blacklist (and categories when they could not go to the device)
            elif floors is None and len(hs) and host_filter:
                ok = np.fromiter(
                    (
                        (int(a), int(b)) not in banned and (cats is None or cats.on_device or cats.match(int(a), int(b)))
                        for a, b in zip(hi, hj)
                    ),
                    dtype=bool, count=len(hs),
                )
                hi, hj, hs = hi[ok], hj[ok], hs[ok]

            if world_size > 1:  # (host-filtered hits: packed, copied to the device, gathered, copied back)
                hs, hi, hj = distributed.all_gather_hits(hs, hi, hj)

        if one_to_one and len(hs):
            taken = grid.assign_hits(grid.Hits(hs, hi.astype(np.int32), hj.astype(np.int32)), n_l, n_r)
            hi, hj, hs = taken.i.astype(np.int64), taken.j.astype(np.int64), taken.score

        # ---- output frame in the reference's row order (pair label ascending)
        label = hi.astype(np.int64) * n_r + hj.astype(np.int64)
        order = np.argsort(label, kind="stable")
        hi, hj, hs, label = hi[order], hj[order], hs[order], label[order]
        lf = lf.assign(**{COMP_COLUMN: levels_l, QUESTION_OUTPUT: argument_l})
        rf = rf.assign(**{COMP_COLUMN: levels_r, QUESTION_OUTPUT: argument_r})
        out = {}
        for frame, prefix, rows in ((lf, lp, hi), (rf, rp, hj)):
            for col in frame.columns:  # survivors keep the frame's column order (:236-240)
                if col in COLUMN_NAMES:
                    out[prefix + col] = frame[col].to_numpy()[rows] if len(rows) else frame[col].to_numpy()[:0]
        out[MATCH_SCORE] = hs
        table = pd.DataFrame(out, index=pd.Index(label))
        logger.info("got %s entries", "{:,}".format(len(table)))
        return Comparable(data=table, left_name=lp, right_name=rp)


# =============================================================================== helpers
def remove_existing_mappings(
    left: ComparableData, right: ComparableData, left_name: str, right_name: str, existing_mappings: Mapping
) -> None:
    """:493-513 -- drop items already linked by a whitelist entry; skipped as a whole on KeyError."""
    try:
        left_ids = left.get_existing_mapping_ids(left_name, existing_mappings)
        right_ids = right.get_existing_mapping_ids(right_name, existing_mappings)
    except KeyError:
        return
    used = set(left_ids) & set(right_ids)
    filtered = existing_mappings.get_filtered(used)
    left.remove_existing_mappings(get_identifiers_from_mapping(filtered, left_name))
    right.remove_existing_mappings(get_identifiers_from_mapping(filtered, right_name))


def _resolve_plugin(score_func):
    if isinstance(score_func, str):
        return getattr(score_functions, score_func)
    if any(score_func is plugin for plugin in score_functions.PLUGINS):
        return score_func
    raise NotImplementedError(
        "only this package's score functions (" + ", ".join(p.__name__ for p in score_functions.PLUGINS) +
        ") have a device implementation"
    )


def _check_best_args(best_margin, mutual_best, top_k):
    """``best_margin`` / ``mutual_best`` of ``compare``: the margin as a float (None: no best filter), else ``ValueError`` --
    before any device work."""
    if best_margin is None:
        if mutual_best:
            raise ValueError("mutual_best needs best_margin (0.0: exact best matches)")
        return None
    if top_k is not None:
        raise ValueError("best_margin and top_k cannot be combined")
    return grid.check_margin(best_margin)


def _check_one_to_one(one_to_one, top_k, best_margin) -> bool:
    """``one_to_one`` of ``compare``: a bool that excludes the per-item queries, else ``ValueError`` -- before any device
    work."""
    if not isinstance(one_to_one, (bool, np.bool_)):
        raise ValueError(f"one_to_one must be a bool, got {one_to_one!r}")
    if one_to_one and top_k is not None:
        raise ValueError("one_to_one and top_k cannot be combined")
    if one_to_one and best_margin is not None:
        raise ValueError("one_to_one and best_margin cannot be combined")
    return bool(one_to_one)


def _prelude_profile(pre, t) -> grid.ThresholdProfile:
    """The threshold profile of the frame ``compare`` returns for the prelude ``pre`` (``_compare_prelude``), by position
    in the compared frames: the device grid's over the items with levels, merged with the zero-level x zero-level pairs,
    which score 0.  Categories and blacklist run in the kernel."""
    parts = []
    if pre.keep_l.size and pre.keep_r.size:
        on_device = pre.cats is not None
        parts.append((_levels_grid(
            pre.plugin, [pre.levels_l[k] for k in pre.keep_l], [pre.levels_r[k] for k in pre.keep_r], float(t[0]),
            pre.cats.left_mask[pre.keep_l] if on_device else None, pre.cats.right_mask[pre.keep_r] if on_device else None,
            pre.cats.mode if on_device else _lib.CAT_NONE, banned=_local_banned(pre.banned, pre.keep_l, pre.keep_r),
            profile=t), pre.keep_l, pre.keep_r))
    if pre.extra_hits:  # zero-level x zero-level pairs score 0
        ei = np.array([p[0] for p in pre.extra_hits], dtype=np.int32)
        ej = np.array([p[1] for p in pre.extra_hits], dtype=np.int32)
        parts.append((grid.profile_of_hits(grid.Hits(np.zeros(len(ei)), ei, ej), t, pre.n_l, pre.n_r), np.arange(pre.n_l),
                      np.arange(pre.n_r)))
    return grid.merge_profiles(parts, t, pre.n_l, pre.n_r)


def _banned_positions(pairs, id_l: Sequence, id_r: Sequence) -> set:
    if not pairs:
        return set()
    pos_l: Dict[object, List[int]] = {}
    pos_r: Dict[object, List[int]] = {}
    for k, v in enumerate(id_l):
        pos_l.setdefault(v, []).append(k)
    for k, v in enumerate(id_r):
        pos_r.setdefault(v, []).append(k)
    out = set()
    for a, b in pairs:
        for i in pos_l.get(a, ()):
            for j in pos_r.get(b, ()):
                out.add((i, j))
    return out


def _first_surviving_pair(n_l: int, n_r: int, banned: set) -> Optional[Tuple[int, int]]:
    for i in range(n_l):
        for j in range(n_r):
            if (i, j) not in banned:
                return i, j
    return None


def _empty_levels(levels: Sequence[Sequence]) -> frozenset:
    """Indices of the item's EMPTY levels that a step can reach: step s >= 1 uses level min(s, L - 1), so level 0 only
    counts for a one-level item.  (Nested levels: the empty ones are a prefix; the reference's tokenizer may yield any.)"""
    n = len(levels)
    return frozenset(k for k, lv in enumerate(levels) if len(lv) == 0 and (k >= 1 or n == 1))


def _divides_by_zero(levels_l, empty_l: frozenset, levels_r, empty_r: frozenset, predicate=None) -> bool:
    """Does ``compare_terms`` reach a step at which the plugin divides by zero?  ``predicate(a, b)``: the plugin's
    ``divides_by_zero`` on the sizes of the step's two sets -- every rule only asks which of them are empty, so 0 / 1 stand
    in for the sizes; None: BOTH level sets empty (score_functions.py:13)."""
    n_l, n_r = len(levels_l), len(levels_r)
    if predicate is None:
        return any(min(s, n_l - 1) in empty_l and min(s, n_r - 1) in empty_r for s in range(1, max(n_l, n_r) + 1))
    return any(predicate(int(min(s, n_l - 1) not in empty_l), int(min(s, n_r - 1) not in empty_r))
               for s in range(1, max(n_l, n_r) + 1))


def _raise_first_pair_error(is_sets, levels_l, levels_r, nlev_l, nlev_r, n_r, survives, extra_hits, predicate=None) -> None:
    zero_l, zero_r = np.flatnonzero(nlev_l == 0), np.flatnonzero(nlev_r == 0)
    candidates: List[Tuple[int, int, type]] = []
    for i in zero_l:
        for j in range(len(nlev_r)):
            if nlev_r[j] == 0:
                extra_hits.append((int(i), j))
            else:
                candidates.append((int(i), j, IndexError))
    for j in zero_r:
        for i in range(len(nlev_l)):
            if nlev_l[i] != 0:
                candidates.append((i, int(j), IndexError))
    if is_sets:
        emp_l = [_empty_levels(v) for v in levels_l]
        emp_r = [_empty_levels(v) for v in levels_r]
        sus_l = [i for i, v in enumerate(emp_l) if v]
        sus_r = [j for j, v in enumerate(emp_r) if v]
        one_side = predicate is not None and (predicate(0, 1) or predicate(1, 0))  # (one empty set is enough to divide by zero)
        some = lambda n: [k for k in range(len(n)) if n[k] > 0]
        pairs = ((i, j) for i in sus_l for j in sus_r)
        if one_side:  # every pair with a suspect on either side, each once
            in_l = set(sus_l)
            pairs = itertools.chain(((i, j) for i in sus_l for j in some(nlev_r)),
                                    ((i, j) for j in sus_r for i in some(nlev_l) if i not in in_l))
        for i, j in pairs:
            if _divides_by_zero(levels_l[i], emp_l[i], levels_r[j], emp_r[j], predicate):
                candidates.append((i, j, ZeroDivisionError))
    best = None
    for i, j, exc in candidates:
        if survives(i, j):
            lab = i * n_r + j
            if best is None or lab < best[0]:
                best = (lab, exc)
    extra_hits[:] = [p for p in extra_hits if survives(*p)]
    if best is not None:
        if best[1] is IndexError:
            raise IndexError("list index out of range")
        raise ZeroDivisionError("division by zero")


def _may_be_wide_sets(*sides) -> bool:
    """Cheap pre-check of the 64-token limit: the largest level's token count WITH repeats (strings: words)."""
    size = lambda lv: len(lv) if isinstance(lv, list) else len(lv.split())
    return any(size(it[-1]) > 64 for items in sides for it in items if len(it))


def _fast_jaccard_levels(levels_l, levels_r, as_set_levels, threshold, cat_l, cat_r, cat_mode, dev, defer=False, top_k=None,
                         banned=None, profile=None, floors=None, measure="union"):
    """The suffix-nested fast layout of both sides + ``nsm_jaccard_levels_grid``; raises ``tables.IrregularLevels`` when an
    item does not fit it.  ``top_k``: ``nsm_jaccard_levels_top_k`` instead, without the ``banned`` pairs (tables without a
    category partition and without an inverted index).  ``profile`` (a ladder of thresholds): ``nsm_jaccard_levels_profile``
    on the same tables.  ``floors`` ((left, right) arrays by position, the right one or None):
    ``nsm_jaccard_levels_floor_grid`` on the same tables.  ``measure``: the plugin's; beside "union" every query is a
    per-item sweep (``nsm_set_levels_*``), the plain grid the floor grid without floors."""
    per_item = top_k is not None or profile is not None or floors is not None or measure != "union"
    part = False if per_item else tables.partition_allowed(cat_mode, cat_l, cat_r)
    index = False if per_item else None
    memo = ComparableData._item_memo
    if memo is not None:
        # inside item_memo(): one vocabulary for the whole run, every item encoded once (tables.LevelPool,
        # keyed by the identity of the memoised level lists)
        pool = memo.setdefault(("level pool",), tables.LevelPool())
        vocab = pool.vocab
        rows = [pool.rows_keyed(levels, as_set_levels) for levels in (levels_l, levels_r)]
        width = tables.pick_width(*(int((ids >= 0).sum(axis=1).max(initial=1)) for ids, _, _ in rows))
        sides = []
        for (ids, plen, nlev), side, cat in zip(rows, ("left", "right"), (cat_l, cat_r)):
            deepest = max(4, -(-(int(nlev.max()) if len(nlev) else 1) // 4) * 4)
            sides.append(tables.SetTable.from_nested_arrays(ids, plen[:, :deepest], nlev, side, dev, categories=cat,
                                                            width=width, category_mode=cat_mode, partition=part,
                                                            index=index))
        lt, rt = sides
    else:
        vocab = tables.Vocabulary()
        sl, sr = [as_set_levels(it) for it in levels_l], [as_set_levels(it) for it in levels_r]
        width = tables.pick_width(
            max((len(set(it[-1])) for it in sl if it), default=1), max((len(set(it[-1])) for it in sr if it), default=1)
        )
        lt = tables.SetTable.from_levels(sl, "left", dev, vocab, width=width, categories=cat_l, category_mode=cat_mode,
                                         partition=part, index=index)
        rt = tables.SetTable.from_levels(sr, "right", dev, vocab, width=width, categories=cat_r,
                                         category_mode=cat_mode, partition=part, index=index)
    if len(vocab) >= 1 << 25:
        raise NotImplementedError("vocabulary of 2^25 or more distinct tokens")
    if profile is not None:
        return grid.jaccard_levels_profile(lt, rt, profile, category_mode=cat_mode, banned=banned, measure=measure)
    if floors is not None:
        return grid.jaccard_levels_floor_grid(lt, rt, threshold, floors[0], floors[1], category_mode=cat_mode, banned=banned,
                                              measure=measure)
    if top_k is not None:
        return grid.jaccard_levels_top_k(lt, rt, top_k, threshold, category_mode=cat_mode, banned=banned, measure=measure)
    if measure != "union":
        return grid.jaccard_levels_grid(lt, rt, threshold, category_mode=cat_mode, defer=defer, measure=measure, banned=banned)
    # the library picks the inverted-index kernel from the threshold alone (it cannot see the vocabulary); the host
    # can: with a large vocabulary few pairs share an id and the index wins at every threshold (3 x 100k^2 items of
    # ~8 ids: 20k words 2.1 vs 2.2 ms at 0.7 and 4.2 vs 22 ms at 0.1; 2^17 words 1.0 vs 2.3 ms and 1.8 vs 20.9 ms)
    use_index = True if (threshold > 0 and len(vocab) >= 8192) else None
    return grid.jaccard_levels_grid(lt, rt, threshold, category_mode=cat_mode, index=use_index, defer=defer)


def _levels_grid(plugin, levels_l, levels_r, threshold, cat_l, cat_r, cat_mode=_lib.CAT_NONE, defer: bool = False, top_k=None,
                 banned=None, profile=None, floors=None):
    """Encode both sides' levels for ``plugin`` and run the levels grid on the current device.  ``defer``: when the
    whole grid goes through ONE fast kernel call, return its hits still on the device (``grid.PendingHits``: the sharded
    ``gen_comparable`` exchanges them without a host detour); grids that are split (wide / irregular items) return
    ``grid.Hits`` as always.

    ``top_k``: per left item only the first ``top_k`` records (score descending, right index ascending) of that grid
    without the ``banned`` pairs ((left, right) positions in these lists, or None); ``defer`` is then ignored.  Items the
    fast kernels take go through ``nsm_*_levels_top_k`` (tables without a category partition or an inverted index: an item
    must stay one row to keep one list); wide or irregular items through the general kernels at the threshold, cut per
    item on the host; the parts are disjoint in j for every i, so the per-item selection over their union is the answer.

    ``profile`` (a validated ladder, ``threshold`` its first entry): the grid's ``grid.ThresholdProfile`` without the
    ``banned`` pairs instead of its hits, routed like a top-k query -- ``nsm_*_levels_profile`` for the items the fast
    kernels take, ``grid.profile_of_hits`` of the general kernels' hits for the rest, merged.

    ``floors`` ((left floors, right floors or None), float64 by position in these lists): only the records of that grid
    without the ``banned`` pairs that reach both their items' floors (``grid.filter_by_floors``), routed like a top-k
    query -- ``nsm_*_levels_floor_grid`` with the floors gathered to the sub-tables for the items the fast kernels take, the
    general kernels' hits gated on the host for the rest."""
    import torch

    if not torch.cuda.is_available():
        raise _lib.NsmLibraryError("the match loop runs on an MI355X (HIP device); there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    from .. import wide

    # (idx None: the whole side)
    sub = lambda seq, idx: seq if idx is None else [seq[k] for k in idx]
    cut = lambda cat, idx: cat if cat is None or idx is None else np.asarray(cat)[np.asarray(idx, dtype=np.int64)]
    cut_floors = lambda li, ri: None if floors is None else (cut(floors[0], li), cut(floors[1], ri))

    def split_grid(split, fast, general):
        """The parts of a split grid, merged; a top-k query cuts the general parts and the merged result per item."""
        if floors is not None:
            gate = lambda li, ri: grid.filter_by_floors(_drop_banned(general(li, ri), banned, li, ri), *cut_floors(li, ri))
            return wide.split_grid(split[0], split[1], fast, gate)
        if profile is not None:
            tally = lambda li, ri: grid.profile_of_hits(_drop_banned(general(li, ri), banned, li, ri), profile, len(li), len(ri))
            return wide.split_profile(split, len(levels_l), len(levels_r), profile, fast, tally)
        if top_k is None:
            return wide.split_grid(split[0], split[1], fast, general)
        cut_general = lambda li, ri: grid.select_top_k(_drop_banned(general(li, ri), banned, li, ri), top_k)
        return grid.select_top_k(wide.split_grid(split[0], split[1], fast, cut_general), top_k)

    if plugin.kind == "sets":
        as_set_levels = lambda it: [lv if isinstance(lv, list) else lv.split() for lv in it]
        def split_route(split):
            # items of more than 64 distinct tokens / more than 64 levels / levels that are not suffix-nested leave the fast
            # path (wide.py: general kernel, every step's level sets scored on their own); the rest is scored as always
            fast = lambda li, ri: _levels_grid(plugin, sub(levels_l, li), sub(levels_r, ri), threshold, cut(cat_l, li),
                                               cut(cat_r, ri), cat_mode, top_k=top_k, banned=_restrict_banned(banned, li, ri),
                                               profile=profile, floors=cut_floors(li, ri))
            general = lambda li, ri: wide.jaccard_any_grid(
                [as_set_levels(levels_l[k]) for k in li], [as_set_levels(levels_r[k]) for k in ri], threshold, cut(cat_l, li),
                cut(cat_r, ri), cat_mode, device=dev)
            return split_grid(split, fast, general)

        measure = plugin.measure
        split = wide.wide_set_items([as_set_levels(it) for it in levels_l], [as_set_levels(it) for it in levels_r]) \
            if _may_be_wide_sets(levels_l, levels_r) else None
        if split is not None:
            _need_general(plugin, f"an item of more than {wide.FAST_TOKENS} distinct tokens or {wide.FAST_LEVELS} levels")
            return split_route(split)
        try:
            return _fast_jaccard_levels(levels_l, levels_r, as_set_levels, threshold, cat_l, cat_r, cat_mode, dev,
                                        defer and top_k is None and floors is None, top_k, banned, profile, floors, measure)
        except tables.IrregularLevels:
            _need_general(plugin, "an item whose levels are not suffix-nested")
            # the reference scores whatever its tokenizer yields per level (:283-299): find the items the nested layout
            # cannot hold and route only them
            split = wide.wide_set_items([as_set_levels(it) for it in levels_l], [as_set_levels(it) for it in levels_r],
                                        nesting=True)
            if split is None:
                raise
            return split_route(split)
    prep = lambda items: ComparableData._memoised(
        "fuzzy", items, lambda it: [score_functions.fuzzy_operand(lv) for lv in it])
    ops_l, ops_r = prep(levels_l), prep(levels_r)

    metric = getattr(plugin, "metric", "indel")  # (beside "indel" every query is a per-item sweep: tables without a category partition)

    def fast(li, ri, defer=False):
        if profile is not None:
            a, b, c, d = tables.encode_level_strings(sub(ops_l, li), sub(ops_r, ri), dev, cut(cat_l, li), cut(cat_r, ri), cat_mode,
                                                     partition=False)
            return grid.indel_levels_profile(a, b, c, d, profile, category_mode=cat_mode, banned=_restrict_banned(banned, li, ri),
                                             metric=metric)
        if floors is not None:
            a, b, c, d = tables.encode_level_strings(sub(ops_l, li), sub(ops_r, ri), dev, cut(cat_l, li), cut(cat_r, ri), cat_mode,
                                                     partition=False)
            return grid.indel_levels_floor_grid(a, b, c, d, threshold, *cut_floors(li, ri), category_mode=cat_mode,
                                                banned=_restrict_banned(banned, li, ri), metric=metric)
        if top_k is None and metric != "indel":
            a, b, c, d = tables.encode_level_strings(sub(ops_l, li), sub(ops_r, ri), dev, cut(cat_l, li), cut(cat_r, ri), cat_mode,
                                                     partition=False)
            return grid.indel_levels_grid(a, b, c, d, threshold, category_mode=cat_mode, defer=defer, metric=metric,
                                          banned=_restrict_banned(banned, li, ri))
        if top_k is None:
            a, b, c, d = tables.encode_level_strings(sub(ops_l, li), sub(ops_r, ri), dev, cut(cat_l, li), cut(cat_r, ri), cat_mode)
            return grid.indel_levels_grid(a, b, c, d, threshold, category_mode=cat_mode, defer=defer)
        a, b, c, d = tables.encode_level_strings(sub(ops_l, li), sub(ops_r, ri), dev, cut(cat_l, li), cut(cat_r, ri), cat_mode,
                                                 partition=False)
        return grid.indel_levels_top_k(a, b, c, d, top_k, threshold, category_mode=cat_mode,
                                       banned=_restrict_banned(banned, li, ri), metric=metric)

    split = wide.wide_string_items(ops_l, ops_r)
    if split is None:
        return fast(None, None, defer)
    _need_general(plugin, f"a level string of more than {wide.FAST_LEN} code units, more than {wide.FAST_ALPHABET} distinct code "
                          f"units in the grid, or an item of more than {wide.FAST_LEVELS} levels")
    # level strings of more than 512 code units / a grid of more than 255 distinct code units (wide.py)
    general = lambda li, ri: wide.indel_any_grid(sub(ops_l, li), sub(ops_r, ri), threshold, cut(cat_l, li), cut(cat_r, ri),
                                                 cat_mode, device=dev)
    return split_grid(split, fast, general)


def _need_general(plugin, what: str) -> None:
    """The general (any-operand) kernels score Jaccard and the Indel ratio alone: another measure or string metric refuses
    what only they can take, before any launch."""
    if getattr(plugin, "measure", "union") != "union":
        raise NotImplementedError(f"{plugin.__name__}: {what} (measure {plugin.measure!r} has no general kernel)")
    if getattr(plugin, "metric", "indel") != "indel":
        raise NotImplementedError(f"{plugin.__name__}: {what} (metric {plugin.metric!r} has no general kernel)")


# =============================================================================== listed pairs
_NO_LEVELS: list = []  # stands in for the items no listed pair names


def _levels_pairs(plugin, levels_l, levels_r, pi: np.ndarray, pj: np.ndarray) -> np.ndarray:
    """``compare_terms`` x ``plugin`` of the listed pairs ``(levels_l[pi[p]], levels_r[pj[p]])`` -- every item with at
    least one level, no pair the reference raises for -- on the current device: tables of the listed items only, one
    ``nsm_*_levels_pairs`` launch.  Pairs with an item the fast layouts cannot hold (``wide.py``) go through
    ``_levels_grid``'s general kernels instead, one 1 x partners grid per distinct left item of such pairs."""
    import torch

    if not torch.cuda.is_available():
        raise _lib.NsmLibraryError("the match loop runs on an MI355X (HIP device); there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    from .. import wide

    pi, pj = np.asarray(pi, dtype=np.int64), np.asarray(pj, dtype=np.int64)
    used = lambda items, idx: [items[k] if k in idx else _NO_LEVELS for k in range(len(items))]  # (unlisted items: not looked at)
    set_l, set_r = set(pi.tolist()), set(pj.tolist())
    if plugin.kind == "sets":
        as_set_levels = lambda it: [lv if isinstance(lv, list) else lv.split() for lv in it]
        sl, sr = [as_set_levels(it) for it in used(levels_l, set_l)], [as_set_levels(it) for it in used(levels_r, set_r)]

        def fast(li, ri, qi, qj):
            vocab = tables.Vocabulary()
            a, b = [sl[k] for k in li], [sr[k] for k in ri]
            width = tables.pick_width(max((len(set(it[-1])) for it in a if it), default=1),
                                      max((len(set(it[-1])) for it in b if it), default=1))
            lt = tables.SetTable.from_levels(a, "left", dev, vocab, width=width, partition=False, index=False)
            rt = tables.SetTable.from_levels(b, "right", dev, vocab, width=width, partition=False, index=False)
            return grid.jaccard_levels_pairs(lt, rt, qi, qj, measure=plugin.measure)

        general = lambda li, ri: wide.jaccard_any_grid([sl[k] for k in li], [sr[k] for k in ri], float("-inf"), device=dev)
        split = wide.wide_set_items(sl, sr)
        if split is not None:
            _need_general(plugin, f"an item of more than {wide.FAST_TOKENS} distinct tokens or {wide.FAST_LEVELS} levels")
        try:
            return wide.split_pairs(split, pi, pj, fast, general)
        except tables.IrregularLevels:  # levels that are not suffix-nested: only those items leave the fast path
            _need_general(plugin, "an item whose levels are not suffix-nested")
            split = wide.wide_set_items(sl, sr, nesting=True)
            if split is None:
                raise
            return wide.split_pairs(split, pi, pj, fast, general)
    prep = lambda items: ComparableData._memoised("fuzzy", items, lambda it: [score_functions.fuzzy_operand(lv) for lv in it])
    ops_l, ops_r = prep(used(levels_l, set_l)), prep(used(levels_r, set_r))

    def fast(li, ri, qi, qj):
        a, b, c, d = tables.encode_level_strings([ops_l[k] for k in li], [ops_r[k] for k in ri], dev, partition=False)
        return grid.indel_levels_pairs(a, b, c, d, qi, qj, metric=getattr(plugin, "metric", "indel"))

    general = lambda li, ri: wide.indel_any_grid([ops_l[k] for k in li], [ops_r[k] for k in ri], float("-inf"), device=dev)
    split = wide.wide_string_items(ops_l, ops_r)
    if split is not None:
        _need_general(plugin, f"a level string of more than {wide.FAST_LEN} code units, more than {wide.FAST_ALPHABET} distinct "
                              f"code units among the listed items, or an item of more than {wide.FAST_LEVELS} levels")
    return wide.split_pairs(split, pi, pj, fast, general)


# =============================================================================== per-item top-k
def _local_banned(banned: set, keep_l: np.ndarray, keep_r: np.ndarray):
    """The blacklist's pairs among the items ``keep_l`` x ``keep_r`` as (left, right) positions in those lists."""
    if not banned:
        return None
    pos_l = {int(g): k for k, g in enumerate(keep_l)}
    pos_r = {int(g): k for k, g in enumerate(keep_r)}
    pairs = [(pos_l[a], pos_r[b]) for a, b in banned if a in pos_l and b in pos_r]
    if not pairs:
        return None
    arr = np.array(pairs, dtype=np.int64)
    return arr[:, 0], arr[:, 1]


def _restrict_banned(banned, li, ri):
    """``banned`` (positions in the parent lists) restricted to the sub-grid ``li`` x ``ri`` (None: the whole grid), in
    positions of the sub-lists."""
    if banned is None or li is None:
        return banned
    li, ri = np.asarray(li, dtype=np.int64), np.asarray(ri, dtype=np.int64)
    bi, bj = banned
    size = lambda idx, b: int(max(idx.max(initial=-1), b.max(initial=-1))) + 1
    pos_l = np.full(size(li, bi), -1, dtype=np.int64)
    pos_r = np.full(size(ri, bj), -1, dtype=np.int64)
    pos_l[li], pos_r[ri] = np.arange(len(li)), np.arange(len(ri))
    ok = (pos_l[bi] >= 0) & (pos_r[bj] >= 0)
    return (pos_l[bi][ok], pos_r[bj][ok]) if ok.any() else None


def _drop_banned(hits: grid.Hits, banned, li, ri) -> grid.Hits:
    """``hits`` of the sub-grid ``li`` x ``ri`` without the pairs of ``banned`` (positions in the parent lists)."""
    if banned is None or len(hits) == 0:
        return hits
    li, ri = np.asarray(li, dtype=np.int64), np.asarray(ri, dtype=np.int64)
    n_r = int(max(ri.max(initial=-1), banned[1].max(initial=-1))) + 1
    ok = ~np.isin(li[hits.i] * n_r + ri[hits.j], banned[0] * n_r + banned[1])
    return grid.Hits(hits.score[ok], hits.i[ok], hits.j[ok])
