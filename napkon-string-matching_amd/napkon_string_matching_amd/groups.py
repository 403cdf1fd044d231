"""From match results to a ``Mapping``: entries ``{id: {cohort: [identifier, ...]}}`` that hold every spelling of one
concept across all cohorts.

The reference builds such entries on the host by merging pairs that share an item (``Mapping.update_mapping``, reached from
``MatchedMapping.read_excel(combine_entries=True)``: napkon_string_matching/types/mapping.py).  Here the pairs of ALL cohort
pairs of a ``Matcher`` run are closed transitively in one ``grid.group_hits`` call (``nsm_group_hits``,
include/nsm_hip_groups.h): ``hap:A ~ pop:B`` from one frame and ``pop:B ~ suep:C`` from another make one entry.

Three steps, the first and the last pure host functions:

* ``lists_of_results``   frames -> node numbering and hit lists
* ``grid.group_hits``    hit lists -> labels (the device)
* ``mapping_of_labels``  labels -> ``Mapping``

``forest_of_results`` is the same at EVERY threshold from one device call: ``grid.span_hits`` (``nsm_span_hits``,
include/nsm_hip_span.h) in place of ``grid.group_hits``, and ``ResultForest.mapping(threshold)`` cuts it on the host.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import grid
from .types.comparable import IDENTIFIER, MATCH_SCORE, ComparisonResults
from .types.mapping import Mapping


def lists_of_results(results: ComparisonResults):
    """The node space and hit lists of a run's frames.  Cohort of a side = ``left_name.lower()`` / ``right_name.lower()``;
    nodes are the distinct identifiers per cohort -- cohorts sorted case-insensitively as the Matcher sorts them,
    identifiers sorted -- so an identifier that several rows or frames repeat is ONE node.  Returns
    ``(cohorts, identifiers, lists)``: the cohort names, per cohort its identifiers in node order, and
    ``[(Hits, left_base, right_base), ...]`` with one list per frame, ids relative to the cohort's base."""
    frames = []
    found: Dict[str, set] = {}
    for _key, comp in results.items():
        cl, cr = comp.left_name.lower(), comp.right_name.lower()
        frame = comp.dataframe()
        if len(frame) == 0:
            left, right, score = [], [], np.zeros(0, dtype=np.float64)
        else:
            left = [str(v) for v in frame[comp.left_name + IDENTIFIER].tolist()]
            right = [str(v) for v in frame[comp.right_name + IDENTIFIER].tolist()]
            score = frame[MATCH_SCORE].to_numpy(dtype=np.float64)
        found.setdefault(cl, set()).update(left)
        found.setdefault(cr, set()).update(right)
        frames.append((cl, cr, left, right, score))
    cohorts = sorted(found, key=lambda name: (name.lower(), name))
    identifiers = [sorted(found[c]) for c in cohorts]
    bases = dict(zip(cohorts, np.r_[0, np.cumsum([len(v) for v in identifiers])].tolist()))
    where = {c: {ident: k for k, ident in enumerate(ids)} for c, ids in zip(cohorts, identifiers)}
    lists = []
    for cl, cr, left, right, score in frames:
        i = np.fromiter((where[cl][v] for v in left), dtype=np.int32, count=len(left))
        j = np.fromiter((where[cr][v] for v in right), dtype=np.int32, count=len(right))
        lists.append((grid.Hits(score, i, j), bases[cl], bases[cr]))
    return cohorts, identifiers, lists


def node_id(cohort: str, identifier: str) -> str:
    """The entry id a component gets from its smallest node: stable across runs, 32 hex digits like the reference's
    ``uuid4().hex``."""
    return hashlib.md5(f"{cohort}\0{identifier}".encode()).hexdigest()


def mapping_of_labels(label, cohorts: Sequence[str], identifiers: Sequence[Sequence[str]],
                      id_reference: Optional[Mapping] = None) -> Mapping:
    """Labels -> ``Mapping``.  ``label[v]`` is the smallest node of node v's component (``grid.groups_of_hits``), node
    ``sum(len(identifiers[:c])) + k`` is ``identifiers[c][k]`` of ``cohorts[c]``.  An entry is a component with at least two
    identifiers: ``{cohort: [identifiers in node order]}``, cohorts without a member left out; entries in label order.

    Entry id: with ``id_reference`` the first reference id (in the reference's iteration order) that holds any member of
    the component; an id is given once, and a later claimant -- like every component no reference entry holds -- gets
    ``node_id`` of its smallest node."""
    label = np.asarray(label)
    sizes = [len(ids) for ids in identifiers]
    bases = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    if len(cohorts) != len(identifiers) or label.shape != (int(bases[-1]),):
        raise ValueError(f"mapping_of_labels: {label.shape} labels for {int(bases[-1])} identifiers in {len(cohorts)} cohorts")
    groups = grid.MatchGroups(label, tuple(bases[:-1].tolist()), tuple(sizes)).members(2)
    named: List[Tuple[str, str, Dict[str, List[str]]]] = []  # (cohort, identifier) of the smallest node, members
    for members in groups:
        entry = {c: [identifiers[k][m] for m in part.tolist()] for k, (c, part) in enumerate(zip(cohorts, members)) if len(part)}
        first = next(iter(entry))
        named.append((first, entry[first][0], entry))
    wanted: Dict[int, str] = {}  # component -> the first reference id that holds any of its members
    if id_reference is not None:
        holder = {(c, ident): g for g, (_c, _i, entry) in enumerate(named) for c, ids in entry.items() for ident in ids}
        for ref_id, ref_entry in id_reference.items():
            for c, ids in ref_entry.dict().items():
                for ident in ids:
                    if (c, ident) in holder:
                        wanted.setdefault(holder[(c, ident)], ref_id)
    out: Dict[str, Dict[str, List[str]]] = {}
    given = {ref_id for g, ref_id in wanted.items()}
    for g, (cohort, identifier, entry) in enumerate(named):
        key = wanted.get(g)
        if key is None or key in out:  # no reference entry holds a member, or an earlier component took the id
            key = node_id(cohort, identifier)
            while key in out or key in given:  # (a reference that carries this very id for another component)
                key = hashlib.md5(key.encode()).hexdigest()
        out[key] = entry
    return Mapping(out)


def mapping_of_results(results: ComparisonResults, min_score: Optional[float] = None, id_reference: Optional[Mapping] = None,
                       device=None, min_support=0) -> Mapping:
    """The ``Mapping`` of a run: every frame's rows scoring ``>= min_score`` (None: all rows) are edges between
    identifiers, closed transitively over ALL frames in one ``grid.group_hits`` call.  ``min_support > 0``: only the rows of
    the ``(min_support + 2)``-truss link (``grid.group_hits``): with 1, ``hap:A ~ pop:B`` and ``pop:B ~ suep:C`` make an
    entry only where ``hap:A ~ suep:C`` is a row too.  Needs three or more cohorts: two are a bipartite graph."""
    min_support = grid.check_min_support(min_support)
    cohorts, identifiers, lists = lists_of_results(results)
    nodes = sum(len(ids) for ids in identifiers)
    floor = float("-inf") if min_score is None else float(min_score)
    label = grid.group_hits(lists, nodes, floor, device=device, min_support=min_support)
    return mapping_of_labels(label, cohorts, identifiers, id_reference)


@dataclass
class ResultForest:
    """The merge forest of a run's frames with the node naming of ``lists_of_results``: cohort ``c``'s identifier ``k`` is
    node ``forest.bases[c] + k``."""

    forest: grid.MergeForest
    cohorts: List[str]
    identifiers: List[List[str]]

    def mapping(self, threshold: float, id_reference: Optional[Mapping] = None) -> Mapping:
        """``mapping_of_results(results, min_score=threshold)`` without another pass over the frames (``ValueError`` below
        the forest's ``min_score``)."""
        return mapping_of_labels(self.forest.cut(threshold).label, self.cohorts, self.identifiers, id_reference)

    def ladder(self, thresholds) -> dict:
        """``forest.ladder``: per threshold the components, the entries (groups of at least two identifiers), the
        identifiers in entries and the largest entry's size."""
        return self.forest.ladder(thresholds)


def forest_of_results(results: ComparisonResults, min_score: Optional[float] = None, device=None) -> ResultForest:
    """The merge forest of a run: every frame's rows scoring ``>= min_score`` (None: all rows) are edges between
    identifiers, spanned over ALL frames in one ``grid.span_hits`` call.  ``.mapping(t)`` is ``mapping_of_results(results,
    min_score=t)`` for every ``t >= min_score``."""
    cohorts, identifiers, lists = lists_of_results(results)
    sizes = [len(ids) for ids in identifiers]
    bases = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    floor = float("-inf") if min_score is None else float(min_score)
    forest = grid.span_hits(lists, int(bases[-1]), floor, device=device, bases=tuple(bases[:-1].tolist()), cohort_sizes=tuple(sizes))
    return ResultForest(forest, cohorts, identifiers)
