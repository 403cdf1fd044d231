"""Hit lists for match groups (``grid.groups_of_hits`` / ``nsm_group_hits``, include/nsm_hip_groups.h), an independent
reference, and the checks both test files share.

Every family is a ``Case``: a few ``HitList`` s over one node space and the ``min_score`` they are grouped under.  Built
once per process (``case(name)``), never modified; the reference's labels are cached beside it (``answer(name)``).

The reference is NOT a union-find: it builds adjacency lists and runs a breadth-first search from every unvisited node in
ascending order, so a component is labelled by the node its search started from -- its smallest."""
from collections import deque
from dataclasses import dataclass
from typing import Dict, List

import numpy as np


@dataclass
class HitList:
    score: np.ndarray
    i: np.ndarray
    j: np.ndarray
    left_base: int
    left_ids: int
    right_base: int
    right_ids: int

    def __len__(self) -> int:
        return int(self.score.shape[0])

    def hits(self):
        from napkon_string_matching_amd import grid

        return grid.Hits(self.score, self.i, self.j)

    def entry(self):
        """(Hits, left_base, right_base): what ``grid.groups_of_hits`` / ``grid.group_hits`` take."""
        return self.hits(), self.left_base, self.right_base

    def records(self) -> np.ndarray:
        """The 16-byte records as an (n, 2) float64 array, in the order given."""
        n = len(self)
        host = np.zeros((n, 2), dtype=np.float64)
        host[:, 0] = self.score
        ij = host.view(np.int32).reshape(n, 4)
        ij[:, 2], ij[:, 3] = self.i, self.j
        return host


@dataclass
class Case:
    name: str
    lists: List[HitList]
    nodes: int
    min_score: float = 0.0

    def entries(self):
        return [l.entry() for l in self.lists]

    def records(self) -> int:
        return sum(len(l) for l in self.lists)


def hit_list(score, i, j, left_base, left_ids, right_base, right_ids) -> HitList:
    i, j = np.asarray(i, dtype=np.int32), np.asarray(j, dtype=np.int32)
    score = np.full(len(i), float(score)) if np.isscalar(score) else np.asarray(score, dtype=np.float64)
    assert len(score) == len(i) == len(j)
    assert len(i) == 0 or (0 <= i.min() and i.max() < left_ids and 0 <= j.min() and j.max() < right_ids)
    return HitList(score, i, j, int(left_base), int(left_ids), int(right_base), int(right_ids))


def same_space(score, i, j, nodes) -> HitList:
    """A self-join: both sides number the same ``nodes`` nodes."""
    return hit_list(score, i, j, 0, nodes, 0, nodes)


# ---------------------------------------------------------------------------------------------------------- reference
def bfs_labels(lists, nodes: int, min_score: float, start=None) -> np.ndarray:
    """label[v] = the smallest node of v's component: adjacency lists, one breadth-first search per component, started
    from the nodes in ascending order.  ``start``: a forest whose edges (v, start[v]) count too."""
    adjacent = [[] for _ in range(nodes)]
    for l in lists:
        for s, a, b in zip(l.score.tolist(), l.i.tolist(), l.j.tolist()):
            if s >= min_score:  # (False for a NaN)
                u, v = l.left_base + a, l.right_base + b
                adjacent[u].append(v)
                adjacent[v].append(u)
    if start is not None:
        for v, p in enumerate(np.asarray(start).tolist()):
            adjacent[v].append(p)
            adjacent[p].append(v)
    label = [-1] * nodes
    for first in range(nodes):
        if label[first] >= 0:
            continue
        label[first] = first
        queue = deque([first])
        while queue:
            for w in adjacent[queue.popleft()]:
                if label[w] < 0:
                    label[w] = first
                    queue.append(w)
    return np.asarray(label, dtype=np.int32)


def counted(c: Case) -> int:
    """stats[0] of a call on the case: the records with score >= min_score (self-loops and duplicates included)."""
    return int(sum(int((l.score >= c.min_score).sum()) for l in c.lists))


def components(label) -> int:
    label = np.asarray(label)
    return int((label == np.arange(len(label))).sum())


# ------------------------------------------------------------------------------------------------------------ families
def _path(order: str) -> Case:
    """5000 nodes in one chain: longer than any fixed hop count, over several blocks."""
    n = 5000
    k = np.arange(n - 1)
    if order == "descending":
        k = k[::-1].copy()
    elif order == "shuffled":
        k = np.random.default_rng(50).permutation(n - 1)
    return Case(f"path_{order}", [same_space(0.5, k, k + 1, n)], n)


def _star(hub_largest: bool) -> Case:
    leaves = np.arange(3000)
    if hub_largest:  # every hook finds a smaller leaf: the root moves again and again
        return Case("star_hub_largest", [same_space(0.5, np.random.default_rng(30).permutation(leaves), np.full(3000, 3000), 3001)], 3001)
    return Case("star_hub_smallest", [same_space(0.5, np.zeros(3000, int), leaves + 1, 3001)], 3001)


def _bipartite() -> Case:
    i, j = np.meshgrid(np.arange(300), np.arange(300), indexing="ij")
    return Case("bipartite_300x300", [hit_list(0.5, i.ravel(), j.ravel(), 0, 300, 300, 300)], 600)


def _pairs() -> Case:
    """1025 disjoint pairs among 1100 + 1100 nodes; the other 150 are isolated."""
    rng = np.random.default_rng(1025)
    left, right = rng.permutation(1100)[:1025], rng.permutation(1100)[:1025]
    return Case("pairs_1025", [hit_list(0.5, left, right, 0, 1100, 1100, 1100)], 2200)


def _random(name: str, nodes: int, n: int, seed: int, repeat: int = 1) -> Case:
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, nodes, n), rng.integers(0, nodes, n)
    return Case(name, [same_space(0.5, np.repeat(i, repeat), np.repeat(j, repeat), nodes)], nodes)


def _self_loops() -> Case:
    """Records (i, i) under equal bases link nothing; three real edges among them."""
    k = np.arange(200)
    return Case("self_loops", [same_space(0.5, np.r_[k, 5, 17, 150], np.r_[k, 6, 150, 151], 200)], 200)


def _empty_among() -> Case:
    rng = np.random.default_rng(9)
    none = np.zeros(0, int)
    full = lambda: hit_list(0.5, rng.integers(0, 90, 40), rng.integers(0, 110, 40), 0, 90, 90, 110)
    return Case("empty_among", [hit_list(0.5, none, none, 0, 90, 90, 110), full(), hit_list(0.5, none, none, 0, 0, 0, 0), full(),
                                hit_list(0.5, none, none, 90, 110, 0, 90)], 200)


def _overlapping() -> Case:
    """The left range [0, 60) and the right range [30, 100) overlap."""
    rng = np.random.default_rng(31)
    return Case("overlapping_ranges", [hit_list(0.5, rng.integers(0, 60, 50), rng.integers(0, 70, 50), 0, 60, 30, 70)], 100)


def _three_cohorts() -> Case:
    """A = [0, 40), B = [40, 90), C = [90, 135).  a ~ b only in list AB and b ~ c only in list BC: A and C meet by
    transitivity alone (list AC holds unrelated pairs)."""
    ab = hit_list(0.5, [3, 3, 10, 20], [7, 8, 11, 30], 0, 40, 40, 50)
    bc = hit_list(0.5, [7, 11, 11, 49], [5, 6, 44, 0], 40, 50, 90, 45)
    ac = hit_list(0.5, [30, 31], [20, 21], 0, 40, 90, 45)
    return Case("three_cohorts", [ab, bc, ac], 135)


LADDER = (0.25, 0.5, 0.75, 1.0)


def _ladder(min_score: float, tag: str) -> Case:
    """Scores on four values: a chain whose k-th edge scores LADDER[k % 4], and a NaN record between two nodes nothing
    else touches."""
    n = 300
    k = np.arange(n - 3)
    score = np.r_[np.asarray(LADDER)[k % 4], np.nan]
    return Case(f"ladder_{tag}", [same_space(score, np.r_[k, n - 2], np.r_[k + 1, n - 1], n)], n, min_score)


def _build() -> Dict[str, Case]:
    cases = [_path("ascending"), _path("descending"), _path("shuffled"), _star(True), _star(False), _bipartite(), _pairs(),
             _random("every_record_thrice", 700, 500, 7, repeat=3), _self_loops(), _empty_among(), _overlapping(), _three_cohorts()]
    cases += [_random(f"nodes_{n}", n, max(1, (2 * n) // 3), 100 + n) for n in (1, 63, 64, 65, 256, 257)]
    for value in LADDER:
        cases += [_ladder(value, f"at_{value}"), _ladder(np.nextafter(value, -np.inf), f"below_{value}"),
                  _ladder(np.nextafter(value, np.inf), f"above_{value}")]
    return {c.name: c for c in cases}


_CASES = _build()
NAMES = list(_CASES)
# one per family, for the tests that cost more per case
FAMILIES = ["path_shuffled", "star_hub_largest", "bipartite_300x300", "pairs_1025", "every_record_thrice", "three_cohorts",
            "ladder_at_0.5"]
_ANSWERS: Dict[str, np.ndarray] = {}


def case(name: str) -> Case:
    return _CASES[name]


def answer(name: str) -> np.ndarray:
    if name not in _ANSWERS:
        c = _CASES[name]
        got = bfs_labels(c.lists, c.nodes, c.min_score)
        got.setflags(write=False)
        _ANSWERS[name] = got
    return _ANSWERS[name]


def shuffled(c: Case, seed: int) -> Case:
    """The same edges: every list's records permuted, the lists in another order."""
    rng = np.random.default_rng(seed)
    lists = []
    for l in c.lists:
        p = rng.permutation(len(l))
        lists.append(HitList(l.score[p], l.i[p], l.j[p], l.left_base, l.left_ids, l.right_base, l.right_ids))
    return Case(c.name + "_shuffled", [lists[k] for k in rng.permutation(len(lists))], c.nodes, c.min_score)
