"""Hit lists for merge forests (``grid.forest_of_hits`` / ``nsm_span_hits``, include/nsm_hip_span.h), an independent
reference, and the helpers both test files share.

Every family is a ``match_groups.Case``: a few ``HitList`` s over one node space and the ``min_score`` they are spanned
under.  Built once per process (``case(name)``), never modified; the reference's records are cached beside it
(``answer(name)``).

The reference is NOT Kruskal's walk: it is Prim's algorithm with a heap on the record key, started from the nodes in
ascending order.  The key is worked out here from the bytes of the double (``struct``), not with the package's helper:
score descending by its bits (``+0.0`` before ``-0.0``), then lo, then hi."""
import heapq
import struct
from typing import Dict, List, Tuple

import numpy as np

from support.match_groups import LADDER, Case, HitList, bfs_labels, components, counted, hit_list, same_space, shuffled  # noqa: F401
from support import match_groups as mg


# ---------------------------------------------------------------------------------------------------------- reference
def score_key(score: float) -> int:
    """nsm_sort_hits's K(score) as a Python int: smaller key = earlier record."""
    bits = struct.unpack("<Q", struct.pack("<d", score))[0]
    asc = bits ^ (0xFFFFFFFFFFFFFFFF if bits >> 63 else 1 << 63)
    return asc ^ 0xFFFFFFFFFFFFFFFF


def record_key(score: float, lo: int, hi: int) -> Tuple[int, int, int]:
    return score_key(score), lo, hi


def edges_of(lists, min_score: float):
    """(score, lo, hi) of every record that counts as an edge."""
    out = []
    for l in lists:
        for s, a, b in zip(l.score.tolist(), l.i.tolist(), l.j.tolist()):
            u, v = l.left_base + a, l.right_base + b
            if s >= min_score and u != v:  # (False for a NaN)
                out.append((s, min(u, v), max(u, v)))
    return out


def prim_forest(lists, nodes: int, min_score: float):
    """The merge forest as (score float64, u int32, v int32) in canonical order: Prim with a heap on the record key, one
    tree per unvisited node in ascending order."""
    adjacent: List[list] = [[] for _ in range(nodes)]
    for s, lo, hi in edges_of(lists, min_score):
        item = (record_key(s, lo, hi), s, lo, hi)
        adjacent[lo].append(item)
        adjacent[hi].append(item)
    seen = [False] * nodes
    taken = []
    for first in range(nodes):
        if seen[first]:
            continue
        seen[first] = True
        heap = list(adjacent[first])
        heapq.heapify(heap)
        while heap:
            item = heapq.heappop(heap)
            _key, _s, lo, hi = item
            if seen[lo] and seen[hi]:
                continue
            taken.append(item)
            new = hi if seen[lo] else lo
            seen[new] = True
            for other in adjacent[new]:
                if not (seen[other[2]] and seen[other[3]]):
                    heapq.heappush(heap, other)
    taken.sort(key=lambda item: item[0])
    return (np.asarray([t[1] for t in taken], dtype=np.float64), np.asarray([t[2] for t in taken], dtype=np.int32),
            np.asarray([t[3] for t in taken], dtype=np.int32))


def canonical(score, u, v):
    """Any records in canonical order, by the reference's own key."""
    score, u, v = np.asarray(score, dtype=np.float64), np.asarray(u, dtype=np.int32), np.asarray(v, dtype=np.int32)
    order = sorted(range(len(score)), key=lambda k: record_key(float(score[k]), int(u[k]), int(v[k])))
    order = np.asarray(order, dtype=np.int64)
    return score[order], u[order], v[order]


def same_records(got, want) -> bool:
    """Bitwise: the scores by their 64 bits (``-0.0`` is not ``+0.0``)."""
    return (np.array_equal(np.asarray(got[0], dtype=np.float64).view(np.int64), np.asarray(want[0], dtype=np.float64).view(np.int64))
            and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]))


def as_list(forest, nodes: int) -> HitList:
    """A forest (score, u, v) fed back as a list over the whole node space."""
    return HitList(np.asarray(forest[0], dtype=np.float64), np.asarray(forest[1], dtype=np.int32),
                   np.asarray(forest[2], dtype=np.int32), 0, nodes, 0, nodes)


def round_bound(nodes: int) -> int:
    """ceil(log2(max(nodes, 2))) + 1"""
    return (max(nodes, 2) - 1).bit_length() + 1


# ------------------------------------------------------------------------------------------------------------ families
def _renamed(name: str) -> Case:
    c = mg.case(name)
    return Case(name, c.lists, c.nodes, c.min_score)


def _distinct(nodes: int) -> Case:
    """A random graph whose scores are all different."""
    rng = np.random.default_rng(400 + nodes)
    n = max(1, (2 * nodes) // 3)
    score = (rng.permutation(n) + 1.0) / (n + 1.0)
    return Case(f"distinct_{nodes}", [same_space(score, rng.integers(0, nodes, n), rng.integers(0, nodes, n), nodes)], nodes, 0.0)


def _tied(min_score: float, tag: str) -> Case:
    """A random graph on the four LADDER scores: many ties, and a NaN record between two nodes nothing else touches."""
    rng = np.random.default_rng(77)
    nodes, n = 300, 400
    score = np.r_[np.asarray(LADDER)[rng.integers(0, 4, n)], np.nan]
    return Case(f"tied_{tag}", [same_space(score, np.r_[rng.integers(0, nodes - 2, n), nodes - 2],
                                           np.r_[rng.integers(0, nodes - 2, n), nodes - 1], nodes)], nodes, min_score)


def _thrice() -> Case:
    rng = np.random.default_rng(8)
    nodes, n = 700, 500
    score = np.round(rng.random(n), 2)  # two decimals: ties among different pairs as well
    rep = lambda a: np.repeat(a, 3)
    return Case("every_record_thrice", [same_space(rep(score), rep(rng.integers(0, nodes, n)), rep(rng.integers(0, nodes, n)), nodes)],
                nodes, 0.0)


def _two_scores() -> Case:
    """The pair (2, 5) under 0.4 and under 0.9 (both directions): the higher one is taken.  Without it 2 and 5 meet through
    3 at 0.6, so taking the 0.4 record instead would be a different forest."""
    return Case("one_pair_two_scores", [same_space([0.4, 0.9, 0.6, 0.6, 0.4, 0.3], [2, 5, 2, 3, 5, 0], [5, 2, 3, 5, 2, 1], 8)], 8, 0.0)


def _two_bases() -> Case:
    """A = [0, 40), B = [40, 90), C = [90, 135), scored.  The pair (b7, c5) = nodes (47, 95) comes from list BC as (7, 5)
    and from list (A u B) x C as (47, 5), under different scores; so does (b11, c6)."""
    ab = hit_list([0.9, 0.5, 0.7, 0.6], [3, 3, 10, 20], [7, 8, 11, 30], 0, 40, 40, 50)
    bc = hit_list([0.55, 0.8, 0.65, 0.5], [7, 11, 11, 49], [5, 6, 44, 0], 40, 50, 90, 45)
    abc = hit_list([0.75, 0.6, 0.7], [47, 51, 30], [5, 6, 20], 0, 90, 90, 45)
    ac = hit_list([0.5, 0.85], [30, 31], [20, 21], 0, 40, 90, 45)
    return Case("one_pair_two_bases", [ab, bc, abc, ac], 135, 0.5)


def _self_loops() -> Case:
    k = np.arange(200)
    score = np.r_[np.full(200, 0.9), 0.5, 0.6, 0.7]
    return Case("self_loops", [same_space(score, np.r_[k, 5, 17, 150], np.r_[k, 6, 150, 151], 200)], 200, 0.0)


def _nan() -> Case:
    """The NaN record is the only one between nodes 8 and 9."""
    return Case("nan_record", [same_space([0.5, np.nan, 0.7, np.nan], [0, 8, 1, 0], [1, 9, 2, 2], 10)], 10, 0.0)


def _zeros() -> Case:
    """+0.0 and -0.0 both pass min_score = 0.0 and are different keys: +0.0 first.  The triangle 0-1-2 has two +0.0 edges
    and one -0.0 edge; the square 3-4-5-6 mixes them with a tie-break on (lo, hi)."""
    score = [-0.0, 0.0, 0.0, 0.0, -0.0, 0.0, -0.0, -1e-300]
    return Case("signed_zeros", [same_space(score, [0, 1, 0, 3, 4, 5, 3, 7], [1, 2, 2, 4, 5, 6, 6, 8], 9)], 9, 0.0)


def _infinities() -> Case:
    """-inf passes min_score = -inf: (1, 2) closes a cycle, (5, 6) is the only way to node 6."""
    score = [np.inf, -np.inf, 1.0, np.inf, -np.inf, 0.5]
    return Case("infinities", [same_space(score, [0, 1, 0, 3, 5, 3], [1, 2, 2, 4, 6, 5], 7)], 7, -np.inf)


def _empty_among() -> Case:
    rng = np.random.default_rng(9)
    none = np.zeros(0, int)
    full = lambda: hit_list(np.round(rng.random(40), 1), rng.integers(0, 90, 40), rng.integers(0, 110, 40), 0, 90, 90, 110)
    return Case("empty_among", [hit_list(0.5, none, none, 0, 90, 90, 110), full(), hit_list(0.5, none, none, 0, 0, 0, 0), full(),
                                hit_list(0.5, none, none, 90, 110, 0, 90)], 200, 0.2)


def _overlapping() -> Case:
    """The left range [0, 60) and the right range [30, 100) overlap: (40, 10) is a self-loop, (35, 10) and (40, 5) one pair."""
    rng = np.random.default_rng(31)
    i, j = np.r_[rng.integers(0, 60, 50), 40, 35, 40], np.r_[rng.integers(0, 70, 50), 10, 10, 5]
    return Case("overlapping_ranges", [hit_list(np.round(rng.random(53), 1), i, j, 0, 60, 30, 70)], 100, 0.0)


def _hierarchy() -> Case:
    """1024 nodes, edges v -- v ^ (1 << b) scoring 1 - b / 16: level b joins the groups of level b - 1 in pairs, so every
    round of a Boruvka scheme can only merge pairs -- 10 hooking rounds."""
    v = np.arange(1024)
    i = np.concatenate([v for _ in range(10)])
    j = np.concatenate([v ^ (1 << b) for b in range(10)])
    score = np.concatenate([np.full(1024, 1.0 - b / 16.0) for b in range(10)])
    p = np.random.default_rng(1024).permutation(len(i))
    return Case("hierarchy_1024", [same_space(score[p], i[p], j[p], 1024)], 1024, 0.0)


def _build() -> Dict[str, Case]:
    cases = [_renamed(n) for n in ("path_ascending", "path_descending", "path_shuffled", "star_hub_smallest", "star_hub_largest",
                                   "bipartite_300x300")]
    cases += [_distinct(n) for n in (1, 2, 63, 64, 65, 255, 256, 257, 700)]
    for value in LADDER:
        cases += [_tied(value, f"at_{value}"), _tied(float(np.nextafter(value, -np.inf)), f"below_{value}"),
                  _tied(float(np.nextafter(value, np.inf)), f"above_{value}")]
    cases += [_thrice(), _two_scores(), _two_bases(), _self_loops(), _nan(), _zeros(), _infinities(), _empty_among(), _overlapping(),
              _hierarchy()]
    return {c.name: c for c in cases}


_CASES = _build()
NAMES = list(_CASES)
# one per family, for the tests that cost more per case
FAMILIES = ["path_shuffled", "bipartite_300x300", "distinct_257", "tied_at_0.5", "one_pair_two_bases", "hierarchy_1024"]
# small enough for brute force through cut()
SMALL = ["distinct_63", "distinct_65", "tied_at_0.25", "one_pair_two_scores", "one_pair_two_bases", "nan_record", "signed_zeros",
         "infinities", "overlapping_ranges"]
_ANSWERS: Dict[str, tuple] = {}
_LABELS: Dict[str, np.ndarray] = {}


def case(name: str) -> Case:
    return _CASES[name]


def answer(name: str):
    """The Prim reference's (score, u, v) of a case, computed once and read-only."""
    if name not in _ANSWERS:
        c = _CASES[name]
        got = prim_forest(c.lists, c.nodes, c.min_score)
        for a in got:
            a.setflags(write=False)
        _ANSWERS[name] = got
    return _ANSWERS[name]


def labels(name: str) -> np.ndarray:
    """The breadth-first labels of a case at its min_score."""
    if name not in _LABELS:
        c = _CASES[name]
        got = bfs_labels(c.lists, c.nodes, c.min_score)
        got.setflags(write=False)
        _LABELS[name] = got
    return _LABELS[name]


def cut_points(c: Case) -> List[float]:
    """Every distinct score that counts, and one ulp on either side, as far as they stay >= min_score (no NaN)."""
    scores = sorted({s for s, _, _ in edges_of(c.lists, c.min_score)})
    points = set()
    for s in scores:
        points.update(float(t) for t in (np.nextafter(s, -np.inf), s, np.nextafter(s, np.inf)))
    return sorted(t for t in points if t >= c.min_score)
