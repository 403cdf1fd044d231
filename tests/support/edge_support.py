"""Inputs and models for edge support and truss groups (``grid.support_of_hits`` / ``grid.truss_of_hits``,
``nsm_support_hits``): hand graphs with their values as literals, a seeded generator of hit lists, the seam graph whose
supports follow from its construction, a pinned cascade graph, and a numpy restatement of the device scheme."""
import itertools
import re
from pathlib import Path

import numpy as np

SCORES = (0.2, 0.4, 0.6, 0.8, 1.0)


def hits_of(edges, scores=None):
    from napkon_string_matching_amd import grid

    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    score = np.ones(len(e), dtype=np.float64) if scores is None else np.asarray(scores, dtype=np.float64)
    return grid.Hits(score, e[:, 0].copy(), e[:, 1].copy())


def one_list(edges, scores=None):
    """A self-join list over the whole node space."""
    return [(hits_of(edges, scores), 0, 0)]


def complete(n):
    return list(itertools.combinations(range(n), 2))


def strip(n):
    return [(k, k + 1) for k in range(n - 1)] + [(k, k + 2) for k in range(n - 2)]


DIAMOND = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
BOWTIE = [(0, 1), (0, 2), (1, 2), (2, 3), (2, 4), (3, 4)]
K5_TRIANGLE = complete(5) + [(4, 5), (4, 6), (5, 6)]
K33 = [(a, 3 + b) for a in range(3) for b in range(3)]

# name -> (edges, nodes, the support of every edge in that order)
HAND = {
    "triangle": ([(0, 1), (1, 2), (0, 2)], 3, [1, 1, 1]),
    "k4": (complete(4), 4, [2] * 6),
    "k5": (complete(5), 5, [3] * 10),
    "path": ([(k, k + 1) for k in range(6)], 7, [0] * 6),
    "k33": (K33, 6, [0] * 9),
    "diamond": (DIAMOND, 4, [1, 1, 2, 1, 1]),
    "bowtie": (BOWTIE, 5, [1] * 6),
}

# (edges, nodes, min_support) -> (alive edges, rounds)
PEELS = [
    ("diamond", DIAMOND, 4, 2, 0, 3),
    ("strip6_s1", strip(6), 6, 1, len(strip(6)), 1),
    ("strip10_s1", strip(10), 10, 1, len(strip(10)), 1),
    ("strip14_s1", strip(14), 14, 1, len(strip(14)), 1),
    ("strip6_s2", strip(6), 6, 2, 0, 3),
    ("strip10_s2", strip(10), 10, 2, 0, 3),
    ("strip14_s2", strip(14), 14, 2, 0, 3),
    ("k5_triangle_s1", K5_TRIANGLE, 7, 1, 13, 1),
    ("k5_triangle_s2", K5_TRIANGLE, 7, 2, 10, 2),
    ("k5_triangle_s3", K5_TRIANGLE, 7, 3, 10, 2),
    ("k5_triangle_s4", K5_TRIANGLE, 7, 4, 0, 2),
]

FUZZY_CHAIN = ["aaaa", "aaab", "aabb", "abbb", "bbbb"]
FUZZY_CHAIN_SUPPORT_AT_HALF = {(0, 1): 1, (0, 2): 1, (1, 2): 2, (1, 3): 1, (2, 3): 2, (2, 4): 1, (3, 4): 1}


def fuzzy_chain_list(threshold):
    """The self-join of FUZZY_CHAIN under fuzzy_match at ``threshold``, both orientations and the diagonal, as the grid
    reports it: items k apart score 1 - k / 4."""
    recs = [(1.0 - abs(a - b) / 4.0, a, b) for a in range(5) for b in range(5) if 1.0 - abs(a - b) / 4.0 >= threshold]
    return [(hits_of([(a, b) for _, a, b in recs], [s for s, _, _ in recs]), 0, 0)]


def random_graph(seed, nodes, edges):
    """``edges`` distinct pairs (a < b) over ``nodes`` nodes, sorted."""
    rng = np.random.RandomState(seed)
    found = set()
    while len(found) < edges:
        a, b = rng.randint(0, nodes, 2).tolist()
        if a != b:
            found.add((min(a, b), max(a, b)))
    return sorted(found)


def search_cascade(nodes, edges, want_rounds, seeds=range(4000)):
    """The seed search behind CASCADE (run on the CPU): the first seed whose graph peels in at least ``want_rounds`` rounds
    at ``min_support = 2``."""
    from napkon_string_matching_amd import grid

    for seed in seeds:
        words, rounds = grid.truss_of_hits(one_list(random_graph(seed, nodes, edges)), nodes, 2)
        if rounds >= want_rounds:
            return seed, rounds, int((words[0] >= 0).sum())
    return None


# random_graph(seed, nodes, edges): at min_support = 2 it peels in `rounds` rounds and keeps `alive` edges
CASCADE = dict(seed=11, nodes=24, edges=90, rounds=8, alive=12)


def seeded_lists(seed, density=1.0):
    """Three cohorts pairwise plus one self-join list over the whole node space: five distinct scores, duplicates, both
    orientations, self-loops and NaN scores.  Returns ``(lists, nodes)``, lists as ``(Hits, left_base, right_base)``."""
    rng = np.random.RandomState(seed)
    sizes = [int(v) for v in rng.randint(9, 30, 3)]
    bases = np.r_[0, np.cumsum(sizes)].tolist()
    nodes = bases[-1]
    lists = []
    for a, b in ((0, 1), (0, 2), (1, 2)):
        n = int(density * rng.randint(60, 160))
        i, j = rng.randint(0, sizes[a], n), rng.randint(0, sizes[b], n)
        lists.append([rng.choice(SCORES, n), i, j, bases[a], bases[b]])
    n = int(density * rng.randint(80, 200))
    i, j = rng.randint(0, nodes, n), rng.randint(0, nodes, n)
    i[:5] = j[:5]  # self-loops
    lists.append([rng.choice(SCORES, n), i, j, 0, 0])
    out = []
    for score, i, j, lb, rb in lists:
        dup = rng.randint(0, len(score), max(3, len(score) // 10))  # duplicates (with another score, maybe)
        score = np.r_[score, rng.choice(SCORES, len(dup))]
        i, j = np.r_[i, i[dup]], np.r_[j, j[dup]]
        if lb == rb:  # the other orientation of some
            back = rng.randint(0, len(score), len(score) // 3)
            score, i, j = np.r_[score, score[back]], np.r_[i, j[back]], np.r_[j, i[back]]
        score = score.astype(np.float64)
        score[rng.randint(0, len(score), 4)] = np.nan
        order = rng.permutation(len(score))
        from napkon_string_matching_amd import grid

        out.append((grid.Hits(score[order], i[order].astype(np.int32), j[order].astype(np.int32)), lb, rb))
    return out, nodes


def seam_graph(n_a, n_b, n_c, seed=0):
    """Nodes u and v, sets A (neighbours of u only), B (neighbours of v only) and C (neighbours of both); the edge (u, v).
    C holds the smallest and the largest node id.  Returns ``(lists, nodes, want)``: one self-join list with shuffled
    records, some of them twice and in either orientation, and the words its construction dictates: ``|C|`` on (u, v), 1 on
    every edge into C, 0 on every edge into A or B."""
    order = (["c"] if n_c else []) + ["u", "v"] + ["a"] * n_a + ["b"] * n_b + ["c"] * max(0, n_c - 1)
    ids = {role: [k for k, r in enumerate(order) if r == role] for role in "uvabc"}
    u, v = ids["u"][0], ids["v"][0]
    edges = [(u, v, n_c)] + [(u, w, 0) for w in ids["a"]] + [(v, w, 0) for w in ids["b"]]
    edges += [(x, w, 1) for w in ids["c"] for x in (u, v)]
    rng = np.random.RandomState(seed + 7 * n_a + 11 * n_b + 13 * n_c)
    extra = [edges[k] for k in rng.randint(0, len(edges), min(len(edges), 9))]
    recs = [(b, a, w) if rng.randint(2) else (a, b, w) for a, b, w in edges + extra]
    recs = [recs[k] for k in rng.permutation(len(recs))]
    if n_c >= 2:
        assert min(ids["c"]) == 0 and max(ids["c"]) == len(order) - 1
    return one_list([(a, b) for a, b, _ in recs]), len(order), np.array([w for _, _, w in recs], dtype=np.int32)


def routing_constants():
    """The ``NSM_SUPPORT_*`` routing constants of csrc/support.hip, by name."""
    text = (Path(__file__).resolve().parents[2] / "napkon-string-matching_amd" / "csrc" / "support.hip").read_text()
    return {name: int(value) for name, value in re.findall(r"^#define (NSM_SUPPORT_\w+) (\d+)$", text, flags=re.M)}


SEAM_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129)


def seam_sizes():
    return sorted(set(SEAM_SIZES) | {max(0, c + d) for c in routing_constants().values() for d in (-1, 0, 1)})


def seam_cases(size):
    """The (|A|, |B|, |C|) of one size: short against long and long against short; the shorter row of (u, v) -- |A| + |C| + 1
    or |B| + |C| + 1 arcs -- at size + 1, size + 2, 2 and exactly ``size``."""
    cases = [(size, 0, size), (0, size, 1), (1, 2, size), (size, size, 0), (2, size, size)]
    if size >= 1:
        cases += [(0, 5, size - 1), (5, 0, size - 1)]
    return cases


def final_triangles_x3(lists, nodes, words):
    """Three times the triangles of the final graph: the sum of the final supports over the alive DISTINCT edges."""
    seen = {}
    for (hits, lb, rb), word in zip(lists, words):
        for i, j, w in zip(hits.i.tolist(), hits.j.tolist(), word.tolist()):
            if w >= 0:
                seen[(min(lb + i, rb + j), max(lb + i, rb + j))] = w
    return sum(seen.values()), len(seen)


def edge_counts(lists, nodes, min_score):
    """(edge records, distinct edges)."""
    records, distinct = 0, set()
    for hits, lb, rb in lists:
        for s, i, j in zip(hits.score.tolist(), hits.i.tolist(), hits.j.tolist()):
            if s >= min_score and lb + i != rb + j:
                records += 1
                distinct.add((min(lb + i, rb + j), max(lb + i, rb + j)))
    return records, len(distinct)


def scheme(lists, nodes, min_support, min_score=0.0, dedupe=True, kill_both=True):
    """The device scheme restated in numpy: two packed arcs per edge record, one sort, equal neighbours dropped, a row
    offset per node, per distinct edge (arc with u < v) the shorter row walked and the longer one binary-searched with dead
    arcs skipped, a synchronous kill of both arcs, and a lookup per record.  Returns ``(words per list, rounds)``.
    ``dedupe=False`` / ``kill_both=False`` are the two mutants of the scheme."""
    bits = 1
    while (1 << bits) < nodes:
        bits += 1
    mask = (1 << bits) - 1
    ends = []
    for hits, lb, rb in lists:
        u, v = hits.i.astype(np.int64) + lb, hits.j.astype(np.int64) + rb
        edge = (hits.score >= min_score) & (u != v)
        ends.append((u, v, edge))
    arcs = np.concatenate([np.r_[(u[e] << bits) | v[e], (v[e] << bits) | u[e]] for u, v, e in ends] + [np.zeros(0, np.int64)])
    arcs = np.sort(arcs)
    if dedupe and len(arcs):
        arcs = arcs[np.r_[True, arcs[1:] != arcs[:-1]]]
    off = np.searchsorted(arcs, np.arange(nodes + 1, dtype=np.int64) << bits)
    src, dst = arcs >> bits, arcs & mask
    alive = np.ones(len(arcs), dtype=bool)
    sup = np.zeros(len(arcs), dtype=np.int32)
    rounds = 0
    while True:
        rounds += 1
        for t in np.flatnonzero((src < dst) & alive).tolist():
            u, v = int(src[t]), int(dst[t])
            (a0, a1), (b0, b1), b = (off[u], off[u + 1]), (off[v], off[v + 1]), v
            if a1 - a0 > b1 - b0:
                (a0, a1), (b0, b1), b = (b0, b1), (a0, a1), u
            count = 0
            for p in range(a0, a1):
                if not alive[p]:
                    continue
                want = (b << bits) | int(dst[p])
                at = b0 + int(np.searchsorted(arcs[b0:b1], want))
                if at < b1 and arcs[at] == want and alive[at]:
                    count += 1
            sup[t] = count
        drop = np.flatnonzero((src < dst) & alive & (sup < min_support)) if min_support else np.zeros(0, int)
        if len(drop) == 0:
            break
        if rounds > len(arcs):
            raise AssertionError("the scheme does not end")
        for t in drop.tolist():
            alive[t] = False
            if kill_both:
                alive[int(np.searchsorted(arcs, (int(dst[t]) << bits) | int(src[t])))] = False
    words = []
    for u, v, edge in ends:
        out = np.full(len(u), -1, dtype=np.int32)
        a, b = np.minimum(u, v), np.maximum(u, v)
        at = np.searchsorted(arcs, (a[edge] << bits) | b[edge])
        out[edge] = np.where(alive[at], sup[at], -2)
        words.append(out)
    return words, rounds
