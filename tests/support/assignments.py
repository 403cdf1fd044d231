"""Hit lists for the one-to-one assignment (``grid.assign_of_hits`` / ``nsm_assign_hits``, include/nsm_hip_assign.h), a
plain-Python restatement of the parallel round scheme, and the checks both test files share.

Every family is a ``Case``: a canonically ordered ``grid.Hits`` with the id bounds it is assigned under.  Built once per
process (``case(name)``), never modified.  The definition's answer and the round model's figures are cached beside it.

The round model (``rounds_model``) is the scheme of csrc/assign.hip on numpy arrays: per round every live record mins its
rank into both its items, a record that holds both minima is matched, records with a taken item die.  It yields what
``route="rounds"`` must report: ``stats[0]`` = rounds until nothing is live, ``stats[2]`` = all matches."""
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

SEAM_SIZES = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193)  # wave, block, batch, SMALL_SORT_MAX


@dataclass
class Case:
    name: str
    score: np.ndarray
    i: np.ndarray
    j: np.ndarray
    left_ids: int
    right_ids: int

    def __len__(self) -> int:
        return int(self.score.shape[0])

    def hits(self):
        from napkon_string_matching_amd import grid

        return grid.Hits(self.score, self.i, self.j)


def canonical(score, i, j):
    score, i, j = np.asarray(score, np.float64), np.asarray(i, np.int32), np.asarray(j, np.int32)
    order = np.lexsort((j, i, -score))
    return score[order], i[order], j[order]


def _case(name, score, i, j, left_ids=None, right_ids=None) -> Case:
    score, i, j = canonical(score, i, j)
    n = len(score)
    return Case(name, score, i, j, int(left_ids if left_ids is not None else (i.max() + 1 if n else 0)),
                int(right_ids if right_ids is not None else (j.max() + 1 if n else 0)))


# ------------------------------------------------------------------------------------------------------------ families
def _random_sparse(n: int) -> Case:
    rng = np.random.default_rng(1000 + n)
    ids = n // 2 + 3
    return _case(f"sparse_{n}", rng.integers(1, 40, n) / 40.0, rng.integers(0, ids, n), rng.integers(0, ids, n), ids, ids)


def _all_ties() -> Case:
    i, j = np.meshgrid(np.arange(65), np.arange(130), indexing="ij")
    return _case("all_ties_65x130", np.full(i.size, 0.5), i.ravel(), j.ravel())


def _path(m: int, flip: bool) -> Case:
    """2m - 1 records along l0 - r0 - l1 - r1 - ..., scores rising: only the last record is locally dominant."""
    t = np.arange(2 * m - 1)
    i, j = (t + 1) // 2, t // 2
    if flip:
        i, j = j, i
    return _case(f"path_{m}{'_flipped' if flip else ''}", (t + 1) / (2.0 * m), i, j)


def _star(left: int, right: int) -> Case:
    i, j = np.meshgrid(np.arange(left), np.arange(right), indexing="ij")
    rng = np.random.default_rng(left * 7 + right)
    return _case(f"star_{left}x{right}", rng.integers(1, 9, i.size) / 9.0, i.ravel(), j.ravel())


def _duplicated() -> Case:
    base = _random_sparse(700)
    return _case("every_record_twice", np.repeat(base.score, 2), np.repeat(base.i, 2), np.repeat(base.j, 2), base.left_ids,
                 base.right_ids)


def _perfect() -> Case:
    """2049 records, a permutation, distinct scores: every record wins, the resolve loop runs at full length."""
    rng = np.random.default_rng(5)
    n = 2049
    return _case("perfect_2049", (rng.permutation(n) + 1) / float(n + 1), np.arange(n), rng.permutation(n))


def _runs() -> Case:
    """Runs of 64 consecutive records that share ``i``, then runs that share ``j``: one record wins per run."""
    score, i, j = [], [], []
    for g in range(20):  # one score per run, descending: a run's records are consecutive in canonical order
        shared_i = g < 10
        for t in range(64):
            score.append(1.0 - g / 32.0)
            i.append(g if shared_i else 100 + g * 64 + t)
            j.append(g * 64 + t if shared_i else 5000 + g)
    return _case("runs_of_64", score, i, j)


def _gaps(ids: int) -> Case:
    rng = np.random.default_rng(ids)
    n = 900
    left = rng.integers(0, 60, n) * 37
    right = rng.integers(0, 60, n) * 41 + 5
    if ids < 100000:  # the largest id in use is ids - 1
        left[0], right[1] = ids - 1, ids - 1
    return _case(f"gaps_ids_{ids}", rng.integers(1, 30, n) / 30.0, left, right, ids, ids)


def _model_lists() -> Dict[str, Case]:
    """The two 300 x 300 x 20 000 lists of the design's CPU model, drawn as it drew them (one generator, in its order)."""
    rng = np.random.default_rng(1)
    out = {}
    for name, (nl, nr, n, vals) in (("ties5_300x300", (300, 300, 20000, 5)), ("", (70, 229, 6000, 3)),
                                    ("distinct_300x300", (300, 300, 20000, 10 ** 6))):
        i = rng.integers(0, nl, n).astype(np.int32)
        j = rng.integers(0, nr, n).astype(np.int32)
        s = rng.integers(0, vals, n) / vals
        if name:
            out[name] = _case(name, s, i, j, nl, nr)
    return out


def _build() -> Dict[str, Case]:
    cases = [_case("empty", [], [], [], 5, 7), _case("one_record", [0.25], [3], [2], 4, 3)]
    cases += [_random_sparse(n) for n in SEAM_SIZES]
    cases += [_all_ties(), _path(3, False), _path(3, True), _path(40, False), _path(40, True), _star(1, 300), _star(300, 1),
              _duplicated(), _perfect(), _runs(), _gaps(60 * 41 + 5), _gaps(100000)]
    out = {c.name: c for c in cases}
    out.update(_model_lists())
    return out


_CASES: Dict[str, Case] = {}
_ANSWERS: Dict[str, object] = {}
_MODELS: Dict[str, tuple] = {}


def cases() -> Dict[str, Case]:
    if not _CASES:
        _CASES.update(_build())
    return _CASES


NAMES = (["empty", "one_record"] + [f"sparse_{n}" for n in SEAM_SIZES] +
         ["all_ties_65x130", "path_3", "path_3_flipped", "path_40", "path_40_flipped", "star_1x300", "star_300x1",
          "every_record_twice", "perfect_2049", "runs_of_64", f"gaps_ids_{60 * 41 + 5}", "gaps_ids_100000", "ties5_300x300",
          "distinct_300x300"])
MODEL_ROUNDS = {"all_ties_65x130": 65, "path_3": 3, "path_3_flipped": 3, "path_40": 40, "path_40_flipped": 40,
                "ties5_300x300": 20, "distinct_300x300": 8, "perfect_2049": 1, "one_record": 1, "empty": 0}


def case(name: str) -> Case:
    return cases()[name]


# ------------------------------------------------------------------------------------------- definition and round model
def walk(c: Case) -> List[int]:
    """The definition, on ranks: a record is taken iff neither of its items has been taken."""
    left, right, out = set(), set(), []
    for r, (a, b) in enumerate(zip(c.i.tolist(), c.j.tolist())):
        if a not in left and b not in right:
            left.add(a)
            right.add(b)
            out.append(r)
    return out


def rounds_model(c: Case) -> Tuple[List[int], List[int], List[int]]:
    """(matched ranks ascending, live records at the start of every round, ranks matched in the first round)."""
    n = len(c)
    alive = np.arange(n)
    taken_l, taken_r = np.zeros(c.left_ids, bool), np.zeros(c.right_ids, bool)
    out, history, first = [], [], []
    while len(alive):
        history.append(len(alive))
        best_l, best_r = np.full(c.left_ids, n), np.full(c.right_ids, n)
        np.minimum.at(best_l, c.i[alive], alive)
        np.minimum.at(best_r, c.j[alive], alive)
        won = alive[(best_l[c.i[alive]] == alive) & (best_r[c.j[alive]] == alive)]
        if not out:
            first = won.tolist()
        out += won.tolist()
        taken_l[c.i[won]] = True
        taken_r[c.j[won]] = True
        alive = alive[~taken_l[c.i[alive]] & ~taken_r[c.j[alive]]]
    return sorted(out), history, first


def answer(name: str):
    """``grid.assign_of_hits`` of the case, cached."""
    from napkon_string_matching_amd import grid

    if name not in _ANSWERS:
        _ANSWERS[name] = grid.assign_of_hits(case(name).hits())
    return _ANSWERS[name]


def model(name: str):
    if name not in _MODELS:
        _MODELS[name] = rounds_model(case(name))
    return _MODELS[name]


def same(got, want, what: str) -> None:
    """Records and doubles equal, bit for bit."""
    assert len(got) == len(want), f"{what}: {len(got)} records, expected {len(want)}"
    assert np.array_equal(got.i, want.i) and np.array_equal(got.j, want.j), f"{what}: pairs differ"
    assert np.array_equal(np.asarray(got.score).view(np.int64), np.asarray(want.score).view(np.int64)), f"{what}: scores differ"


def records_bytes(c: Case) -> np.ndarray:
    """The case as the ``nsm_hit`` records the C entry reads: ``[n, 2]`` float64 whose second column holds (i, j)."""
    host = np.zeros((len(c), 2), dtype=np.float64)
    host[:, 0] = c.score
    ij = host.view(np.int32).reshape(len(c), 4)
    ij[:, 2], ij[:, 3] = c.i, c.j
    return host


def hits_of_records(host: np.ndarray):
    """Device records copied to the host, in canonical order."""
    from napkon_string_matching_amd import grid

    n = host.shape[0]
    ij = np.ascontiguousarray(host).view(np.int32).reshape(n, 4)
    score, i, j = canonical(host[:, 0], ij[:, 2], ij[:, 3])
    return grid.Hits(score, i, j)
