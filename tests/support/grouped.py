"""The definition of the grouped top-k query, on tuples, and the group patterns the tests and the fuzzer draw from."""
import numpy as np


def group_cut(hits, groups, k):
    """hits: (score, i, j) tuples of a threshold grid; groups[j] = the group of right item j.  Per left item i: the best
    record of every group (first in (score descending, j ascending)), of those the first k; in canonical order."""
    rows = {}
    for s, i, j in hits:
        rows.setdefault(i, []).append((s, i, j))
    kept = []
    for lst in rows.values():
        seen, reps = set(), []
        for r in sorted(lst, key=lambda t: (-t[0], t[2])):
            if groups[r[2]] not in seen:
                seen.add(groups[r[2]])
                reps.append(r)
        kept += reps[:k]
    return sorted(kept, key=lambda t: (-t[0], t[1], t[2]))


GROUP_PATTERNS = ("identity", "one", "three", "quarter", "half_in_one")


def draw_groups(rng, m, pattern):
    """int32 group ids of m right rows (rng: random.Random): every row its own group, one group, 3 groups, m / 4 random
    groups, or half of the rows in one group and the rest on their own.  Ids are arbitrary values, negative ones included."""
    if pattern == "identity":
        g = list(range(m))
    elif pattern == "one":
        g = [-7] * m
    elif pattern == "three":
        g = [rng.choice((-1, 0, 2 ** 31 - 1)) for _ in range(m)]
    elif pattern == "quarter":
        g = [rng.randrange(max(1, m // 4)) * 3 - 5 for _ in range(m)]
    elif pattern == "half_in_one":
        g = [m + 1 if rng.random() < 0.5 else j for j in range(m)]
    else:
        raise ValueError(pattern)
    return np.array(g, dtype=np.int32)
