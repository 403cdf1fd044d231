"""GPU parity of the grouped top-k queries (nsm_indel_raw_top_k_grouped, nsm_jaccard_raw_top_k_grouped and their faces).

Every expectation is the definition (tests/support/grouped.py: group_cut) applied to the oracle's FULL grid: per left item
the best record of every group of right rows, of those the first k in (score descending, j ascending), all in canonical
order.  Records and scores must be identical (bit-exact doubles, no tolerance).
"""
import random

import numpy as np
import pytest

from support.grouped import GROUP_PATTERNS, draw_groups, group_cut

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _rand_codes(rng, n, stride, lmin, lmax, alpha):
    codes = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    for r in range(n):
        lens[r] = rng.randint(lmin, lmax)
        codes[r, : lens[r]] = [rng.randrange(alpha) for _ in range(lens[r])]
    return codes, lens


@pytest.mark.parametrize("stride,lmin,lmax,alpha", [
    (64, 0, 64, 4), (64, 0, 64, 37), (128, 65, 128, 4), (128, 0, 128, 37), (512, 65, 512, 37), (512, 300, 512, 4)])
def test_indel_grouped_random(dev, stride, lmin, lmax, alpha):
    import torch

    from napkon_string_matching_amd import grid, tables
    from oracle import native

    rng = random.Random(stride * 1000 + lmax + alpha)
    n, m = (70, 150) if stride == 64 else (40, 90)
    lc, ll = _rand_codes(rng, n, stride, lmin, lmax, alpha)
    rc, rl = _rand_codes(rng, m, stride, lmin, lmax, alpha)
    lt = tables.StrTable.from_codes(lc, ll, alpha, dev)
    rt = tables.StrTable.from_codes(rc, rl, alpha, dev)
    full = native.indel_raw(native.csr_from_codes(lc, ll), native.csr_from_codes(rc, rl), -1.0, cap=n * m + 1)
    for pattern in GROUP_PATTERNS:
        groups = draw_groups(rng, m, pattern)
        on_device = torch.from_numpy(groups).to(dev)
        for thr in (-1.0, 0.0, 0.3, 0.5, 0.8, 1.0, 1.5):
            grid_hits = [h for h in full if h[0] >= thr]
            for k in (1, 3, 64, m, m + 5):
                want = group_cut(grid_hits, groups.tolist(), k)
                for prune in (True, False):
                    st = []
                    got = grid.indel_raw_top_k(lt, rt, k, thr, prune=prune, stats=st, groups=on_device if prune else groups)
                    assert got.as_tuples() == want, (pattern, thr, k, prune)
                    if not prune:
                        assert st[3] == n * m
                if pattern == "identity":
                    assert grid.indel_raw_top_k(lt, rt, k, thr).as_tuples() == want, (thr, k)
                if pattern == "one":
                    assert len(want) <= n


def _rand_padded(rng, n, width, vocab, kmax, allow_empty):
    ids = np.full((n, width), -1, dtype=np.int32)
    for r in range(n):
        c = rng.randint(0 if allow_empty else 1, kmax)
        ids[r, :c] = rng.sample(range(vocab), c)
    return ids


@pytest.mark.parametrize("width,vocab", [(16, 30), (32, 80), (64, 200)])
@pytest.mark.parametrize("empty_side", ["left", "right"])
def test_jaccard_grouped_random(dev, width, vocab, empty_side):
    from napkon_string_matching_amd import grid, tables
    from oracle import native

    rng = random.Random(width * 7 + len(empty_side))
    n, m = 80, 160
    left = _rand_padded(rng, n, width, vocab, width, empty_side == "left")
    right = _rand_padded(rng, m, width, vocab, width, empty_side == "right")
    lt = tables.SetTable.from_padded(left, "left", dev, width=width)
    rt = tables.SetTable.from_padded(right, "right", dev, width=width)
    full = native.jaccard_raw(native.csr_from_padded(left), native.csr_from_padded(right), -1.0, cap=n * m + 1)
    for pattern in GROUP_PATTERNS:
        groups = draw_groups(rng, m, pattern)
        for thr in (-1.0, 0.0, 0.1, 0.3, 0.5, 1.0, 1.5):
            grid_hits = [h for h in full if h[0] >= thr]
            for k in (1, 3, 64, m + 5):
                want = group_cut(grid_hits, groups.tolist(), k)
                for prune in (True, False):
                    st = []
                    got = grid.jaccard_raw_top_k(lt, rt, k, thr, prune=prune, stats=st, groups=groups)
                    assert got.as_tuples() == want, (pattern, thr, k, prune)
                if pattern == "identity":
                    assert grid.jaccard_raw_top_k(lt, rt, k, thr).as_tuples() == want, (thr, k)


def test_ties_inside_and_across_groups_go_to_the_smaller_j(dev):
    """Seven distinct right strings, 120 rows: equal scores abound, also across length classes (2 LCS of 2 + 4 and 4 of
    4 + 8 are the same double).  Groups by j % 5 put equal rows both into one group and into different groups, so the
    representatives and the k-th place are decided by j alone."""
    from napkon_string_matching_amd import grid, tables
    from oracle import native

    rng = random.Random(17)
    left = ["aaaa", "aab", "abab"]
    right = [rng.choice(["aa", "aaaaaaaa", "aaaa", "bb", "ab", "abababab", "aabb"]) for _ in range(120)]
    lt, rt = tables.encode_strings(left, right, dev)
    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    full = native.indel_raw(cp(left), cp(right), -1.0, cap=len(left) * len(right) + 1)
    for groups in ([j % 5 for j in range(120)], [j // 3 for j in range(120)], [rng.randrange(40) for _ in range(120)]):
        # the premise: some group holds two rows of equal score, and two groups' best rows score the same
        by_group = {}
        for s, i, j in full:
            if i == 0:
                by_group.setdefault(groups[j], []).append(s)
        assert any(sorted(v)[-1] == sorted(v)[-2] for v in by_group.values() if len(v) > 1)
        assert len({max(v) for v in by_group.values()}) < len(by_group)
        for k in (1, 2, 5, 17, 40):
            for thr in (0.0, 0.5):
                want = group_cut([h for h in full if h[0] >= thr], groups, k)
                for prune in (True, False):
                    got = grid.indel_raw_top_k(lt, rt, k, thr, prune=prune, groups=np.array(groups, dtype=np.int32))
                    assert got.as_tuples() == want, (k, thr, prune)


def test_replacement_inside_a_full_list(dev):
    """All right rows share the left row's length class and are visited in table order; the weaker spelling of a group
    comes first.  With k = 3 the list is full after j = 2 (worst: group A).  j = 3 improves group B's record, which is NOT
    the worst; j = 4 improves group A's, which IS the worst (the floor moves to C); j = 5 ties with the worst from a
    new group and loses on j; j = 6 evicts C; j = 7 brings C back with a better row."""
    from napkon_string_matching_amd import grid, tables
    from oracle import native

    left = ["abcdefgh", "abcdxxxx"]
    right = ["abcdxxxx", "abcdexxx", "abcdefxx", "abcdefgx", "abcdefgh", "abcdefxy", "abcdefgy", "abcdefgh"]
    groups = ["A", "B", "C", "B", "A", "D", "D", "C"]
    gid = [ord(g) for g in groups]
    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    for pad in (0, 100):  # (with 100 more rows in front, in groups of their own, the story spans two passes of 64 lanes)
        r = ["zzzzzzzq"] * pad + right
        g = list(range(1000, 1000 + pad)) + gid
        lt, rt = tables.encode_strings(left, r, dev)
        full = native.indel_raw(cp(left), cp(r), -1.0, cap=len(left) * len(r) + 1)
        for k in (1, 2, 3, 4, 5):
            for thr in (0.0, 0.6):
                want = group_cut([h for h in full if h[0] >= thr], g, k)
                for prune in (True, False):
                    got = grid.indel_raw_top_k(lt, rt, k, thr, prune=prune, groups=np.array(g, dtype=np.int32))
                    assert got.as_tuples() == want, (pad, k, thr, prune)
        if pad == 0:
            got = grid.indel_raw_top_k(lt, rt, 3, 0.0, groups=np.array(g, dtype=np.int32)).as_tuples()
            assert [h for h in got if h[1] == 0] == [(1.0, 0, 4), (1.0, 0, 7), (0.875, 0, 3)]


def test_public_faces_with_wide_items_and_string_groups(dev):
    from napkon_string_matching_amd.compare.score_functions import fuzzy_match, intersection_vs_union
    from oracle import score_functions as osf

    rng = random.Random(5)
    words = ["alpha", "beta", "gamma", "delta", "omega", "kappa"]
    short = lambda: " ".join(rng.choice(words) for _ in range(rng.randint(1, 4)))
    long_s = " ".join(rng.choice(words) for _ in range(100))  # > 512 code units
    exotic = "".join(chr(0x4E00 + c) for c in range(300))  # > 255 distinct code units
    left = [short() for _ in range(5)] + [long_s] + [short() for _ in range(3)]
    right = [short() for _ in range(9)] + [exotic, long_s[:530]] + [short() for _ in range(6)] + [long_s[:520]]
    groups = [f"H{rng.randrange(6)}" for _ in right]
    groups[10] = groups[-1] = groups[2]  # wide and regular spellings share a group
    index = {g: q for q, g in enumerate(dict.fromkeys(groups))}
    gl = [index[g] for g in groups]
    for thr in (0.0, 0.3):
        full = [(osf.fuzzy_match(a, b), i, j) for i, a in enumerate(left) for j, b in enumerate(right)]
        full = [h for h in full if h[0] >= thr]
        for k in (1, 2, 4, 10):
            got = fuzzy_match.top_k(left, right, k, thr, groups=groups)
            assert got.as_tuples() == group_cut(full, gl, k), (thr, k)

    toks = [f"t{q}" for q in range(90)]
    sets_l = [rng.sample(toks[:20], rng.randint(1, 6)) for _ in range(7)] + [toks[:70]]  # > 64 tokens
    sets_r = [rng.sample(toks[:20], rng.randint(1, 6)) for _ in range(12)] + [toks[5:80], toks[:66]]
    groups = [("g", rng.randrange(5)) for _ in sets_r]
    groups[-1] = groups[0]
    index = {g: q for q, g in enumerate(dict.fromkeys(groups))}
    gl = [index[g] for g in groups]
    for thr in (0.0, 0.2):
        full = [(osf.intersection_vs_union(a, b), i, j) for i, a in enumerate(sets_l) for j, b in enumerate(sets_r)]
        full = [h for h in full if h[0] >= thr]
        for k in (1, 3, 20):
            got = intersection_vs_union.top_k(sets_l, sets_r, k, thr, groups=groups)
            assert got.as_tuples() == group_cut(full, gl, k), (thr, k)
    with pytest.raises(ZeroDivisionError):
        intersection_vs_union.top_k(["a", ""], ["", "b"], 1, groups=["x", "x"])


WORDS = ["dialyse", "niere", "herz", "lunge", "fieber", "husten", "impfung", "therapie", "nach", "vor", "bei"]


def _synonym_frame(rng, ids):
    import pandas as pd

    return pd.DataFrame({"Id": ids, "Term": [" ".join(rng.sample(WORDS, rng.randint(1, 4))).title() for _ in ids]})


def _oracle_lists(table, items, thr, limit):
    from oracle import terminology

    ids, terms = list(table["Id"]), list(table["Term"])
    return [terminology.get_matches(ids, terms, it, thr)[:limit] for it in items]


@pytest.mark.parametrize("limit", [1, 3, 50])
def test_mesh_limit_is_one_bounded_query(golden, monkeypatch, limit):
    """limit = 50 with an Id of 100 rows: 50 x 100 rows per term are beyond the kernels' lists, 50 Ids are not."""
    import pandas as pd

    from napkon_string_matching_amd.compare import score_functions
    from napkon_string_matching_amd.terminology.mesh import MeshProvider

    refs = pd.DataFrame(golden("mesh_references.json")["references"])
    rng = random.Random(9)
    ids = [f"D{rng.randrange(3000):04d}" for _ in range(5900)] + ["D9999"] * 100  # one Id with 100 synonym rows
    perm = list(range(6000))
    rng.shuffle(perm)
    syn = _synonym_frame(rng, [ids[q] for q in perm])
    items = [rng.sample(WORDS, rng.randint(1, 4)) for _ in range(8)] + [["Dialyse", "nach", "Entlassung"]]
    for table in (refs, syn):
        provider = MeshProvider(None, synonyms=table)
        assert provider.get_matches_batch(items, 0.1, limit=limit) == _oracle_lists(table, items, 0.1, limit)

    def no_grid(*args, **kwargs):
        raise AssertionError("the threshold grid was used for a bounded query")

    monkeypatch.setattr(score_functions.fuzzy_match, "raw_grid", no_grid)
    provider = MeshProvider(None, synonyms=syn)
    got = provider.get_matches_batch(items, 0.1, limit=limit)
    assert got == _oracle_lists(syn, items, 0.1, limit)
    assert all(len(rows) <= limit and len({r[0] for r in rows}) == len(rows) for rows in got)


def test_mesh_limit_beyond_the_kernels_goes_through_the_grid(dev):
    """More than 4096 distinct Ids and a limit above 4096: the threshold grid is cut; the lists are the same prefix."""
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd.terminology.mesh import MeshProvider

    rng = random.Random(10)
    ids = [f"D{q:05d}" for q in range(4300)] + [f"D{rng.randrange(4300):05d}" for _ in range(200)]
    syn = _synonym_frame(rng, ids)
    items = [rng.sample(WORDS, rng.randint(1, 4)) for _ in range(3)]
    limit = grid.TOP_K_MAX + 100
    got = MeshProvider(None, synonyms=syn).get_matches_batch(items, 0.1, limit=limit)
    assert got == _oracle_lists(syn, items, 0.1, limit)
    assert max(len(rows) for rows in got) > grid.TOP_K_MAX


def test_full_size_c3_groups_of_eight(dev):
    """200k x 200k at threshold 0, groups j // 8: every left row has 25 000 eligible groups, so exactly n k records."""
    from napkon_string_matching_amd import grid, synthetic, tables

    (lc, ll), (rc, rl) = synthetic.c3_corpus()
    alpha = len(synthetic.STRING_ALPHABET)
    lt = tables.StrTable.from_codes(lc, ll, alpha, dev)
    rt = tables.StrTable.from_codes(rc, rl, alpha, dev)
    k = 10
    groups = (np.arange(len(rl)) // 8).astype(np.int32)
    got = grid.indel_raw_top_k(lt, rt, k, 0.0, groups=groups)
    assert len(got) == len(ll) * k
    rng = np.random.default_rng(3)
    sample = np.sort(rng.choice(len(ll), 64, replace=False))
    st = tables.StrTable.from_codes(lc[sample], ll[sample], alpha, dev)
    ref = grid.indel_raw_grid(st, rt, 0.0, prune=False, capacity=64 * len(rl) + 1)
    want = group_cut([(s, int(sample[i]), j) for s, i, j in ref.as_tuples()], groups.tolist(), k)
    mine = set(sample.tolist())
    assert [h for h in got.as_tuples() if h[1] in mine] == want
