"""GPU parity of the per-item top-k of the LEVELS grids (nsm_indel_levels_top_k, nsm_jaccard_levels_top_k) and of
``ComparableData.compare(..., top_k=)``.

Every kernel expectation is the definition: the C oracle's levels threshold grid (``oracle.native.levels``) without the
banned pairs, cut per left item after rank k in the order (score descending, j ascending), returned in canonical order.
Records and scores must be identical (bit-exact doubles), with pruning on and off.  The API expectation is ``compare()``
without ``top_k``, cut per left item.
"""
import random

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

THRESHOLDS = (-1.0, 0.0, 0.3, 0.5, 0.8, 1.0, 1.5)


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def rank_cut(hits, k, banned=frozenset()):
    """(score, i, j) tuples of a threshold grid -> the top-k records of every i without the banned pairs, canonical order."""
    rows = {}
    for s, i, j in hits:
        if (i, j) not in banned:
            rows.setdefault(i, []).append((s, i, j))
    kept = [r for lst in rows.values() for r in sorted(lst, key=lambda t: (-t[0], t[2]))[:k]]
    return sorted(kept, key=lambda t: (-t[0], t[1], t[2]))


def _random_cats(rng, n, mode):
    """Category masks with empty ones among them (the "both empty" rule of mode 2)."""
    return np.array([0 if rng.random() < 0.2 else (1 << rng.randrange(5)) | (1 << rng.randrange(5)) for _ in range(n)],
                    dtype=np.uint64)


def _banned_for(rng, full, n):
    """Pairs that would otherwise be in the top k (every row's best), and every pair of row 0."""
    best = {}
    for s, i, j in full:
        if i not in best or (-s, j) < (-best[i][0], best[i][1]):
            best[i] = (s, j)
    banned = {(i, j) for i, (s, j) in best.items() if rng.random() < 0.6}
    banned |= {(0, j) for s, i, j in full if i == 0}
    return banned


def _as_arrays(banned):
    if not banned:
        return None
    arr = np.array(sorted(banned), dtype=np.int64)
    return arr[:, 0], arr[:, 1]


# ------------------------------------------------------------------------------------------------------------- fuzzy
def _fuzzy_items(rng, n, lmin, lmax, alpha):
    items = []
    for k in range(n):
        depth = 1 if k % 4 == 0 else rng.randint(1, 6)
        items.append([[rng.randrange(alpha) for _ in range(rng.randint(lmin, lmax))] for _ in range(depth)])
    return items


def _encode_fuzzy(items, stride):
    rows = [lv for it in items for lv in it]
    codes = np.zeros((max(1, len(rows)), stride), dtype=np.uint8)
    lens = np.zeros(max(1, len(rows)), dtype=np.int32)
    for r, lv in enumerate(rows):
        codes[r, : len(lv)] = lv
        lens[r] = len(lv)
    nlev = np.array([len(it) for it in items], dtype=np.int32)
    first = np.concatenate([[0], np.cumsum(nlev)[:-1]]).astype(np.int32)
    return codes[: len(rows)], lens[: len(rows)], first, nlev


def _fuzzy_case(dev, seed, n, m, stride, lmin, lmax, alpha, cat_mode=0, partition=False):
    from napkon_string_matching_amd import tables
    from oracle import native

    rng = random.Random(seed)
    left = _fuzzy_items(rng, n, lmin, lmax, alpha)
    right = _fuzzy_items(rng, m, lmin, lmax, alpha)
    for k in range(4, m, 5):  # duplicated right items: equal scores, only j decides
        right[k] = [list(lv) for lv in right[rng.randrange(m)]]
    cl = cr = None
    if cat_mode:
        cl, cr = _random_cats(rng, n, cat_mode), _random_cats(rng, m, cat_mode)
    li, ls, ri, rs = tables.encode_level_codes(_encode_fuzzy(left, stride), _encode_fuzzy(right, stride), alpha, dev, cl, cr,
                                               cat_mode, partition=partition)
    full = native.levels(True, left, right, -1.0, cl, cr, cat_mode, cap=n * m + 1)
    return (li, ls, ri, rs), full, rng


@pytest.mark.parametrize("stride,lmin,lmax", [(64, 0, 64), (128, 30, 128), (256, 100, 256), (512, 200, 512)])
@pytest.mark.parametrize("alpha", [4, 37])
def test_indel_levels_top_k_random(dev, stride, lmin, lmax, alpha):
    from napkon_string_matching_amd import grid

    n, m = (40, 90) if stride <= 128 else (24, 50)
    tabs, full, _ = _fuzzy_case(dev, stride * 100 + alpha, n, m, stride, lmin, lmax, alpha)
    assert tabs[1].stride == stride
    for thr in THRESHOLDS:
        grid_hits = [h for h in full if h[0] >= thr]
        for k in (1, 3, 7, m, m + 5):
            want = rank_cut(grid_hits, k)
            for prune in (True, False):
                st = []
                got = grid.indel_levels_top_k(*tabs, k, thr, prune=prune, stats=st)
                assert got.as_tuples() == want, (thr, k, prune)
                if not prune:
                    assert st[3] == n * m


def test_indel_levels_top_k_largest_lds(dev):
    """Stride 512 with 255 symbols: the largest match-mask table plus text image the Indel kernel asks for (51 KB)."""
    from napkon_string_matching_amd import grid

    n, m = 12, 40
    tabs, full, _ = _fuzzy_case(dev, 4242, n, m, 512, 400, 512, 255)
    assert tabs[1].stride == 512 and tabs[1].alphabet == 255
    for thr in (0.0, 0.3):
        grid_hits = [h for h in full if h[0] >= thr]
        for k in (1, 7, m):
            for prune in (True, False):
                assert grid.indel_levels_top_k(*tabs, k, thr, prune=prune).as_tuples() == rank_cut(grid_hits, k), (thr, k)


@pytest.mark.parametrize("cat_mode", [1, 2])
def test_indel_levels_top_k_categories_and_blacklist(dev, cat_mode):
    from napkon_string_matching_amd import grid

    n, m = 40, 80
    tabs, full, rng = _fuzzy_case(dev, 77 + cat_mode, n, m, 128, 0, 100, 11, cat_mode=cat_mode)
    banned = _banned_for(rng, full, n)
    assert any(i == 0 for _, i, _ in full)
    for thr in (-1.0, 0.0, 0.3, 0.5):
        grid_hits = [h for h in full if h[0] >= thr]
        for k in (1, 3, 7, m):
            for ban in (frozenset(), banned):
                want = rank_cut(grid_hits, k, ban)
                for prune in (True, False):
                    st = []
                    got = grid.indel_levels_top_k(*tabs, k, thr, category_mode=cat_mode, prune=prune, banned=_as_arrays(ban),
                                                  stats=st)
                    assert got.as_tuples() == want, (thr, k, prune, len(ban))
                    if ban:
                        assert not any(i == 0 for _, i, _ in got.as_tuples())  # every allowed pair of row 0 is banned
                    if not prune:
                        assert st[3] == len(full)  # the pairs the category predicate allows


def test_indel_levels_top_k_refuses_partition(dev):
    from napkon_string_matching_amd import grid

    tabs, _, _ = _fuzzy_case(dev, 5, 10, 12, 64, 1, 20, 6, cat_mode=1, partition=True)
    assert tabs[0].seg is not None
    with pytest.raises(NotImplementedError):
        grid.indel_levels_top_k(*tabs, 3, 0.2, category_mode=1)


# ----------------------------------------------------------------------------------------------------------- Jaccard
def _set_items(rng, n, width, vocab, dup=False):
    items = []
    for k in range(n):
        cnt = rng.randint(1, width)
        ids = rng.sample(range(vocab), min(cnt, vocab))
        depth = 1 if k % 4 == 0 else rng.randint(1, 6)
        cuts = sorted(rng.randint(1, len(ids)) for _ in range(depth - 1)) + [len(ids)]
        items.append([ids[:c] for c in cuts])
    if dup:
        for k in range(4, n, 5):
            items[k] = [list(lv) for lv in items[rng.randrange(n)]]
    return items


def _jaccard_case(dev, seed, n, m, width, vocab, cat_mode=0, partition=False):
    from napkon_string_matching_amd import tables
    from oracle import native

    rng = random.Random(seed)
    left, right = _set_items(rng, n, width, vocab), _set_items(rng, m, width, vocab, dup=True)
    cl = cr = None
    if cat_mode:
        cl, cr = _random_cats(rng, n, cat_mode), _random_cats(rng, m, cat_mode)
    vocab_t = tables.Vocabulary()
    lt = tables.SetTable.from_levels(left, "left", dev, vocab_t, width=width, categories=cl, category_mode=cat_mode,
                                     partition=partition, index=False)
    rt = tables.SetTable.from_levels(right, "right", dev, vocab_t, width=width, categories=cr, category_mode=cat_mode,
                                     partition=partition, index=False)
    full = native.levels(False, left, right, -1.0, cl, cr, cat_mode, cap=n * m + 1)
    return (lt, rt), full, rng


@pytest.mark.parametrize("width,vocab", [(16, 20), (32, 40), (64, 90)])
def test_jaccard_levels_top_k_random(dev, width, vocab):
    from napkon_string_matching_amd import grid

    n, m = 40, 90
    (lt, rt), full, _ = _jaccard_case(dev, width, n, m, width, vocab)
    assert lt.width == width
    for thr in THRESHOLDS:
        grid_hits = [h for h in full if h[0] >= thr]
        for k in (1, 3, 7, m, m + 5):
            want = rank_cut(grid_hits, k)
            for prune in (True, False):
                st = []
                got = grid.jaccard_levels_top_k(lt, rt, k, thr, prune=prune, stats=st)
                assert got.as_tuples() == want, (thr, k, prune)
                if not prune:
                    assert st[3] == n * m


@pytest.mark.parametrize("cat_mode", [1, 2])
def test_jaccard_levels_top_k_categories_and_blacklist(dev, cat_mode):
    from napkon_string_matching_amd import grid

    n, m = 40, 70
    (lt, rt), full, rng = _jaccard_case(dev, 300 + cat_mode, n, m, 32, 30, cat_mode=cat_mode)
    banned = _banned_for(rng, full, n)
    for thr in (-1.0, 0.0, 0.3, 0.5):
        grid_hits = [h for h in full if h[0] >= thr]
        for k in (1, 3, 7, m):
            for ban in (frozenset(), banned):
                want = rank_cut(grid_hits, k, ban)
                for prune in (True, False):
                    st = []
                    got = grid.jaccard_levels_top_k(lt, rt, k, thr, category_mode=cat_mode, prune=prune,
                                                    banned=_as_arrays(ban), stats=st)
                    assert got.as_tuples() == want, (thr, k, prune, len(ban))
                    if not prune:
                        assert st[3] == len(full)


def test_jaccard_levels_top_k_refuses_partition(dev):
    from napkon_string_matching_amd import grid

    (lt, rt), _, _ = _jaccard_case(dev, 9, 10, 12, 16, 20, cat_mode=1, partition=True)
    assert lt.seg is not None
    with pytest.raises(NotImplementedError):
        grid.jaccard_levels_top_k(lt, rt, 3, 0.2, category_mode=1)


# ------------------------------------------------------------------------------------------------- compare(top_k=)
def cut_comparable(frame: pd.DataFrame, left_id: str, k: int) -> pd.DataFrame:
    """``compare()``'s frame (score descending, label ascending) cut after rank k per left item."""
    rank = frame.assign(_lab=frame.index).sort_values(["MatchScore", "_lab"], ascending=[False, True], kind="mergesort") \
        .groupby(left_id, sort=False).cumcount()
    return frame[(rank < k).reindex(frame.index).to_numpy()]


def _left_id(comp) -> str:
    return comp.left_name + "Identifier"


def _check_top_k(left, right, whitelist, blacklist, kw, ks=(1, 2, 5)):
    plain = left.compare(right, whitelist, blacklist, **kw)
    frame = plain.dataframe()
    for k in ks:
        got = left.compare(right, whitelist, blacklist, top_k=k, **kw).dataframe()
        want = cut_comparable(frame, _left_id(plain), k)
        assert list(got.index) == list(want.index), k
        assert list(got["MatchScore"]) == list(want["MatchScore"]), k  # bit-exact
        pd.testing.assert_frame_equal(got, want)
        assert got.empty or got.groupby(_left_id(plain)).size().max() <= k
    return len(frame)


@pytest.mark.parametrize("score_func", ["intersection_vs_union", "fuzzy_match"])
def test_compare_top_k_pair_grids(golden, score_func):
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    total = 0
    for name, case in golden("pair_grids.json").items():
        left, right = Questionnaire(pd.DataFrame(case["left"])), Questionnaire(pd.DataFrame(case["right"]))
        kw = dict(case.get("compare_kwargs") or case["gen_kwargs"], score_func=score_func)
        try:
            left.compare(right, case["whitelist"], case["blacklist"], **kw)
        except Exception as exc:  # the reference's per-pair errors are raised exactly as without top_k
            with pytest.raises(type(exc)):
                left.compare(right, case["whitelist"], case["blacklist"], top_k=2, **kw)
            continue
        total += _check_top_k(left, right, case["whitelist"], case["blacklist"], kw)
        # threshold 0 and no cache threshold: every allowed pair competes
        kw0 = dict(kw, score_threshold=0.0, cache_threshold=None)
        total += _check_top_k(left, right, case["whitelist"], case["blacklist"], kw0)
    assert total > 100


def _frame(rows):
    return pd.DataFrame(rows, columns=["Identifier", "Variable", "Sheet", "Category", "Term", "Tokens", "Parameter"])


def _odd_cohort(seed, n, words, long_item=False, deep=False, empty=False):
    rng = random.Random(seed)
    rows = []
    for k in range(n):
        toks = [rng.choice(words) for _ in range(rng.randint(1, 6))]
        if long_item and k % 7 == 3:
            # > 64 distinct tokens, and level strings beyond 512 code units (the general kernels' share of the grid)
            toks = [f"longtoken{rng.randrange(400):03d}" for _ in range(80)]
        term = [" ".join(toks[q:q + 2]) for q in range(0, len(toks), 2)]
        if deep and k % 5 == 1:
            term = [[t, "zz" + t] for t in term]  # irregular levels (an entry that is itself a list)
        if empty and k % 9 == 4:
            term = []  # zero levels
        rows.append([f"{seed}-{k}", f"v{k}", "s", [f"c{k % 3}"], term, toks, "p"])
    return _frame(rows)


@pytest.mark.parametrize("score_func", ["intersection_vs_union", "fuzzy_match"])
@pytest.mark.parametrize("shape", ["wide", "irregular", "zero_levels"])
def test_compare_top_k_odd_items(score_func, shape):
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    words = [f"word{q}" for q in range(25)]
    opts = dict(long_item=shape == "wide", deep=shape == "irregular", empty=shape == "zero_levels")
    left = Questionnaire(_odd_cohort(1, 30, words, **opts))
    right = Questionnaire(_odd_cohort(2, 35, words, **opts))
    if shape == "wide":  # the items really leave the fast kernels: the split route and its merge are what is checked
        from napkon_string_matching_amd import wide
        from napkon_string_matching_amd.compare import score_functions as sf

        levels = lambda q: [q.gen_comp_value(t) for t in q.dataframe()["Term"]]
        if score_func == "fuzzy_match":
            ops = lambda q: [[sf.fuzzy_operand(lv) for lv in it] for it in levels(q)]
            assert max(len(op) for it in ops(left) for op in it) > 512
            assert wide.wide_string_items(ops(left), ops(right)) is not None
        else:
            assert wide.wide_set_items(levels(left), levels(right)) is not None
    for cats in (False, True):
        for thr in (0.0, 0.2):
            kw = dict(score_func=score_func, compare_column="Term", left_name="hap", right_name="pop", score_threshold=thr,
                      filter_categories=cats)
            try:
                plain = left.compare(right, None, None, **kw)
            except (IndexError, ZeroDivisionError) as exc:
                with pytest.raises(type(exc)):
                    left.compare(right, None, None, top_k=3, **kw)
                continue
            assert _check_top_k(left, right, None, None, kw, ks=(1, 3)) > 10
            # a blacklist that removes the best pair of every left item (wide items among them): the fast and the general
            # kernels' shares each drop their banned pairs before the per-item cut
            frame = plain.dataframe()
            best = frame.drop_duplicates("HapIdentifier")
            blacklist = {f"b{q}": {"hap": [a], "pop": [b]}
                         for q, (a, b) in enumerate(zip(best["HapIdentifier"], best["PopIdentifier"]))}
            assert len(blacklist) > 5
            if shape == "wide" and thr == 0.0:
                assert any(int(a.split("-")[1]) % 7 == 3 for a in best["HapIdentifier"])
            assert _check_top_k(left, right, None, blacklist, kw, ks=(1, 3)) > 0


def test_compare_top_k_cache(golden, tmp_path):
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    case = golden("pair_grids.json")["rand_40x30_categories"]
    left, right = Questionnaire(pd.DataFrame(case["left"])), Questionnaire(pd.DataFrame(case["right"]))
    kw = dict(case["compare_kwargs"], cache_dir=tmp_path)
    plain = left.compare(right, case["whitelist"], case["blacklist"], **kw)
    assert len(list(tmp_path.iterdir())) == 1
    cut = left.compare(right, case["whitelist"], case["blacklist"], top_k=1, **kw)
    assert len(list(tmp_path.iterdir())) == 2  # its own file, not the plain call's
    assert len(cut) < len(plain)
    again = left.compare(right, case["whitelist"], case["blacklist"], top_k=1, **kw)  # read back from its file
    assert list(again.match_score) == list(cut.match_score)
    assert len(list(tmp_path.iterdir())) == 2
    assert list(left.compare(right, case["whitelist"], case["blacklist"], **kw).match_score) == list(plain.match_score)


def test_matcher_top_k(golden, tmp_path):
    """A ``top_k`` key in the matching config reaches compare() through the Matcher's keyword forwarding, and the result
    file name pattern ignores it."""
    from napkon_string_matching_amd.matcher import RESULTS_FILE_PATTERN, Matcher
    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    case = golden("pair_grids.json")["rand_40x30_categories"]
    left, right = Questionnaire(pd.DataFrame(case["left"])), Questionnaire(pd.DataFrame(case["right"]))
    kw = {key: v for key, v in case["compare_kwargs"].items() if key not in ("left_name", "right_name")}
    kw.update(score_threshold=0.1, cache_threshold=None)
    plain = Matcher(None, {"matching": kw}, questionnaires={"hap": left, "suep": right})
    plain.match_questionnaires()
    cut = Matcher(None, {"matching": dict(kw, top_k=2)}, questionnaires={"hap": left, "suep": right})
    cut.match_questionnaires()
    want = cut_comparable(plain.results["hap vs suep"].dataframe(), "HapIdentifier", 2)
    assert 0 < len(want) < len(plain.results["hap vs suep"])
    pd.testing.assert_frame_equal(cut.results["hap vs suep"].dataframe(), want)
    name = lambda m: RESULTS_FILE_PATTERN.format(**{**m, "score_func": m["score_func"].replace("_", "-")})
    assert name(dict(kw, top_k=2)) == name(kw)


_DIST_WORKER = r'''
import json, os, sys
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {root!r})
import pandas as pd, torch, torch.distributed as dist
from napkon_string_matching_amd.types.questionnaire import Questionnaire
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
torch.cuda.set_device(0)
case = json.load(open({fixture!r}))["rand_40x30_categories"]
left, right = Questionnaire(pd.DataFrame(case["left"])), Questionnaire(pd.DataFrame(case["right"]))
out = {{}}
for func in ("intersection_vs_union", "fuzzy_match"):
    for label, blacklist in (("", case["blacklist"]), ("/no blacklist", None)):
        kw = dict(case["compare_kwargs"], score_func=func, score_threshold=0.2, cache_threshold=None)
        comp = left.compare(right, case["whitelist"], blacklist, top_k=3, **kw)
        out[func + label] = [list(map(int, comp.dataframe().index)), [float(v) for v in comp.match_score]]
json.dump(out, open({out!r} + str(dist.get_rank()), "w"))
dist.destroy_process_group()
'''


def test_sharded_compare_top_k_world2(golden, tmp_path):
    """Two ranks (gloo, sharing this GPU) each select the lists of their block of left items and exchange them on the
    host: the same Comparable as a single process."""
    import json
    import os
    import socket
    import subprocess
    import sys
    from pathlib import Path

    from napkon_string_matching_amd.types.questionnaire import Questionnaire

    root = Path(__file__).resolve().parent.parent
    script = tmp_path / "worker.py"
    script.write_text(_DIST_WORKER.format(pkg=str(root / "napkon-string-matching_amd"), root=str(root),
                                          fixture=str(root / "tests" / "golden" / "pair_grids.json"),
                                          out=str(tmp_path / "out")))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0, out.decode()[-2000:]
    case = golden("pair_grids.json")["rand_40x30_categories"]
    left, right = Questionnaire(pd.DataFrame(case["left"])), Questionnaire(pd.DataFrame(case["right"]))
    for func in ("intersection_vs_union", "fuzzy_match"):
        for label, blacklist in (("", case["blacklist"]), ("/no blacklist", None)):
            kw = dict(case["compare_kwargs"], score_func=func, score_threshold=0.2, cache_threshold=None)
            single = left.compare(right, case["whitelist"], blacklist, top_k=3, **kw)
            want = [list(map(int, single.dataframe().index)), [float(v) for v in single.match_score]]
            assert len(want[0]) > 5
            for rank in range(2):
                got = json.load(open(str(tmp_path / "out") + str(rank)))
                assert got[func + label] == want, (func, label, rank)


def test_term_full_size_top_k(dev):
    """The reference's default configuration at 20k x 20k: at 0.5 the threshold grid plus a per-item cut; at 0 (a grid of
    4e8 records) exactly N k records in canonical order, sampled items checked against the oracle."""
    from napkon_string_matching_amd import grid, synthetic, tables
    from napkon_string_matching_amd.compare import score_functions as sf
    from oracle import native

    n = m = 20_000
    left_items = synthetic.term_cohort(n, 1234)
    right_items = synthetic.term_cohort(m, 5678, plant_from=left_items)
    lops = [[sf.fuzzy_operand(lv) for lv in it] for it in synthetic.term_levels(left_items)]
    rops = [[sf.fuzzy_operand(lv) for lv in it] for it in synthetic.term_levels(right_items)]
    tabs = tables.encode_level_strings(lops, rops, dev, partition=False)
    k = 10
    full = grid.indel_levels_grid(*tabs, 0.5)
    want = grid.select_top_k(full, k)
    got = grid.indel_levels_top_k(*tabs, k, 0.5)
    assert got.as_tuples() == want.as_tuples() and len(want) > n // 10

    st = []
    got0 = grid.indel_levels_top_k(*tabs, k, 0.0, stats=st)
    assert len(got0) == n * k
    assert np.all(np.bincount(got0.i, minlength=n) == k)
    key = list(zip((-got0.score).tolist(), got0.i.tolist(), got0.j.tolist()))
    assert key == sorted(key)
    cps = lambda items: [[[ord(ch) for ch in s] for s in it] for it in items]
    rng = random.Random(5)
    rows = rng.sample(range(n), 3)
    right_cps = cps(rops)
    for i in rows:
        exact = native.levels(True, cps([lops[i]]), right_cps, 0.0, cap=m + 1)
        want_i = [(s, i, j) for s, _, j in rank_cut(exact, k)]
        got_i = [t for t in got0.as_tuples() if t[1] == i]
        assert got_i == sorted(want_i, key=lambda t: (-t[0], t[2])), i
    assert st[0] == n * m and st[3] < st[0]
