"""Listed pairs on the GPU: ``nsm_*_pairs`` (csrc/pairs.hip) against the oracle's full grid at threshold 0.0 picked through
``grid.lookup_pairs`` -- bit for bit, ``-1.0`` exactly where the ABI says so, the caller's order kept, ``i`` / ``j`` untouched
-- and the host faces ``plugin.pairs`` / ``ComparableData.score_pairs`` against the per-pair calls they replace.

The grids are those of tests/support/threshold_probes.py (the twelve plain ones: every stride, every RAW width) and the seam
cases of tests/support/pairs_cases.py; tests/test_cpu_pairs.py checks both through the oracle alone."""
import random

import numpy as np
import pytest

from support import pairs_cases as pc
from support import threshold_probes as tp

pytestmark = pytest.mark.gpu

PLAIN = tp.RAW_INDEL + tp.RAW_JACCARD + ["levels_indel_one_word"] + [f"levels_indel_multi_word_{s}" for s in (128, 256, 512)] + \
    ["levels_jaccard"]


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ tables
class Encoded:
    """The tables of one grid (levels: unpartitioned) over the items ``keep_l`` x ``keep_r``, reporting the items' positions
    in the grid as caller ids; ``args`` are the entry's table arguments, ``left`` / ``right`` the tables the ids name."""

    def __init__(self, g, dev, keep_l=None, keep_r=None):
        import torch

        from napkon_string_matching_amd import tables

        keep_l = list(range(len(g.left))) if keep_l is None else list(keep_l)
        keep_r = list(range(len(g.right))) if keep_r is None else list(keep_r)
        left, right = [g.left[k] for k in keep_l], [g.right[k] for k in keep_r]
        if g.raw and g.kind == "indel":
            lt, rt = tables.encode_strings([tp.text(r) for r in left], [tp.text(r) for r in right], dev)
            self.args, self.left, self.right, self.entry = (lt, rt), lt, rt, "nsm_indel_raw_pairs"
            assert lt.stride == g.size
        elif g.raw:
            def padded(rows):
                ids = np.full((len(rows), g.size), -1, dtype=np.int32)
                for r, row in enumerate(rows):
                    ids[r, : len(row)] = row
                return ids

            lt = tables.SetTable.from_padded(padded(left), "left", dev, width=g.size)
            rt = tables.SetTable.from_padded(padded(right), "right", dev, width=g.size)
            self.args, self.left, self.right, self.entry = (lt, rt), lt, rt, "nsm_jaccard_raw_pairs"
        elif g.kind == "indel":
            items = lambda side: [[tp.text(lv) for lv in it] for it in side]
            li, ls, ri, rs = tables.encode_level_strings(items(left), items(right), dev, partition=False)
            self.args, self.left, self.right, self.entry = (li, ls, ri, rs), li, ri, "nsm_indel_levels_pairs"
            assert ls.stride == g.size and li.seg is None
        else:
            vocabulary = tables.Vocabulary()
            lt = tables.SetTable.from_levels(left, "left", dev, vocabulary, width=g.size, partition=False)
            rt = tables.SetTable.from_levels(right, "right", dev, vocabulary, width=g.size, partition=False)
            self.args, self.left, self.right, self.entry = (lt, rt), lt, rt, "nsm_jaccard_levels_pairs"
            assert lt.seg is None and lt.width == g.size
        for table, keep in ((self.left, keep_l), (self.right, keep_r)):  # caller ids: the positions in the grid
            table.orig.copy_(torch.tensor(keep, dtype=torch.int32, device=dev)[table.orig.long()])

    def scores(self, i, j):
        from napkon_string_matching_amd import grid

        return getattr(grid, self.entry[len("nsm_"):])(*self.args, i, j)

    def call(self, records, stream=None):
        """The C entry on a device tensor of records [P][2] float64, in place."""
        import torch

        from napkon_string_matching_amd import _lib, grid

        dev = records.device
        if not hasattr(self, "maps"):  # (built once: a captured call must not synchronise)
            self.maps = grid._row_map(self.left.orig, self.left.n, dev), grid._row_map(self.right.orig, self.right.n, dev)
            self.structs = [t.struct() for t in self.args]
        lmap, rmap = self.maps
        stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        _lib.check(getattr(_lib.load(), self.entry)(*self.structs, lmap.data_ptr(), lmap.numel(), rmap.data_ptr(), rmap.numel(),
                                                    records.data_ptr(), records.shape[0], stream), self.entry)


def _records(i, j, fill=-7.0):
    rec = np.full((len(i), 2), fill, dtype=np.float64)
    ij = rec.view(np.int32).reshape(len(i), 4)
    ij[:, 2], ij[:, 3] = i, j
    return rec


def _all_pairs(g, seed, duplicates=0):
    rng = random.Random(seed)
    pairs = [(i, j) for i in range(len(g.left)) for j in range(len(g.right))]
    rng.shuffle(pairs)
    pairs += [pairs[rng.randrange(len(pairs))] for _ in range(duplicates)]
    return np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64)


def _differences(got, want, i, j):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return [(int(i[k]), int(j[k]), float(got[k]), float(want[k])) for k in bad[:5]], len(bad)


# ------------------------------------------------------------------------------------------- all pairs of the plain grids
@pytest.mark.parametrize("name", PLAIN)
def test_all_pairs_of_a_plain_grid(dev, name):
    """All N x M pairs shuffled, 100 duplicates, ids out of range and negative, and ids without a row (three items dropped
    from each table; the last left item among them, so its id lies beyond the row map): bit equality with the oracle,
    -1.0 exactly for the ids without a row, the records' order and ids untouched."""
    import torch

    from napkon_string_matching_amd import grid

    g = tp.grid(name)
    n_l, n_r = len(g.left), len(g.right)
    drop_l, drop_r = [1, 5, n_l - 1], [0, 7, 100]
    enc = Encoded(g, dev, [k for k in range(n_l) if k not in drop_l], [k for k in range(n_r) if k not in drop_r])
    i, j = _all_pairs(g, 6100 + len(name), duplicates=100)
    odd = [(-1, 0), (2, -1), (n_l, 3), (2, n_r), (n_l + 1000, n_r + 1000), (2**31 - 1, 2), (2, 2**31 - 1), (-(2**31), -(2**31))]
    i = np.concatenate([i, [p[0] for p in odd]]).astype(np.int64)
    j = np.concatenate([j, [p[1] for p in odd]]).astype(np.int64)
    want = grid.lookup_pairs(tp.all_scores(g), i, j)
    gone = np.isin(i, drop_l) | np.isin(j, drop_r)
    assert (want[-len(odd):] == -1.0).all() and (want[: -len(odd)] >= 0.0).all()  # (the oracle scores every real pair)
    want[gone] = -1.0
    rec = _records(i, j)
    records = torch.from_numpy(rec.copy()).to(dev)
    enc.call(records)
    back = records.cpu().numpy()
    assert np.array_equal(back.view(np.int32).reshape(-1, 4)[:, 2:], rec.view(np.int32).reshape(-1, 4)[:, 2:]), "i / j were written"
    diff, n_bad = _differences(back[:, 0], want, i, j)
    assert n_bad == 0, f"{name}: {n_bad} of {len(i)} records differ, first (i, j, got, want): {diff}"
    assert gone.sum() >= 3 * n_r and np.array_equal(back[:, 0][gone], np.full(int(gone.sum()), -1.0))
    # the Python wrapper: the same scores in the caller's order
    assert np.array_equal(enc.scores(i, j), want)


@pytest.mark.parametrize("name", pc.LEVELS_JACCARD_WIDE)
def test_levels_jaccard_at_widths_32_and_64(dev, name):
    g = pc.grid(name)
    enc = Encoded(g, dev)
    i, j = _all_pairs(g, 6200)
    got, want = enc.scores(i, j), grid_lookup(g, i, j)
    diff, n_bad = _differences(got, want, i, j)
    assert n_bad == 0 and (want > 0.0).any(), f"{name}: {n_bad} records differ, first (i, j, got, want): {diff}"


def grid_lookup(g, i, j):
    from napkon_string_matching_amd import grid

    return grid.lookup_pairs(tp.all_scores(g), i, j)


# ---------------------------------------------------------------------------------------------------------------- seams
@pytest.mark.parametrize("name", pc.INDEL_SEAMS + pc.JACCARD_SEAMS + pc.LEVELS_SEAMS)
def test_seam_cases(dev, name):
    """Every pair of a seam grid, then lists of 1, 63, 64, 65 and 259 records (the list repeated where it is shorter)."""
    g = pc.grid(name)
    enc = Encoded(g, dev)
    i, j = _all_pairs(g, 6300)
    want = grid_lookup(g, i, j)
    got = enc.scores(i, j)
    diff, n_bad = _differences(got, want, i, j)
    assert n_bad == 0, f"{name}: {n_bad} of {len(i)} records differ, first (i, j, got, want): {diff}"
    for count in pc.PAIR_COUNTS:
        ci, cj = np.resize(i, count), np.resize(j, count)
        assert np.array_equal(enc.scores(ci, cj), np.resize(want, count)), (name, count)
    if name in pc.INDEL_SEAMS:
        score_of = dict(zip(zip(i.tolist(), j.tolist()), got.tolist()))
        for a, b in g.self_pairs:  # a string against itself: LCS = length
            assert score_of[(a, b)] == (1.0 if g.left[a] else 0.0)
        for a, b, lcs in [g.straddle] + g.runs:
            n = len(g.left[a]) + len(g.right[b])
            assert score_of[(a, b)] == ((1.0 - (n - 2 * lcs) / n) * 100.0) / 100.0


def test_pairs_without_a_score(dev):
    """-1.0 for what the host resolves before a grid launch: two empty sets (RAW), an item without levels, an empty level
    against an empty level; 0.0 for an empty string or set against anything else."""
    import torch

    from napkon_string_matching_amd import grid, tables

    lt = tables.SetTable.from_padded(np.array([[-1, -1], [4, -1]], dtype=np.int32), "left", dev, width=16)
    rt = tables.SetTable.from_padded(np.array([[-1, -1], [4, 5]], dtype=np.int32), "right", dev, width=16)
    assert grid.jaccard_raw_pairs(lt, rt, [0, 0, 1, 1], [0, 1, 0, 1]).tolist() == [-1.0, 0.0, 0.0, 0.5]
    ls, rs = tables.encode_strings(["", "ab"], ["", "abab"], dev)
    assert grid.indel_raw_pairs(ls, rs, [0, 0, 1, 1], [0, 1, 0, 1]).tolist() == [0.0, 0.0, 0.0, ((1.0 - 2 / 6) * 100.0) / 100.0]
    # levels: the tables are encoded with levels everywhere, then one item per side loses its levels / its ids in place
    # (the columns are the caller's)
    items = [[[1, 2]], [[1, 2], [1, 2, 3]], [[7]]]
    vocabulary = tables.Vocabulary()
    lt = tables.SetTable.from_levels(items, "left", dev, vocabulary, width=16, partition=False)
    rt = tables.SetTable.from_levels(items, "right", dev, vocabulary, width=16, partition=False)
    row = lambda t, k: int((t.orig == k).nonzero()[0, 0])
    before = grid.jaccard_levels_pairs(lt, rt, [0, 1, 2, 2], [0, 1, 2, 0])
    assert before.tolist() == [0.5, 0.5 * 1.0 + 0.25 * 1.0, 0.5, 0.0]
    for t in (lt, rt):
        t.nlev[row(t, 1)] = 0       # item 1: no levels
        t.plen[row(t, 2)] = 0       # item 2: its one level is empty
        t.cnt[row(t, 2)] = 0
    torch.cuda.synchronize(dev)
    got = grid.jaccard_levels_pairs(lt, rt, [0, 1, 0, 1, 2, 2, 0], [0, 1, 1, 0, 2, 0, 2])
    assert got.tolist() == [0.5, -1.0, -1.0, -1.0, -1.0, 0.0, 0.0]
    strings = [["ab"], ["ab", "abc"], []]
    li, lstr, ri, rstr = tables.encode_level_strings(strings, strings, dev, partition=False)
    got = grid.indel_levels_pairs(li, lstr, ri, rstr, [0, 1, 2, 2, 0, 1], [0, 1, 2, 0, 2, 0])
    part = ((1.0 - 1 / 5) * 100.0) / 100.0  # "abc" against "ab", at both steps
    assert got.tolist() == [0.5, 0.75, -1.0, -1.0, -1.0, part * 0.5 + part * 0.25]


def test_partitioned_tables_are_refused(dev):
    from napkon_string_matching_amd import grid, tables

    g = tp.grid("levels_jaccard-cat1_partition")
    vocabulary = tables.Vocabulary()
    lt = tables.SetTable.from_levels(g.left, "left", dev, vocabulary, width=g.size, categories=g.cat_l, category_mode=g.mode)
    rt = tables.SetTable.from_levels(g.right, "right", dev, vocabulary, width=g.size, categories=g.cat_r, category_mode=g.mode)
    assert lt.seg is not None
    with pytest.raises(NotImplementedError, match="partitioned tables are not supported"):
        grid.jaccard_levels_pairs(lt, rt, [0], [0])


# ------------------------------------------------------------------------------------------------- hits handed back in
@pytest.mark.parametrize("name", ["raw_indel_64", "levels_jaccard"])
def test_a_grids_hits_handed_back_in(dev, name):
    """The rescoring workflow: the device records of ``nsm_*_grid`` at a mid threshold go to the pairs entry as they are
    and come back unchanged, bit for bit -- also after their scores were wiped."""
    import torch

    from napkon_string_matching_amd import _lib, grid

    g = tp.grid(name)
    enc = Encoded(g, dev)
    lib = _lib.load()
    structs = [t.struct() for t in enc.args]
    if g.raw:
        launch = lambda buf, stream: lib.nsm_indel_raw_grid(*structs, 0.5, _lib.FLAG_PRUNE, buf.records.data_ptr(), buf.capacity,
                                                            buf.count.data_ptr(), stream)
        pending = grid.run_grid(launch, dev, g.pairs + 1, "nsm_indel_raw_grid", defer=True)
    else:
        pending = grid.jaccard_levels_grid(*enc.args, 0.3, capacity=g.pairs + 1, defer=True)
    n = pending.n
    assert 0 < n < g.pairs
    hits = pending.buf.records[:n]
    want = hits.clone()
    enc.call(hits)
    assert torch.equal(hits.view(torch.int64), want.view(torch.int64))
    hits[:, 0] = -3.0
    enc.call(hits)
    assert torch.equal(hits.view(torch.int64), want.view(torch.int64))
    host = want.cpu().numpy()
    ij = host.view(np.int32).reshape(n, 4)
    assert np.array_equal(grid_lookup(g, ij[:, 2], ij[:, 3]), host[:, 0])


# --------------------------------------------------------------------------------------------------------- host faces
def _words(rng, n):
    return " ".join(rng.choice(["fieber", "dialyse", "nach", "ja", "nein", "w1", "w2", "w3", "x_y", "Entlassung"]) for _ in range(n))


def test_plugin_pairs_equal_the_scalar_plugin_calls(dev):
    """200 listed pairs, duplicates among them, one string of more than 512 code units and one set of more than 64 tokens
    on either side: ``plugin.pairs`` equals ``[plugin(a, b) ...]``."""
    from napkon_string_matching_amd.compare import score_functions as sf

    rng = random.Random(6500)
    left = [_words(rng, rng.randint(1, 6)) for _ in range(14)] + [["b a", "c"], "", " ".join(f"t{k}" for k in range(70)),
                                                                  "long " * 120]
    right = [_words(rng, rng.randint(1, 6)) for _ in range(17)] + [["c", "a b"], " ".join(f"t{k}" for k in range(5, 80)),
                                                                   "long " * 110 + "tail"]
    pairs = [(rng.randrange(len(left)), rng.randrange(len(right))) for _ in range(192)]
    pairs += [(16, 18), (17, 19), (16, 0), (0, 18), (17, 0), (0, 19), (15, 3), (3, 3)]  # wide x wide, wide x regular, empty
    assert len(pairs) == 200
    for plugin in (sf.fuzzy_match, sf.intersection_vs_union):
        scalar = {}
        for i, j in pairs:
            if (i, j) not in scalar:
                scalar[(i, j)] = plugin(left[i], right[j])
        got = plugin.pairs(left, right, pairs)
        assert got.dtype == np.float64 and got.tolist() == [scalar[p] for p in pairs], plugin.__name__
        assert np.array_equal(plugin.pairs(left, right, np.array(pairs)), got)
    with pytest.raises(ZeroDivisionError):
        sf.intersection_vs_union.pairs(left, right + [""], [(0, 0), (15, len(right))])


def _score_pairs_case(seed):
    from napkon_string_matching_amd.types.comparable_data import ComparableData
    from support import random_frames

    rng = random.Random(seed)
    left = random_frames.frame(rng, 25, "L", "list", ["c0", "c1"], empty_tokens=0.1)
    right = random_frames.frame(rng, 30, "R", "list", ["c0", "c1"], empty_tokens=0.1)
    return ComparableData(left), ComparableData(right), rng


@pytest.mark.parametrize("score_func", ["intersection_vs_union", "fuzzy_match"])
@pytest.mark.parametrize("column", ["Tokens", "Term"])
def test_score_pairs_equals_compare_terms_per_listed_pair(dev, score_func, column):
    from oracle import compare as oc
    from oracle import score_functions as osf

    left, right, rng = _score_pairs_case(6600)
    lf, rf = left.dataframe().dropna(subset=[column]), right.dataframe().dropna(subset=[column])
    first = lambda frame: {v: k for k, v in reversed(list(enumerate(frame["Identifier"])))}
    pos_l, pos_r = first(lf), first(rf)
    levels = lambda frame, k: oc.gen_comp_value(frame[column].iloc[k])
    candidates = [(a, b) for a in list(left.dataframe()["Identifier"]) + ["nobody"] for b in list(right.dataframe()["Identifier"]) + ["none"]]
    rng.shuffle(candidates)
    pairs, want = [], []
    for a, b in candidates:  # the first 120 pairs the reference does not raise for (the raising ones: the next test)
        if a in pos_l and b in pos_r:
            la, lb = levels(lf, pos_l[a]), levels(rf, pos_r[b])
            try:
                want.append(float(oc.compare_terms(la, lb, osf.get(score_func))))
            except (IndexError, ZeroDivisionError):
                continue
        else:
            want.append(float("nan"))
        pairs.append((a, b))
        if len(pairs) == 120:
            break
    out = left.score_pairs(right, pairs, compare_column=column, score_func=score_func, left_name="hap", right_name="suep")
    frame = out.dataframe()
    got = frame["MatchScore"].to_numpy()
    diff, n_bad = _differences(got, np.array(want), np.arange(len(pairs)), np.arange(len(pairs)))
    assert n_bad == 0 and np.isnan(got).any() and (got > 0).any(), (n_bad, diff)
    assert frame["HapIdentifier"].tolist() == [p[0] for p in pairs] and frame["SuepIdentifier"].tolist() == [p[1] for p in pairs]
    assert list(frame.columns) == [f"{side}{col}" for side in ("Hap", "Suep") for col in ("Identifier", "Variable", "Sheet", "Argument")] + \
        ["MatchScore"]


def test_score_pairs_mapping_input_and_the_reference_exceptions(dev):
    from napkon_string_matching_amd.types.mapping import Mapping

    left, right, _ = _score_pairs_case(6600)
    kw = dict(compare_column="Tokens", score_func="intersection_vs_union", left_name="hap", right_name="suep")
    lf, rf = left.dataframe(), right.dataframe()
    full_l = [v for v, t in zip(lf["Identifier"], lf["Tokens"]) if t]
    full_r = [v for v, t in zip(rf["Identifier"], rf["Tokens"]) if t]
    mapping = Mapping({"u1": {"hap": full_l[:2], "suep": full_r[:3]}, "u2": {"hap": full_l[4:5], "suep": full_r[5:6], "other": ["x"]},
                       "u3": {"hap": full_l[6:7]}})
    listed = [(a, b) for a in full_l[:2] for b in full_r[:3]] + [(full_l[4], full_r[5])]
    by_mapping, by_list = left.score_pairs(right, mapping, **kw), left.score_pairs(right, listed, **kw)
    assert len(by_mapping) == 7 and by_mapping.dataframe().equals(by_list.dataframe())
    # one raising case of each exception type, behind scorable pairs
    bare_r = [v for v, t in zip(rf["Identifier"], rf["Tokens"]) if isinstance(t, list) and not t]
    assert bare_r, "the seeded frame holds no level-less item"
    with pytest.raises(IndexError, match="list index out of range"):
        left.score_pairs(right, listed + [(full_l[0], bare_r[0])], **kw)
    import pandas as pd

    from napkon_string_matching_amd.types.comparable_data import ComparableData

    blank = ComparableData(pd.DataFrame({"Identifier": ["e"], "Term": [["x"]], "Tokens": [[""]], "Variable": ["v"], "Sheet": ["s"],
                                         "Category": [["c0"]]}))
    with pytest.raises(ZeroDivisionError, match="division by zero"):
        blank.score_pairs(blank, [("e", "e")], **kw)


# ------------------------------------------------------------------------------------------------------------ capture
def test_a_captured_pairs_call_replays(dev):
    """One entry captured on a side stream (a single kernel node), replayed twice: the same scores every time."""
    import torch

    g = tp.grid("raw_indel_128")
    enc = Encoded(g, dev)
    i, j = _all_pairs(g, 6700)
    want = grid_lookup(g, i, j)
    stream = torch.cuda.Stream(dev)
    records = torch.from_numpy(_records(i, j)).to(dev)
    with torch.cuda.stream(stream):
        enc.call(records, stream.cuda_stream)  # eager
        stream.synchronize()
        assert np.array_equal(records[:, 0].cpu().numpy(), want)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            enc.call(records, stream.cuda_stream)
        for _ in range(2):
            records[:, 0] = -9.0
            stream.synchronize()
            graph.replay()
            torch.cuda.synchronize(dev)
            assert np.array_equal(records[:, 0].cpu().numpy(), want)
