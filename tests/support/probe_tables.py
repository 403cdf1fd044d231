"""Device tables of the grids of tests/support/threshold_probes.py, built once per process and shared by the GPU test files
that run those grids (threshold probes, profiles, best matches, memory contract).  Never modified by a test."""
import numpy as np

from support import threshold_probes as tp


def first_difference(got, want):
    extra, missing = sorted(set(got) - set(want))[:4], sorted(set(want) - set(got))[:4]
    return f"got {len(got)} hits, oracle {len(want)}; only in got {extra}; lost (only in oracle) {missing}"


_TABLES = {}


def cached(key, make):
    if key not in _TABLES:
        _TABLES[key] = make()
    return _TABLES[key]


def raw_indel_tables(g, dev):
    from napkon_string_matching_amd import tables

    def make():
        lt, rt = tables.encode_strings([tp.text(r) for r in g.left], [tp.text(r) for r in g.right], dev)
        assert lt.stride == rt.stride == g.size and (g.size != 64 or (lt.hist16 is not None and rt.hist16 is not None))
        return lt, rt

    return cached(g.name, make)


def raw_jaccard_tables(g, dev):
    from napkon_string_matching_amd import tables

    def make():
        def padded(rows):
            ids = np.full((len(rows), g.size), -1, dtype=np.int32)
            for r, row in enumerate(rows):
                ids[r, : len(row)] = row
            return ids

        lt = tables.SetTable.from_padded(padded(g.left), "left", dev, width=g.size)
        rt = tables.SetTable.from_padded(padded(g.right), "right", dev, width=g.size)
        assert rt.post is not None and lt.post is None and lt.width == rt.width == g.size
        return lt, rt

    return cached(g.name, make)


def levels_indel_tables(g, dev, partition):
    from napkon_string_matching_amd import tables

    def make():
        items = lambda side: [[tp.text(lv) for lv in it] for it in side]
        li, ls, ri, rs = tables.encode_level_strings(items(g.left), items(g.right), dev, g.cat_l, g.cat_r, g.mode,
                                                     partition=partition)
        assert ls.stride == rs.stride == g.size and (li.seg is not None) == partition
        return li, ls, ri, rs

    return cached((g.name, partition), make)


def levels_jaccard_tables(g, dev, partition):
    from napkon_string_matching_amd import tables

    def make():
        vocabulary = tables.Vocabulary()
        lt = tables.SetTable.from_levels(g.left, "left", dev, vocabulary, width=g.size, categories=g.cat_l, category_mode=g.mode,
                                         partition=partition)
        rt = tables.SetTable.from_levels(g.right, "right", dev, vocabulary, width=g.size, categories=g.cat_r,
                                         category_mode=g.mode, partition=partition)
        assert rt.post is not None and (lt.seg is not None) == partition
        return lt, rt

    return cached((g.name, partition), make)
