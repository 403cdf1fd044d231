"""The packed scan of the two-stage RAW kernel (csrc/indel_raw_coarse.hpp: c3c_pack_left_kernel codes the left operand words
of the FP4 scan once per call, indel_raw_coarse_kernel<.., true> loads them; NSM_FLAG_PACK / NSM_FLAG_NO_PACK).

What can go wrong: the two lane halves or the two operand groups of a packed row in each other's place, a row stride or a
clamp that belongs to the unpacked rows, packed rows counted from the chunk where the scan counts from the table, the
register set that a drain or the end of a block leaves behind, and the host's choice (a captured call must not allocate).
The scan is a filter, so a wrong operand shows as a LOST hit, and only where no other row of the lane's 16 passes: the
cases keep the rows that hit a given right string sparse.

The strings are sorted runs over at most 32 symbols (one bucket each: LCS = sum of min).  The packed call, the unpacked
call, the library's own choice, the one-stage kernel and the oracle are compared bit for bit.
"""
import itertools
import random

import pytest

pytestmark = pytest.mark.gpu

SYMS = "".join(sorted("abcdefghijklmnopqrstuvwxyzABCDEF"))  # 32 symbols, ascending: bucket = position
VARIANTS = ({"pack": True}, {"pack": False}, {}, {"two_stage": False})


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _runs(counts):
    assert len(counts) == 32
    return "".join(s * a for s, a in zip(SYMS, counts))


def _oracle(left, right, thr):
    from oracle import native

    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    return native.indel_raw(cp(left), cp(right), thr, cap=1 << 22)


def _check(dev, left, right, thresholds, in_order=False):
    """Every variant against the oracle at every threshold; returns the oracle's hits at the lowest one."""
    from napkon_string_matching_amd import grid
    from napkon_string_matching_amd import tables as tb

    lt, rt = tb.encode_strings(left, right, dev)
    assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None and lt.alphabet <= 32
    if in_order:  # (built in table order: longest first, equal lengths as given)
        assert lt.orig.cpu().tolist() == list(range(len(left))) and rt.orig.cpu().tolist() == list(range(len(right)))
    base = _oracle(left, right, min(thresholds))
    for thr in thresholds:
        want = [h for h in base if h[0] >= thr]  # (the oracle's list is ordered by score already)
        for kw in VARIANTS:
            got = grid.indel_raw_grid(lt, rt, thr, **kw).as_tuples()
            assert len(got) == len(want), f"thr {thr} {kw}: {len(got)} hits, oracle has {len(want)}"
            assert got == want, f"thr {thr} {kw}"
    return base


def _moved(counts, rng):
    """One unit in another bucket that the string already uses (its set of symbols stays)."""
    out = list(counts)
    used = [s for s in range(32) if out[s] > 0]
    down = rng.choice(used)
    up = rng.choice([s for s in used if s != down])
    out[down] -= 1
    out[up] += 1
    return out


# --- 1. class sizes, table sizes, chunks ------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_right", [1, 33, 129])
def test_class_and_table_sizes(dev, n_right):
    """Left length classes of 65, 33, 32, 31 and 1 rows, 162 rows in three chunks of 64: the class of 65 ends on the first
    row of the second chunk, and the class of 32 straddles the start of the third, whose packed rows are then counted from a
    chunk that begins in the middle of a class.  Right string j is eight runs of five on symbols of its own, and left row i
    is near right string i mod n_right and far from every other: with 33 and 129 right strings a lane's 16 rows hold at
    most one row that hits its string, so every row has to come from its own packed row."""
    rng = random.Random(300 + n_right)
    rights = []
    for _ in range(n_right):
        counts = [0] * 32
        for s in rng.sample(range(32), 8):
            counts[s] = 5
        rights.append(counts)
    left, mates = [], []
    for length, n_rows in ((44, 65), (43, 33), (42, 32), (41, 31), (39, 1)):
        for _ in range(n_rows):
            j = len(left) % n_right
            counts = list(rights[j])
            used = [s for s in range(32) if counts[s]]
            for u in range(abs(length - 40)):
                counts[used[u % 8]] += 1 if length > 40 else -1
            left.append(_runs(_moved(counts, rng)))
            mates.append(j)
            assert len(left[-1]) == length
    assert len(left) == 162
    base = _check(dev, left, list(map(_runs, rights)), (0.8,), in_order=True)
    pairs = {(i, j) for _, i, j in base}
    assert len(pairs) == len(base) and pairs >= set(enumerate(mates))
    if n_right > 1:  # sparse: next to nobody hits a string that is not its mate
        assert len(pairs) <= 2 * len(left)


# --- 2. every left code, at both ends of both lane halves, in the rows of a block -------------------------------------------

_COUNTS = (0, 1, 2, 3, 4, 5, 13, 16, 61)
_BUCKETS = (0, 15, 16, 31)
_ROWS = (0, 3, 4, 31)
_LENGTH = 63


def _special(c, b):
    """63 units: c in bucket b, the rest spread as evenly as it goes over the 31 other buckets, from bucket b + 1 on."""
    counts = [0] * 32
    counts[b] = c
    rest = _LENGTH - c
    for u in range(31):
        counts[(b + 1 + u) % 32] = rest // 31 + (1 if u < rest % 31 else 0)
    assert sum(counts) == _LENGTH
    return counts


def _one_less(counts, b):
    """One unit of bucket b (of the bucket after it where b is empty) in a bucket that gets a unit more."""
    out = list(counts)
    src = b if out[b] > 0 else (b + 1) % 32
    dst = (b + 2) % 32
    assert out[src] > 0
    out[src] -= 1
    out[dst] += 1
    return out


def test_left_codes_in_the_rows_of_a_block(dev):
    """Left counts of 0, 1, 2, 3, 4, 5, 13, 16 and 61 in buckets 0, 15, 16 and 31 (both lane halves, both ends of a lane's 16
    bytes), the row in position 0, 3, 4 and 31 of a block whose 31 other rows are far from everything.  Every left string has
    63 units, so the table is one length class and block k is rows 32 k .. 32 k + 31.  On the right the row's copy (threshold
    1.0: on its need) and the copy with one unit elsewhere (one below)."""
    from tests.support import scan_fp4 as fp4

    far = SYMS[8] * 31 + SYMS[24] * 32
    left, right, about = [], [], []
    for c, b, r in itertools.product(_COUNTS, _BUCKETS, _ROWS):
        counts = _special(c, b)
        block = [far] * 32
        block[r] = _runs(counts)
        about.append((counts, len(left) + r, len(right)))
        left += block
        right += [_runs(counts), _runs(_one_less(counts, b))]
    base = _check(dev, left, right, (0.9, 1.0), in_order=False)
    exact = {(i, j) for s, i, j in base if s >= 1.0}
    for counts, i, j in about:
        assert (i, j) in exact and (i, j + 1) not in exact
        k = fp4.scale_of(counts)  # (16 and 61 on the right: a string with a scale)
        assert sum(fp4.bucket(x, y, k) for x, y in zip(counts, counts)) >= _LENGTH
    assert all(len(x) == _LENGTH for x in left)


# --- 3. a stack that fills in the middle of a class ---------------------------------------------------------------------------


def test_four_letters(dev):
    """A 4-letter alphabet, 96 left rows of one length x 161 right rows at threshold 0: every pair passes, the stack fills in
    the middle of the class and the scan goes on behind a drain with the register set it had loaded before; 0.8 and 1.0
    ride along."""
    rng = random.Random(961)
    word = lambda n: "".join(rng.choice("abcd") for _ in range(n))
    left = [word(40) for _ in range(96)]
    right = [word(rng.randint(24, 64)) for _ in range(150)] + left[:11]
    base = _check(dev, left, right, (0.0, 0.8, 1.0))
    assert len(base) == 96 * 161 and sum(s >= 1.0 for s, _, _ in base) >= 11


# --- 4. the host's choice -----------------------------------------------------------------------------------------------------


def test_a_captured_call_does_not_pack(dev):
    """NSM_FLAG_PACK on a stream that is being captured: the call allocates nothing, runs the unpacked kernel and the graph
    replays to the eager call's hits."""
    import torch

    from napkon_string_matching_amd import _lib, grid
    from napkon_string_matching_amd import tables as tb

    rng = random.Random(4)
    word = lambda: _runs([rng.randint(0, 2) for _ in range(32)])
    left = [word() for _ in range(70)]
    right = left[:20] + [word() for _ in range(50)]
    lt, rt = tb.encode_strings(left, right, dev)
    lib = _lib.load()
    want = grid.indel_raw_grid(lt, rt, 0.8, pack=True).as_tuples()
    assert want == _oracle(left, right, 0.8) and len(want) >= 20

    def launch(buf, stream):
        buf.count.zero_()
        _lib.check(lib.nsm_indel_raw_grid(lt.struct(), rt.struct(), 0.8, _lib.FLAG_PRUNE | _lib.FLAG_PACK, buf.records.data_ptr(),
                                          buf.capacity, buf.count.data_ptr(), stream.cuda_stream), "nsm_indel_raw_grid")

    def hits_of(buf):
        return grid.sort_hits_device(buf, int(buf.count.item())).as_tuples()

    stream = torch.cuda.Stream(dev)
    buf = grid.HitBuffer(1 << 12, dev)
    buf.reset()
    with torch.cuda.stream(stream):
        launch(buf, stream)  # eager: packed
        stream.synchronize()
        assert hits_of(buf) == want
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            launch(buf, stream)
        for _ in range(2):
            g.replay()
            torch.cuda.synchronize(dev)
            assert hits_of(buf) == want
