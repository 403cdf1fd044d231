"""The packed rows of the two-stage RAW scan live in ONE buffer per (device, stream) that the library keeps between calls
(csrc/indel_raw.hip: pack_scratch; nsm_release / nsm_release_all free it).  Only the allocation is kept: the pre-pass codes
the rows again in every call.

What can go wrong: rows of an earlier table read by a later call (a buffer that is reused without the pre-pass, or a smaller
table that scans the tail a larger one left), a buffer that is not grown for a larger table, a released buffer used again,
two streams sharing one buffer, the pre-pass of a call overwriting the rows of the call before it on the same stream.
Every packed result is compared with the unpacked call's and with the oracle's, as tuples.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

SYMS = "abcdefghijklmnopqrstuvwxyzABCDEF"
THR = 0.8


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda:0")


def _words(rng, n, lo=20, hi=64):
    return ["".join(rng.choice(SYMS[:12]) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def _near(rng, word):
    """The word with one symbol replaced: a hit at 0.8 for every length used here."""
    k = rng.randrange(len(word))
    return word[:k] + rng.choice(SYMS[:12]) + word[k + 1:]


def _case(seed, n_left, n_right):
    rng = random.Random(seed)
    left = _words(rng, n_left)
    right = [_near(rng, w) for w in rng.sample(left, min(n_left, n_right // 2))]
    right += _words(rng, n_right - len(right))
    return left, right


def _oracle(left, right):
    from oracle import native

    cp = lambda ss: native.csr([[ord(c) for c in s] for s in ss])
    return native.indel_raw(cp(left), cp(right), THR, cap=1 << 20)


@pytest.fixture(scope="module")
def cases(dev):
    """(tables, oracle hits) of four grids whose left tables have 70, 700, 33 and 260 rows: computed once, never changed."""
    from napkon_string_matching_amd import tables as tb

    out = []
    for seed, (n_left, n_right) in enumerate(((70, 90), (700, 300), (33, 500), (260, 260))):
        left, right = _case(40 + seed, n_left, n_right)
        lt, rt = tb.encode_strings(left, right, dev)
        assert lt.stride == 64 and lt.hist16 is not None and rt.hist16 is not None
        want = _oracle(left, right)
        assert len(want) >= min(n_left, n_right // 2)
        out.append((lt, rt, want))
    return out


def _launch(lib, lt, rt, buf, stream, pack=True):
    from napkon_string_matching_amd import _lib

    buf.count.zero_()
    flags = _lib.FLAG_PRUNE | (_lib.FLAG_PACK if pack else _lib.FLAG_NO_PACK)
    _lib.check(lib.nsm_indel_raw_grid(lt.struct(), rt.struct(), THR, flags, buf.records.data_ptr(), buf.capacity,
                                      buf.count.data_ptr(), stream.cuda_stream), "nsm_indel_raw_grid")


def _hits(buf):
    from napkon_string_matching_amd import grid

    return grid.sort_hits_device(buf, int(buf.count.item())).as_tuples()


def _buffers(dev, n):
    from napkon_string_matching_amd import grid

    bufs = [grid.HitBuffer(1 << 12, dev) for _ in range(n)]
    for b in bufs:
        b.reset()
    return bufs


def test_grow_shrink_release(dev, cases):
    """One stream, left tables of 70, 700, 33 and 260 rows in turn (the buffer grows once, then serves smaller tables whose
    scans must not see the 700-row table's tail), the stream's state released between two rounds and everything released
    after the second: every call gives the unpacked call's hits and the oracle's."""
    import torch

    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.Stream(dev)
    (buf,) = _buffers(dev, 1)
    with torch.cuda.stream(stream):
        for round_ in range(3):
            for lt, rt, want in cases:
                _launch(lib, lt, rt, buf, stream, pack=False)
                stream.synchronize()
                assert _hits(buf) == want
                _launch(lib, lt, rt, buf, stream, pack=True)
                stream.synchronize()
                assert _hits(buf) == want, f"round {round_}, {lt.n} left rows"
            stream.synchronize()
            if round_ == 0:
                assert lib.nsm_release(stream.cuda_stream) == 0
                assert lib.nsm_release(stream.cuda_stream) == 0  # nothing left: still fine
            elif round_ == 1:
                assert lib.nsm_release_all() == 0


def test_back_to_back_calls_on_one_stream(dev, cases):
    """Four packed calls on one stream with nothing between them but the stream's order, each into a hit buffer of its own:
    the pre-pass of a call writes the shared rows behind the scan of the call before it.  Then the same in reverse order."""
    import torch

    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.Stream(dev)
    bufs = _buffers(dev, len(cases))
    with torch.cuda.stream(stream):
        for order in (list(range(len(cases))), list(reversed(range(len(cases))))):
            for k in order:
                _launch(lib, cases[k][0], cases[k][1], bufs[k], stream)
            stream.synchronize()
            for k in order:
                assert _hits(bufs[k]) == cases[k][2], f"order {order}, grid {k}"
    assert lib.nsm_release(stream.cuda_stream) == 0


def test_two_streams_two_buffers(dev, cases):
    """Two streams, each running its own sequence of packed calls with no synchronisation between the two: a buffer belongs
    to one stream."""
    import torch

    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    bufs = [_buffers(dev, len(cases)) for _ in streams]
    torch.cuda.synchronize(dev)
    for rep in range(3):
        for k in range(len(cases)):
            for s, stream in enumerate(streams):
                j = (k + 2 * s) % len(cases)  # the two streams work on different tables at the same time
                with torch.cuda.stream(stream):
                    _launch(lib, cases[j][0], cases[j][1], bufs[s][j], stream)
        torch.cuda.synchronize(dev)
        for s in range(2):
            for k in range(len(cases)):
                assert _hits(bufs[s][k]) == cases[k][2], f"repetition {rep}, stream {s}, grid {k}"
    for stream in streams:
        assert lib.nsm_release(stream.cuda_stream) == 0
