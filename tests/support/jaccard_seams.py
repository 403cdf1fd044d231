"""Host-side model of the launchers of the six Jaccard grid kernels and the inputs of tests/test_cpu_jaccard_seams.py and
tests/test_gpu_jaccard_seams.py.

The kernels are jaccard_raw_kernel (csrc/jaccard_raw_impl.hpp), jaccard_raw_index_kernel (jaccard_raw_index.hip),
jaccard_raw_global_kernel (jaccard_raw_global.hip), jaccard_levels_kernel (jaccard_levels_impl.hpp),
jaccard_levels_index_kernel (jaccard_levels_index.hip) and jaccard_levels_global_kernel (jaccard_levels_global.hip).  Every
rule below is restated from the launcher it cites, in plain Python: nothing is read from the library.  The case families
(A .. G) put tables exactly at the batch, tile, queue and hash seams these rules create; each returns its tables as arrays of
RAW ids (no Vocabulary renumbering: the hash positions are the crafted ones) and a dict of premises for the tests to assert.
All generators are deterministic (one seeded numpy generator per case) and build the big tables with array code.
"""
import ctypes
import functools
import math

import numpy as np

WAVE, WAVES_PER_BLOCK, BLOCK, NEVER = 64, 4, 256, 255  # csrc/nsm_common.hpp:12-15
WAVE_SLOTS = 256 * 8 * WAVES_PER_BLOCK  # jaccard_raw_global.hip:267 (kWaveSlots); the global kernels launch at most 256 * 8 blocks
QUEUE_SLOTS = 32                        # jaccard_levels_impl.hpp:36
GOLDEN = 0x9E3779B1
BLOOM_LOG = 15                          # jaccard_raw_index.hip:33, jaccard_levels_index.hip:20
CAT_NONE, CAT_INTERSECT = 0, 1

LONGEST = {  # the issue's table: W -> {threshold: longest prefix}
    16: {1.0: 1, 0.95: 1, 0.9: 2, 0.8: 4, 0.7: 5, 0.6: 7, 0.5: 9, 0.01: 16},
    32: {1.0: 1, 0.95: 2, 0.9: 4, 0.8: 7, 0.75: 9, 0.5: 17, 0.01: 32},
    64: {1.0: 1, 0.95: 4, 0.9: 7, 0.75: 17, 0.5: 33, 0.01: 64},
}


# --- the launcher model ------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def kmin(W, thr):
    """kmin[s], s = |A| + |B|: the least k with double(k) / double(s - k) >= thr, NEVER if none (jaccard_raw_impl.hpp:308-321,
    fill_kmin; the index kernel's copy jaccard_raw_index.hip:213-226)."""
    out = [NEVER] * (2 * W + 4)
    for s in range(1, 2 * W + 1):
        for k in range(s // 2 + 1):
            if float(k) / float(s - k) >= thr:
                out[s] = k
                break
    return tuple(out)


@functools.lru_cache(maxsize=None)
def prefix(W, thr):
    """(P, longest): P[size] = size - o + 1 with o the least kmin[size + b] a partner size b can reach, 0 where no partner
    reaches the threshold (jaccard_raw_global.hip:225-242, fill_prefix)."""
    km = kmin(W, thr)
    P, longest = [0] * (W + 4), 0
    for a in range(1, W + 1):
        o = min((km[a + b] for b in range(1, W + 1) if km[a + b] != NEVER and 1 <= km[a + b] <= min(a, b)), default=None)
        if o is None:
            continue
        P[a] = a - o + 1
        longest = max(longest, P[a])
    return tuple(P), longest


def longest(W, thr):
    return prefix(W, thr)[1]


def slot_shift(W, thr):
    """log2 of the prefix slots a row takes in a batch (jaccard_raw_global.hip:260-262)."""
    shift = 0
    while (1 << shift) < longest(W, thr):
        shift += 1
    return shift


def cls_end(W, thr):
    """Which of a posting list's five boundaries ends the useful entries (jaccard_raw_global.hip:259)."""
    n = longest(W, thr)
    return 1 if n <= 1 else 2 if n <= 2 else 3 if n <= 4 else 4 if n <= 8 else 5


def posting_class(pos):
    """Posting class of a position in the right row (the builder: tables.inverted_index, positions 0 | 1 | 2-3 | 4-7 | 8+)."""
    return 0 if pos < 1 else 1 if pos < 2 else 2 if pos < 4 else 3 if pos < 8 else 4


def rows_per_batch(n_left, W, thr):
    """Left rows a wavefront takes at once in jaccard_raw_global_kernel (jaccard_raw_global.hip:263-268): 64 >> slot_shift,
    halved while the batches would not fill the 8192 wave slots."""
    r = WAVE >> slot_shift(W, thr)
    while r > 1 and (n_left + r - 1) // r < WAVE_SLOTS:
        r >>= 1
    return r


def n_batches(n_left, W, thr):
    r = rows_per_batch(n_left, W, thr)  # jaccard_raw_global.hip:269
    return (n_left + r - 1) // r


def smallest_n_left(r, W, thr):
    """The smallest left table whose batches hold r rows (rows_per_batch is monotone in n_left), None if the prefix is too
    long for r."""
    if (WAVE >> slot_shift(W, thr)) < r:
        return None
    lo, hi = 1, 1 << 21
    while lo < hi:
        mid = (lo + hi) // 2
        if rows_per_batch(mid, W, thr) >= r:
            hi = mid
        else:
            lo = mid + 1
    return lo


def levels_rows_per_batch(W):
    return WAVE // W  # jaccard_levels_global.hip:48 (kRows)


def levels_n_batches(n_left, W):
    return (n_left + WAVE // W - 1) // (WAVE // W)  # jaccard_levels_global.hip:236-237


def jac_rows_per_chunk(n_left, n_tiles):
    """Left rows per blockIdx.y of jaccard_raw_kernel (jaccard_raw_impl.hpp:323-333)."""
    chunks = max(1, (16 * 256 * 32 + n_tiles - 1) // max(n_tiles, 1))
    return min(4096, max(128, (n_left + chunks - 1) // chunks))


def lev_rows_per_chunk(n_left, n_tiles, partitioned=False):
    """Left rows per blockIdx.y of jaccard_levels_kernel (jaccard_levels_impl.hpp:309-319; :336 caps a partitioned table's
    chunks at 512)."""
    chunks = max(1, (4 * 256 * 32 + n_tiles - 1) // max(n_tiles, 1))
    rows = min(4096, max(512, (n_left + chunks - 1) // chunks))
    return min(rows, 512) if partitioned else rows


def raw_index_geometry(n_left, n_right):
    """(rows per chunk, blocks) of jaccard_raw_index_kernel: four waves per block share a tile and take a chunk each
    (jaccard_raw_index.hip:241-256)."""
    waves, n_tiles, rows = 4, (n_right + WAVE - 1) // WAVE, 1536

    def blocks(rpc):
        return n_tiles * (((n_left + rpc - 1) // rpc + waves - 1) // waves)

    while rows > 256 and blocks(rows) < 4096:
        rows //= 2
    while (n_left + rows - 1) // rows > 65535 * waves:
        rows *= 2
    return rows, blocks(rows)


def lev_index_slices(n_left, n_right, partitioned=False):
    """blockIdx.y slices of jaccard_levels_index_kernel (jaccard_levels_index.hip:278-287)."""
    n_tiles = (n_right + WAVE - 1) // WAVE
    rows_cat = (n_left + 31) // 32 if partitioned else n_left
    slices = (rows_cat + 16383) // 16384
    while slices < 64 and n_tiles * slices < 4096 and rows_cat // (slices * 2) >= 256:
        slices *= 2
    while (n_left + slices - 1) // slices > 4 * 60000:
        slices *= 2
    return slices


def lev_index_wave_ranges(a, b, slices, W):
    """[i0, i1) of every (slice, wave) over the left rows [a, b) (jaccard_levels_index.hip:181-192): a slice of `per` rows, a
    quarter of it per wave, rounded up to whole groups of 64 / W rows."""
    group, per, out = WAVE // W, (b - a + slices - 1) // slices, []
    for y in range(slices):
        lo, hi = a + min(b - a, y * per), a + min(b - a, (y + 1) * per)
        quarter = (((hi - lo) + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK + group - 1) // group * group
        for wave in range(WAVES_PER_BLOCK):
            i0 = min(hi, lo + wave * quarter)
            i1 = min(hi, i0 + quarter)
            if i0 < i1:
                out.append((i0, i1))
    return out


@functools.lru_cache(maxsize=None)
def weak_table(W, thr):
    """weak[a] bit b: the signature bound passes a random pair of these sizes too often and the class runs without the prune
    (jaccard_raw_impl.hpp:342-357)."""
    km, out = kmin(W, thr), []
    for a in range(W + 1):
        bits = 0
        for b in range(min(W, 63) + 1):
            need = km[a + b]
            if need == NEVER or need > min(a, b):
                continue
            mu = float(a) * b / 58.0
            term, below = math.exp(-mu), 0.0
            for k in range(need):
                below += term
                term *= mu / (k + 1)
            if 1.0 - below > 1.0 / 128.0:
                bits |= 1 << b
        out.append(bits)
    return tuple(out)


def weak(W, thr, a, b):
    return b < 64 and bool((weak_table(W, thr)[a] >> b) & 1)  # jaccard_raw_impl.hpp:223


def index_slots(W):
    return 1024 if W == 16 else 2048  # jaccard_raw_impl.hpp:42-43


def is_dense(total_ids, W):
    return total_ids > index_slots(W) * 3 // 4  # jaccard_raw_impl.hpp:46-51 (tile_is_dense)


def _hh(ids):
    return (np.asarray(ids).astype(np.uint64) * np.uint64(GOLDEN)) & np.uint64(0xFFFFFFFF)


def home(ids, W):
    """Home slot of an id in a tile's table (jaccard_raw_index.hip:102-103, jaccard_levels_index.hip:160-161)."""
    return (_hh(ids) >> np.uint64(32 - (10 if W == 16 else 11))).astype(np.int64)


def bloom_bits(ids):
    """The two bits of an id in the presence bitmap (jaccard_raw_index.hip:110-113, jaccard_levels_index.hip:168-171)."""
    hh = _hh(ids)
    return (hh >> np.uint64(32 - BLOOM_LOG)).astype(np.int64), ((hh >> np.uint64(1)) & np.uint64((1 << BLOOM_LOG) - 1)).astype(np.int64)


def probe_table(ids, W):
    """Insert distinct ids in the given order with the kernels' linear probe; returns (slot of every id, occupied [T]).  The
    SET of occupied slots does not depend on the order (the kernels insert in whatever order the atomics resolve)."""
    T = index_slots(W)
    occupied, slot = np.zeros(T, dtype=bool), {}
    for x, h in zip(np.asarray(ids).tolist(), home(ids, W).tolist()):
        while occupied[h]:
            h = (h + 1) & (T - 1)
        occupied[h] = True
        slot[x] = h
    return slot, occupied


def run_across_end(occupied):
    """(first slot, slots past the wrap) of the occupied run that contains both the last slot and slot 0; None if none."""
    T = len(occupied)
    if not (occupied[T - 1] and occupied[0]) or occupied.all():
        return None
    first = T - 1
    while occupied[first - 1]:
        first -= 1
    past = 0
    while occupied[past]:
        past += 1
    return first, past


def cluster_premises(tile_ids, absent_ids, W):
    """What the model counts for a tile (or one pass of a dense tile) of family D."""
    T = index_slots(W)
    present = np.unique(np.asarray(tile_ids))
    slot, occupied = probe_table(present, W)
    run = run_across_end(occupied)
    assert run is not None, "no probe run crosses the table's end"
    first, past = run
    homes = home(present, W)
    in_last4 = present[homes >= T - 4]
    displaced = sum(1 for x, h in zip(present.tolist(), homes.tolist()) if h >= first and slot[x] < past)
    bits = np.zeros(1 << BLOOM_LOG, dtype=bool)
    b1, b2 = bloom_bits(present)
    bits[b1] = True
    bits[b2] = True
    absent = np.setdiff1d(np.unique(np.asarray(absent_ids)), present)
    a1, a2 = bloom_bits(absent)
    passing = bits[a1] & bits[a2]
    ahome = home(absent, W)
    return {
        "run_first": first, "run_past_wrap": past, "run_length": T - first + past,
        "homed_in_last_four": int(len(in_last4)), "displaced_past_wrap": int(displaced),
        "absent_passing_before_wrap": int((passing & (ahome >= first)).sum()),  # probed across the wrap to an empty slot
        "absent_failing": int((~passing).sum()),
    }


COLL_BITS = np.uint64(0xFC00000000000000)  # nsm_common.hpp:94 (kCollBits)


def popcount64(x):
    return np.bitwise_count(np.asarray(x, dtype=np.uint64)).astype(np.int64)




def signature(ids, cnt):
    """Signature word of the first cnt ids of every row (include/nsm_hip.h: sig): bit (h16 * 58) >> 16 per id, h16 = bits
    16 .. 31 of id * 0x9E3779B1; the ids that share a bit with an earlier one of their row are counted in unary in the top
    six bits, and a row with more than six of them is all ones."""
    ids, cnt = np.asarray(ids), np.asarray(cnt, dtype=np.int64)
    h16 = (_hh(ids) >> np.uint64(16)) & np.uint64(0xFFFF)
    bits = np.where(np.arange(ids.shape[1])[None, :] < cnt[:, None], np.uint64(1) << ((h16 * np.uint64(58)) >> np.uint64(16)), np.uint64(0))
    word = np.bitwise_or.reduce(bits, axis=1)
    extra = cnt - popcount64(word)
    unary = ((np.uint64(1) << np.minimum(extra, 6).astype(np.uint64)) - np.uint64(1)) << np.uint64(58)
    return np.where(extra > 6, np.uint64(0xFFFFFFFFFFFFFFFF), word | unary)


def filter_bound_reaches(l_ids, l_cnt, l_plen1, r_ids, r_cnt, r_plen1, thr):
    """[left row][right row]: the signature filter of jaccard_levels_kernel passes (jaccard_levels_impl.hpp:66, 166-175)."""
    sl, sl1 = signature(l_ids, l_cnt), signature(l_ids, np.minimum(l_plen1, l_cnt))
    sr, sr1 = signature(r_ids, r_cnt) | COLL_BITS, signature(r_ids, np.minimum(r_plen1, r_cnt)) | COLL_BITS
    pr1 = np.asarray(r_plen1, dtype=np.int64)
    need = np.ceil(2.0 * thr * pr1.astype(np.float64) * (1.0 - 1e-9)).astype(np.int64)
    bound = np.minimum(popcount64(sl[:, None] & sr[None, :]), pr1[None, :]) + popcount64(sl1[:, None] & sr1[None, :])
    return bound >= need[None, :]


def levels_filter_pass(lfilt, rfilt_row, thr):
    """Which left filter records the signature filter of jaccard_levels_kernel queues for one right item, categories aside
    (jaccard_levels_impl.hpp:66, 166-175): min(bound, |B_1|) + bound_1 >= ceil(2 thr |B_1| (1 - 1e-9))."""
    lf = np.asarray(lfilt).view(np.uint32).reshape(-1, 8).astype(np.uint64)
    rf = np.asarray(rfilt_row).view(np.uint32).reshape(8).astype(np.uint64)
    sl, sl1 = lf[:, 0] | (lf[:, 1] << np.uint64(32)), lf[:, 5] | (lf[:, 6] << np.uint64(32))
    sr, sr1 = (rf[0] | (rf[1] << np.uint64(32))) | COLL_BITS, (rf[5] | (rf[6] << np.uint64(32))) | COLL_BITS
    pr1 = int(rf[4] & np.uint64(0xFF))
    need = int(math.ceil(2.0 * thr * float(pr1) * (1.0 - 1e-9)))
    return np.minimum(popcount64(sl & sr), pr1) + popcount64(sl1 & sr1) >= need


# --- the oracle, as arrays ---------------------------------------------------------------------------------------------------

HIT = np.dtype([("score", "<f8"), ("i", "<i4"), ("j", "<i4")])


def _canonical(buf):
    return buf[np.lexsort((buf["j"], buf["i"], -buf["score"]))]  # score descending, then i, then j (grid.Hits)


def _run_oracle(fn, before, thr, cap):
    while True:
        buf = np.zeros(cap, dtype=HIT)
        n = fn(*before, ctypes.c_double(thr), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(cap))
        assert n >= 0, f"the oracle refused the tables ({n})"
        if n <= cap:
            return _canonical(buf[:n])
        cap = int(n)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def oracle_raw(left, right, thr, cap=1 << 16):
    """oracle.native's RAW Jaccard grid over two padded id arrays; hits as one HIT array in canonical order."""
    from oracle import native

    (lv, lo), (rv, ro) = native.csr_from_padded(np.asarray(left)), native.csr_from_padded(np.asarray(right))
    return _run_oracle(native.lib().oracle_jaccard_raw,
                       (_p(lv), _p(lo), ctypes.c_int(len(lo) - 1), _p(rv), _p(ro), ctypes.c_int(len(ro) - 1)), thr, cap)


def levels_csr(ids, plen, nlev):
    """(values, set offsets, item offsets) of suffix-nested items: level l of item k = its first plen[k][l] ids."""
    ids, plen, nlev = np.asarray(ids), np.asarray(plen, dtype=np.int64), np.asarray(nlev, dtype=np.int64)
    item, lev = np.nonzero(np.arange(plen.shape[1])[None, :] < nlev[:, None])
    length = plen[item, lev]
    off = np.zeros(len(length) + 1, dtype=np.int64)
    np.cumsum(length, out=off[1:])
    pos = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], length)
    val = np.ascontiguousarray(ids[np.repeat(item, length), pos].astype(np.int32))
    lev_off = np.zeros(len(nlev) + 1, dtype=np.int64)
    np.cumsum(nlev, out=lev_off[1:])
    return (val if len(val) else np.zeros(1, np.int32)), off, lev_off


def oracle_levels(left, right, thr, lcat=None, rcat=None, mode=CAT_NONE, cap=1 << 16):
    """oracle.native's levels Jaccard grid over two (ids, plen, nlev) triples; hits as one HIT array in canonical order."""
    from oracle import native

    lv, lo, ll = levels_csr(*left)
    rv, ro, rl = levels_csr(*right)
    lc = None if lcat is None else np.ascontiguousarray(lcat, dtype=np.uint64)
    rc = None if rcat is None else np.ascontiguousarray(rcat, dtype=np.uint64)
    return _run_oracle(native.lib().oracle_levels,
                       (ctypes.c_int(0), _p(lv), _p(lo), _p(ll), ctypes.c_int(len(ll) - 1), _p(rv), _p(ro), _p(rl),
                        ctypes.c_int(len(rl) - 1), _p(lc), _p(rc), ctypes.c_int(mode)), thr, cap)


def case_oracle(case, thr=None):
    thr = case["thr"] if thr is None else thr
    if case["kind"] == "raw":
        return oracle_raw(case["left"], case["right"], thr, cap=case.get("cap", 1 << 16))
    return oracle_levels(case["left"], case["right"], thr, case.get("lcat"), case.get("rcat"), case.get("mode", CAT_NONE),
                         cap=case.get("cap", 1 << 16))


def build_tables(case, device, index=None, compact=True):
    """(left table, right table) of a case through the product's builders: the numpy path on a CPU device, the GPU builder
    on the GPU.  ``index``: the right table's global inverted index (None = the builder's default); ``compact``: its posting
    entries (False = the 64-bit format)."""
    from napkon_string_matching_amd import tables

    W = case["width"]
    keep = tables.COMPACT_POSTINGS
    tables.COMPACT_POSTINGS = bool(compact)
    try:
        if case["kind"] == "raw":
            lt = tables.SetTable.from_padded(case["left"], "left", device, width=W, validate=False)
            rt = tables.SetTable.from_padded(case["right"], "right", device, width=W, validate=False, index=index)
        else:
            mode, part = case.get("mode", CAT_NONE), case.get("partition", False)
            (li, lp, ln), (ri, rp, rn) = case["left"], case["right"]
            lt = tables.SetTable.from_nested_arrays(li, lp, ln, "left", device, categories=case.get("lcat"), width=W,
                                                    category_mode=mode, partition=part)
            rt = tables.SetTable.from_nested_arrays(ri, rp, rn, "right", device, categories=case.get("rcat"), width=W,
                                                    category_mode=mode, partition=part, index=index)
    finally:
        tables.COMPACT_POSTINGS = keep
    return lt, rt


def column(table, name):
    return getattr(table, name).cpu().numpy()


def _pad(rows, W, fill=-1):
    out = np.full((len(rows), W), fill, dtype=np.int32)
    for k, r in enumerate(rows):
        out[k, : len(r)] = r
    return out


def _nested(ids, nlev, L=4):
    """plen of rows whose ids are spread evenly over their levels: plen[l] = ceil(cnt (l + 1) / nlev), padded with cnt."""
    ids = np.asarray(ids)
    cnt = (ids >= 0).sum(axis=1).astype(np.int64)
    nlev = np.broadcast_to(np.asarray(nlev, dtype=np.int64), cnt.shape).copy()
    lv = np.minimum(np.arange(L)[None, :] + 1, nlev[:, None])
    plen = -((-cnt[:, None] * lv) // nlev[:, None])
    return ids.astype(np.int32), plen.astype(np.uint8), nlev.astype(np.int32)


# --- family A: batch geometry of the global RAW index ---------------------------------------------------------------------

A_BASES, A_DUPS, A_HUBS = 48, 16, 6  # right rows: 48 distinct, the first 16 twice; the last 6 distinct ones share id 0


def batch_sizes():
    """(name, W, thr, n_left, small sets) of family A, every count taken from the model."""
    out = []
    for r, thr in ((2, 0.5), (4, 0.5), (8, 0.6), (16, 0.8), (32, 0.9), (64, 0.95)):
        n = smallest_n_left(r, 16, thr)
        out.append((f"w16_r{r}_smallest", 16, thr, n, r == 64))
        if r in (2, 8):  # the seam: still halved | (keeps r: above) | keeps r with a full last batch | a partial last batch
            out.append((f"w16_r{r}_halves", 16, thr, n - 1, False))
            out.append((f"w16_r{r}_full", 16, thr, WAVE_SLOTS * r, False))
            out.append((f"w16_r{r}_partial", 16, thr, WAVE_SLOTS * r + r - 1, False))
    for W, thr in ((32, 0.5), (64, 0.75)):  # two rows per batch at the other widths, and their loop's second trip
        out.append((f"w{W}_r2", W, thr, smallest_n_left(2, W, thr), False))
        out.append((f"w{W}_r2_partial", W, thr, WAVE_SLOTS * 2 + 1, False))
    out.append(("w16_r1_stride", 16, 0.5, WAVE_SLOTS + 9, False))  # one row per batch, more batches than wave slots
    return out


@functools.lru_cache(maxsize=None)
def batch_case(name):
    """Every left row copies a right row (some drop its largest id where the threshold allows); the left rows of the first
    A_DUPS right rows hit twice; the left rows of the last A_HUBS share id 0 -- the smallest id, so inside every prefix --
    with the other hub rows and miss them."""
    _, W, thr, n_left, small = next(s for s in batch_sizes() if s[0] == name)
    rng = np.random.default_rng(W * 1000003 + n_left)
    pool = [6, 5, 4, 3, 2] if small else [W, W - 1, 3 * W // 4, W // 2 + 1, W // 2, W // 4 + 1, 3, 2]
    size = np.array([pool[j % len(pool)] for j in range(A_BASES)])
    base = np.full((A_BASES, W), -1, dtype=np.int32)
    for j in range(A_BASES):
        row = j * 2 * W + 1 + np.arange(size[j])
        if j >= A_BASES - A_HUBS:
            row = np.concatenate([[0], row[:-1]])
        base[j, : size[j]] = row
    right = np.concatenate([base, base[:A_DUPS]])
    partner = rng.integers(0, A_BASES, n_left)
    drop_ok = (size >= 3) & ((size - 1) / size >= thr + 0.02)  # a copy without its largest id still reaches the threshold
    drop = (rng.random(n_left) < 0.3) & drop_ok[partner]
    left = base[partner].copy()
    left[np.flatnonzero(drop), size[partner[drop]] - 1] = -1
    return {"kind": "raw", "name": name, "width": W, "thr": thr, "left": left, "right": right, "cap": 2 * n_left,
            "premises": {"n_left": n_left, "two_hits": partner < A_DUPS, "near_miss": partner >= A_BASES - A_HUBS}}


def mixed_batches(cnt, r):
    """Batches of r consecutive rows of a built table that hold rows of different sizes."""
    cnt = np.asarray(cnt)
    b = np.arange(len(cnt)) // r
    lo = np.full(b[-1] + 1, 1 << 30)
    hi = np.zeros(b[-1] + 1, dtype=np.int64)
    np.minimum.at(lo, b, cnt)
    np.maximum.at(hi, b, cnt)
    return int((lo != hi).sum())


# --- family B: batch geometry of the global levels index ------------------------------------------------------------------

B_COUNT = {16: 6, 32: 20, 64: 40}  # ids per item: every row has the same size, so the builder keeps the input order
B_RIGHT = 64


def levels_batch_sizes():
    out = []
    for W in (16, 32, 64):
        k = WAVE // W
        for tag, n in (("below", WAVE_SLOTS * k - 1), ("at", WAVE_SLOTS * k), ("above", WAVE_SLOTS * k + 1 + k)):
            for part in (False, True):
                out.append((f"w{W}_{tag}_{'part' if part else 'plain'}", W, n, part))
    return out


def planted_batches(n_left, W):
    """The batches family B plants hits in: the first, indices 8191 and 8192 (where they exist) and the last."""
    last = levels_n_batches(n_left, W) - 1
    return sorted({b for b in (0, WAVE_SLOTS - 1, WAVE_SLOTS, last) if b <= last})


@functools.lru_cache(maxsize=None)
def levels_batch_case(name):
    _, W, n_left, part = next(s for s in levels_batch_sizes() if s[0] == name)
    c, k = B_COUNT[W], WAVE // W
    rid = (64 * np.arange(B_RIGHT)[:, None] + np.arange(c)[None, :]).astype(np.int32)
    right = _nested(rid, 2 + np.arange(B_RIGHT) % 3)
    pool = np.array([x for x in range(4096) if x % 64 >= c], dtype=np.int32)  # ids no right item holds
    i = np.arange(n_left, dtype=np.int64)
    lid = pool[(i[:, None] * 7 + np.arange(c)[None, :] * 37) % len(pool)].astype(np.int32)
    share = i % 4 == 1  # candidates that fail: one id (in every level) of a right item, the rest foreign
    lid[share, 0] = 64 * (i[share] % B_RIGHT)
    lnlev = (2 + i % 3).astype(np.int64)
    seg = np.minimum(3, i * 4 // n_left)  # category of a left item: four contiguous blocks, so the partition keeps the order
    rows = np.concatenate([np.arange(b * k, min(n_left, (b + 1) * k)) for b in planted_batches(n_left, W)])
    for row in rows.tolist():
        j = 4 * (row % 16) + int(seg[row])  # a right item of the row's category
        lid[row] = rid[j]
        lnlev[row] = 2 + j % 3
        if row % 2:  # a near copy: the last id (only in the last level) is foreign
            lid[row, c - 1] = pool[row % len(pool)]
    left = _nested(lid, lnlev)
    case = {"kind": "levels", "name": name, "width": W, "thr": 0.5, "left": left, "right": right, "cap": 1 << 12,
            "premises": {"n_left": n_left, "planted_rows": rows, "planted_batches": planted_batches(n_left, W)}}
    if part:
        jj = np.arange(B_RIGHT)
        rcat = (np.uint64(1) << (jj % 4).astype(np.uint64)) | np.where(jj % 4 == 0, np.uint64(2), np.uint64(0))
        case.update(mode=CAT_INTERSECT, partition=True, lcat=np.uint64(1) << seg.astype(np.uint64), rcat=rcat.astype(np.uint64))
    return case


# --- family C: the prefix edge of the global RAW index -----------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def prefix_case(W, thr):
    """Per size pair (a, b) that can reach the threshold: one right row, a left row that shares exactly kmin[a + b] ids with
    it -- the LARGEST ids of both rows, so the first common id sits at positions a - kmin and b - kmin -- and a left row that
    shares one id fewer.  Every pair lives in an id block of its own."""
    km = kmin(W, thr)
    left, right, meta = [], [], []
    for a in range(1, W + 1):
        for b in range(1, W + 1):
            need = km[a + b]
            if need == NEVER or need < 1 or need > min(a, b):
                continue  # (the size pair cannot reach the threshold)
            base = len(right) * 3 * W
            common = base + 2 * W + np.arange(need)
            right.append(np.concatenate([base + W + np.arange(b - need), common]))
            left.append(np.concatenate([base + np.arange(a - need), common]))
            left.append(np.concatenate([base + np.arange(a - need + 1), common[1:]]))
            meta.append((a, b, need))
    meta = np.array(meta)
    return {"kind": "raw", "name": f"w{W}_thr{thr}", "width": W, "thr": thr, "left": _pad(left, W), "right": _pad(right, W),
            "cap": 1 << 14, "premises": {"pairs": meta, "left_pos": meta[:, 0] - meta[:, 2], "right_pos": meta[:, 1] - meta[:, 2]}}


# --- family D: hash-table clusters of the per-tile index kernels ----------------------------------------------------------

D_ABSENT = 40


@functools.lru_cache(maxsize=None)
def cluster_ids(W, limit):
    """(cluster, helpers, absent passing, absent failing, fillers).  cluster: >= 100 ids homed in the last four slots of the
    table plus two per slot of the four before them; absent passing: ids homed in the last eight slots that are NOT in the
    tile but find both their bitmap bits set -- by the cluster or by a helper, an id homed elsewhere that sets the bit as
    its SECOND bit; fillers: ids homed in the middle half of the table (they make a tile dense without touching the run)."""
    T = index_slots(W)
    ids = np.arange(limit, dtype=np.int64)
    h = home(ids, W)
    last4, pre4 = ids[h >= T - 4], ids[(h >= T - 8) & (h < T - 4)]
    n_cluster = 120 if len(last4) >= 200 else 100
    cluster = np.concatenate([last4[:: len(last4) // n_cluster][:n_cluster]] +  # (spread over the whole id range)
                             [pre4[home(pre4, W) == s][:2] for s in range(T - 8, T - 4)])
    spare = np.concatenate([last4, pre4])
    spare = spare[~np.isin(spare, cluster)][:4000]
    ids, h = ids[: 1 << 20], h[: 1 << 20]
    free = ids[(h < T - 8) & (h >= 8)]  # helpers and fillers are not homed at either end of the table
    _, f2 = bloom_bits(free)
    by_second = np.full(1 << BLOOM_LOG, -1, dtype=np.int64)
    by_second[f2[::-1]] = free[::-1]  # the smallest free id whose second bit is v
    bits = np.zeros(1 << BLOOM_LOG, dtype=bool)
    c1, c2 = bloom_bits(cluster)
    bits[c1] = True
    bits[c2] = True
    helpers, passing = [], []
    s1, s2 = bloom_bits(spare)
    for x, v1, v2 in zip(spare.tolist(), s1.tolist(), s2.tolist()):
        need = [v for v in (v1, v2) if not bits[v]]
        if any(by_second[v] < 0 for v in need):
            continue
        for v in need:
            p = int(by_second[v])
            helpers.append(p)
            q1, q2 = bloom_bits(np.array([p]))
            bits[q1] = True
            bits[q2] = True
        passing.append(x)
        if len(passing) == D_ABSENT:
            break
    helpers = np.unique(np.array(helpers, dtype=np.int64))
    taken = np.concatenate([cluster, helpers, np.array(passing, dtype=np.int64)])
    free = free[: 1 << 16]
    fh = home(free, W)
    mid = free[(fh >= T // 4) & (fh < 3 * T // 4)]
    mid = mid[~np.isin(mid, taken)]
    fillers = mid[:: max(1, len(mid) // 1600)][:1600]
    rest = free[~np.isin(free, np.concatenate([taken, fillers]))]
    return cluster, helpers, np.array(passing, dtype=np.int64), rest, fillers


@functools.lru_cache(maxsize=None)
def cluster_case(W, kind, dense):
    """One right tile whose table holds a probe run across the table's end (cluster_ids), sparse or dense; left rows that
    copy the tile's rows (hits; every cluster id is looked up, wherever the insertion order put it), rows of absent ids that
    pass the bitmap -- alone and beside present ids --, and rows of absent ids that fail it."""
    limit = (1 << 24) if kind == "raw" else (1 << 16)
    cluster, helpers, passing, rest, fillers = cluster_ids(W, limit)
    present = np.concatenate([cluster, helpers])
    if dense:  # rows 0 .. 31 (the first pass): all of `present` and fillers up to W ids; rows 32 .. 63: W / 2 + 1 fillers
        rows, f = [], 0
        for r in range(32):
            own = present[r::32]
            rows.append(np.concatenate([own, fillers[f: f + W - len(own)]]))
            f += W - len(own)
        for r in range(32):
            rows.append(fillers[f: f + W // 2 + 1])
            f += W // 2 + 1
    else:
        rows = [present[r::64] for r in range(64)]
    assert all(len(r) <= W for r in rows)
    fail = rest[:: max(1, len(rest) // 64)][:64]  # (whether they really fail the bitmap is counted by cluster_premises)
    groups = [passing[k: k + 4] for k in range(0, len(passing) - 3, 4)]
    lrows = list(rows)  # copies: hits
    lrows += [np.concatenate([rows[k][:2], g]) for k, g in enumerate(groups)]
    lrows += groups
    lrows += [fail[4 * k: 4 * k + 4] for k in range(8)]
    lrows += [np.concatenate([rows[k + 20][:3], fail[32 + 4 * k: 36 + 4 * k]]) for k in range(8)]
    left, right = _pad(lrows, W), _pad(rows, W)
    case = {"kind": kind, "name": f"{kind}_w{W}_{'dense' if dense else 'sparse'}", "width": W, "cap": 1 << 12,
            "thrs": (0.01, 0.3) if kind == "raw" else (0.05, 0.3), "thr": 0.3,
            "premises": {"absent": np.concatenate([passing, fail]), "dense": dense}}
    if kind == "raw":
        case.update(left=left, right=right, index=False)  # (no posting table sized by ids up to 2^24)
    else:
        case.update(left=_nested(left, 2), right=_nested(right, 2))
    return case


# --- family E: the dense rule ---------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def dense_case(W, kind, variant):
    """variant "at": one tile of exactly 3/4 T ids; "over": one id more; "partial": a full tile and a dense partial tile of 49
    full rows, whose second pass holds 17 lanes.  (A partial tile of 33 valid rows cannot be dense at either width:
    33 * 16 = 528 <= 768 and 33 * 32 = 1056 <= 1536; 49 rows is the smallest dense partial tile at both.)"""
    rng = np.random.default_rng(W * 31 + len(variant))
    per = 3 * W // 4 if variant != "partial" else W
    n_right = 64 if variant != "partial" else 64 + 49
    ids = rng.permutation(60000)[: n_right * W + 64].astype(np.int32)
    rows = [ids[r * W: r * W + per] for r in range(n_right)]
    if variant == "over":
        rows[0] = ids[: per + 1]  # (the larger row sorts first: the input order is the built order)
    first, valid = (0, 64) if variant != "partial" else (64, 49)
    rows[first + 40] = np.concatenate([rows[first + 5][:-1], rows[first + 40][-1:]])  # lanes 5 and 40: all but one id in common
    lanes = [0, 31, 32, valid - 1]
    lrows = [rows[first + q] for q in lanes] + [rows[first + 5]]            # hits on both halves of the tile
    lrows += [np.concatenate([rows[first + q][: per // 2], ids[-16:-8]]) for q in lanes]  # half of a row and foreign ids
    lrows += [rows[q] for q in (0, 63)] if variant == "partial" else []
    foreign = 60000 + rng.permutation(60000)[: 100 * 8].astype(np.int32).reshape(100, 8)
    foreign[::5, 0] = ids[: 20]  # (one id of the right table: a candidate that cannot hit)
    lrows += list(foreign)
    left, right = _pad(lrows, W), _pad(rows, W)
    case = {"kind": kind, "name": f"{kind}_w{W}_{variant}", "width": W, "thr": 0.3, "cap": 1 << 12,
            "premises": {"tile": first // 64, "lanes": lanes, "valid": valid}}
    if kind == "raw":
        case.update(left=left, right=right)
    else:
        case.update(left=_nested(left, 2), right=_nested(right, 2))
    return case


# --- family F: the per-lane candidate queues of the levels kernels --------------------------------------------------------

F_DEPTHS = (27, 28, 29, 30, 31, 32, 33, 61, 62, 63)  # (27 / 28: jaccard_levels_kernel flushes past kQueueSlots - 4 - 1 = 27)
F_THR = 0.7


def _queue_items(layout):
    """64 right items of 12 ids in three levels of 4, 8 and 12 (at either width: a row of 32 ids saturates its signature
    word, which then passes every filter, so "exactly c candidates" needs smaller rows).  Layout "all": every item has the
    same first two levels, so a copy of one is a candidate of all 64 lanes; else the items are disjoint."""
    rid = (1000 + 64 * np.arange(64)[:, None] + np.arange(12)[None, :]).astype(np.int32)
    if layout == "all":
        rid[:, :8] = rid[0, :8]
    return rid


def _foreign_rows(rng, n, size, rid, thr):
    """n rows of `size` random ids above every planted id that the signature filter rejects for EVERY right item (three
    levels, spread as _nested does), so that they are candidates of no lane in either levels kernel."""
    out = np.zeros((0, size), dtype=np.int64)
    plen1 = -(-size * 2 // 3)
    while len(out) < n:
        start, stride = rng.integers(0, 1 << 22, (2 * n + 8, 1)), 2 * rng.integers(0, 1 << 20, (2 * n + 8, 1)) + 1
        rows = 100000 + (start + stride * np.arange(size)[None, :]) % (1 << 22)  # (an odd stride: distinct inside the row)
        reach = filter_bound_reaches(rows, np.full(len(rows), size), np.full(len(rows), plen1), rid, np.full(64, 12),
                                     np.full(64, 8), thr)
        out = np.concatenate([out, rows[~reach.any(axis=1)]])
    return list(out[:n].astype(np.int32))


@functools.lru_cache(maxsize=None)
def queue_case(W, c, layout, front=0, n_left=600, cut=False):
    """c candidates of the right item on lane X (layouts "alone": X = 17, "last": X = 63, "all": every lane): copies (hits:
    0.875) and near copies (the first two levels of the item, then 8 foreign ids: 0.65, candidates that fail F_THR).  The
    builder sorts by size: `front` foreign rows of 16 ids come first, then the near copies (16 ids), the copies (12), and
    foreign rows of 11 ids.  ``cut``: a category partition whose segment 1 starts at row 300 and holds the candidates."""
    rng = np.random.default_rng(W * 100 + c)
    rid = _queue_items(layout)
    X = {"alone": 17, "last": 63, "all": 0}[layout]
    near = [np.concatenate([rid[X, :8], 20000 + 64 * t + np.arange(8)]) for t in range(c // 2)]
    copies = [rid[(X + t) % 64 if layout == "all" else X] for t in range(c - c // 2)]
    n_seg0 = 300 if cut else 0
    big = _foreign_rows(rng, front, 16, rid, F_THR)
    small = _foreign_rows(rng, n_left - front - c - n_seg0, 11, rid, F_THR)
    seg0 = _foreign_rows(rng, n_seg0, 8, rid, F_THR)
    lrows = seg0 + big + near + copies + small
    left = _nested(_pad(lrows, W), 3)
    left[1][n_seg0 + front: n_seg0 + front + len(near)] = np.array([4, 8, 16, 16], dtype=np.uint8)
    right = _nested(_pad(list(rid), W), 3)
    case = {"kind": "levels", "name": f"w{W}_c{c}_{layout}_front{front}{'_cut' if cut else ''}", "width": W, "thr": F_THR,
            "left": left, "right": right, "cap": 1 << 14,
            "premises": {"lane": X, "depth": c, "first": n_seg0 + front, "all_lanes": layout == "all"}}
    if cut:
        lcat = np.where(np.arange(len(lrows)) < n_seg0, 1, 2).astype(np.uint64)
        rcat = np.where(np.arange(64) % 2 == 0, 1, 2).astype(np.uint64)
        rcat[X] = 2
        case.update(mode=CAT_INTERSECT, partition=True, lcat=lcat, rcat=rcat)
    return case


def shares_id(left_ids, right_row):
    """Which rows of a built left table share an id with one built right row."""
    r = np.asarray(right_row)
    return np.isin(np.asarray(left_ids), r[r >= 0]).any(axis=1)


# --- family G: run lengths of the pruned signature kernel -----------------------------------------------------------------

G_RUNS = (25, 24, 17, 16, 15, 9, 8, 7, 1, 0)  # rows of sizes W, W - 1, ...; then 20 rows of size W - 10: cut by the chunk end
G_THR = 0.9


@functools.lru_cache(maxsize=None)
def run_case(W):
    """Left size classes of exactly G_RUNS rows inside the first chunk of 128, the next class cut by the chunk boundary; the
    first and the last row of every run copy a right row of their size (hits), the others are foreign."""
    rng = np.random.default_rng(W)
    sizes = [W - k for k in range(len(G_RUNS) + 1)]
    runs = list(G_RUNS) + [20]
    rrows = [5000 * (k + 1) + np.arange(s) for k, s in enumerate(sizes)]
    rrows += [300000 + 64 * t + np.arange(int(rng.integers(W // 4, W + 1))) for t in range(70)]
    lrows, ends = [], []
    for k, (s, n) in enumerate(zip(sizes, runs)):
        for t in range(n):
            edge = t in (0, n - 1)
            lrows.append(rrows[k] if edge else 100000 + 64 * len(lrows) + np.arange(s))
        if n:
            ends.append((s, n))
    lrows += [200000 + 64 * t + np.arange(W - 11) for t in range(40)]
    return {"kind": "raw", "name": f"w{W}", "width": W, "thr": G_THR, "left": _pad(lrows, W), "right": _pad(rrows, W),
            "cap": 1 << 12, "premises": {"runs": dict(zip(sizes, runs)), "cut_size": sizes[-1]}}


# --- the premises, asserted from the BUILT tables (both test files call these first) --------------------------------------


def check_batch(case, lt, rt):
    """Family A: the table sits on the rows_per_batch value its name says; returns what the model derived."""
    name, W, thr, n = case["name"], case["width"], case["thr"], case["premises"]["n_left"]
    assert lt.n == n == len(column(lt, "cnt")) and 64 <= rt.n <= 128
    assert rt.post is not None and rt.vocab > 0, "family A needs the right table's global index"
    r, nb = rows_per_batch(n, W, thr), n_batches(n, W, thr)
    want = int(name.split("_r")[1].split("_")[0])
    if name.endswith("_halves"):
        assert r == want // 2 and rows_per_batch(n + 1, W, thr) == want, f"rows_per_batch {r}: not the last size that halves"
    else:
        assert r == want, f"rows_per_batch is {r}, the case is named for {want}"
        assert want <= WAVE >> slot_shift(W, thr), "the prefix is too long for this rows_per_batch"
    if name.endswith("_smallest"):
        assert rows_per_batch(n - 1, W, thr) == want // 2, "not the smallest table with this rows_per_batch"
    if name.endswith("_full"):
        assert n % r == 0 and nb == WAVE_SLOTS
    if name.endswith("_partial"):
        assert n % r == r - 1 and nb == WAVE_SLOTS + 1, "the last batch is not partial"
    if name.endswith("_stride"):
        assert nb > WAVE_SLOTS, "no second trip through the grid-stride loop"
    mixed = mixed_batches(column(lt, "cnt"), r)
    assert r == 1 or mixed >= 3, "no batch holds rows of different sizes"
    return {"rows_per_batch": r, "n_batches": nb, "mixed_batches": mixed, "second_trip": nb > WAVE_SLOTS}


def check_batch_hits(case, want):
    """Family A through the oracle: every left row hits, the planted share hits twice, and about one row in eight shares an
    id with right rows it misses."""
    p = case["premises"]
    per_row = np.bincount(want["i"], minlength=p["n_left"])
    assert np.array_equal(per_row, np.where(p["two_hits"], 2, 1)), "a left row does not hit exactly its planted right rows"
    assert 0.1 < p["near_miss"].mean() < 0.15
    shared = (case["left"] == 0).any(axis=1)  # id 0, the hub rows' first id
    assert np.array_equal(shared, p["near_miss"]) and (per_row[shared] <= 2).all()


def check_levels_batch(case, lt, rt):
    """Family B: the built left table keeps the input order, so batch b holds the items b * kRows ..; the batch count sits
    below, at or above the 8192 wave slots as the name says."""
    W, n, name = case["width"], case["premises"]["n_left"], case["name"]
    assert lt.n == n and np.array_equal(column(lt, "orig"), np.arange(n)), "the builder moved rows: batch membership is off"
    assert 64 <= rt.n <= 192 and rt.post is not None and int(column(lt, "ids").max()) < 4096
    nb = levels_n_batches(n, W)
    k = WAVE // W
    if "_below_" in name:
        assert n == WAVE_SLOTS * k - 1 and nb <= WAVE_SLOTS
    if "_at_" in name:
        assert n == WAVE_SLOTS * k and nb == WAVE_SLOTS
    if "_above_" in name:  # batches 8192 and 8193 exist; the last one holds a single row
        assert nb == WAVE_SLOTS + 2 and n - (nb - 1) * k == 1, "no second trip through the grid-stride loop"
        assert case["premises"]["planted_batches"] == [0, WAVE_SLOTS - 1, WAVE_SLOTS, WAVE_SLOTS + 1]
    if case.get("partition"):
        assert lt.seg is not None and int((np.diff(column(lt, "seg_start")) > 0).sum()) == 4, "not several category segments"
        assert rt.n > B_RIGHT
    else:
        assert lt.seg is None
    return {"n_batches": nb, "second_trip": nb > WAVE_SLOTS}


def check_levels_batch_hits(case, want):
    k = WAVE // case["width"]
    hit_batches = set((np.unique(want["i"]) // k).tolist())
    assert hit_batches == set(case["premises"]["planted_batches"]), "hits outside / missing in the planted batches"
    assert len(want) >= len(case["premises"]["planted_rows"]) // 2


def check_prefix(case, lt, rt):
    """Family C: the planted first common ids reach the last slot the prefix admits, for every size on both sides, and the
    right positions cover every posting class the launch reads."""
    W, thr, p = case["width"], case["thr"], case["premises"]
    P, _ = prefix(W, thr)
    assert lt.n == 2 * len(p["pairs"]) and rt.n == len(p["pairs"]) and rt.post is not None
    for side, col in (("left_pos", 0), ("right_pos", 1)):
        for size in range(1, W + 1):
            at = p[side][p["pairs"][:, col] == size]
            if P[size] == 0:
                assert len(at) == 0
            else:
                assert len(at) and int(at.max()) == P[size] - 1, f"{side}: size {size} never reaches its last prefix slot"
    classes = {posting_class(int(v)) for v in p["right_pos"]}
    assert classes == set(range(cls_end(W, thr))), f"posting classes {classes}, the launch reads {cls_end(W, thr)}"
    return {"cls_end": cls_end(W, thr), "longest": longest(W, thr), "pairs": len(p["pairs"])}


def check_prefix_hits(case, want):
    k = np.arange(len(case["premises"]["pairs"]))
    assert np.array_equal(np.sort(want["i"]), 2 * k), "a planted pair at kmin is not a hit, or one below kmin is"
    assert np.array_equal(want["j"][np.argsort(want["i"])], k)


def check_cluster(case, lt, rt):
    """Family D: what the model counts for the tile's table (the first pass of a dense tile)."""
    W, p = case["width"], case["premises"]
    rids, rcnt = column(rt, "ids"), column(rt, "cnt")
    assert rt.n == 64 and is_dense(int(rcnt.sum()), W) == p["dense"], f"{int(rcnt.sum())} ids: the tile is on the wrong side"
    rows = rids[:32] if p["dense"] else rids
    m = cluster_premises(rows[rows >= 0], p["absent"], W)
    assert m["homed_in_last_four"] >= 100 and m["run_length"] >= m["homed_in_last_four"]
    assert m["displaced_past_wrap"] >= 20 and m["absent_passing_before_wrap"] >= 20 and m["absent_failing"] >= 20
    assert np.isin(p["absent"], column(lt, "ids")).all(), "an absent id is in no left row"
    if case["kind"] == "raw":
        assert rt.post is None
    else:
        assert int(max(column(lt, "ids").max(), rids.max())) < 65536
    return m


def check_dense(case, lt, rt):
    """Family E: the id totals of the tiles, read from the built cnt column."""
    W, p, variant = case["width"], case["premises"], case["name"].split("_")[-1]
    cnt = column(rt, "cnt")
    assert np.array_equal(column(rt, "orig"), np.arange(rt.n)), "the builder moved rows: the planted lanes are off"
    T = index_slots(W)
    totals = [int(cnt[t: t + 64].sum()) for t in range(0, rt.n, 64)]
    if variant == "at":
        assert totals == [3 * T // 4] and not is_dense(totals[0], W)
    elif variant == "over":
        assert totals == [3 * T // 4 + 1] and is_dense(totals[0], W)
    else:
        assert totals == [64 * W, 49 * W] and is_dense(totals[1], W) and rt.n - 64 - 32 == 17, "second pass: not 17 lanes"
        assert not is_dense(33 * W, W), "a partial tile of 33 rows is dense after all"
    return {"totals": totals}


def check_dense_hits(case, want):
    p = case["premises"]
    first = 64 * p["tile"]
    hit_lanes = set((want["j"][want["j"] >= first] - first).tolist())
    assert set(p["lanes"]) <= hit_lanes and {5, 40} <= set((want["j"][want["i"] == 4] - first).tolist())
    left, right = (case["left"], case["right"]) if case["kind"] == "raw" else (case["left"][0], case["right"][0])
    shared = np.isin(left, right[right >= 0]).any(axis=1)
    assert shared.sum() > len(np.unique(want["i"])), "no left row shares an id with the table and misses the threshold"


def queue_geometry(case, lt, rt, kernel):
    """Family F: (rows of the built left table that are candidates of lane X, the wave ranges of ``kernel``)."""
    W, p, thr = case["width"], case["premises"], case["thr"]
    assert np.array_equal(column(rt, "orig")[:64], np.arange(64)) or case.get("partition"), "the planted lane moved"
    lane = int(np.flatnonzero(column(rt, "orig") == p["lane"])[0])
    lids = column(lt, "ids")
    part = bool(case.get("partition"))
    if kernel == "index":
        cand = shares_id(lids, column(rt, "ids")[lane])
        if part:
            ss = column(lt, "seg_start")
            ranges = [rg for c in range(64) if ss[c + 1] > ss[c]
                      for rg in lev_index_wave_ranges(int(ss[c]), int(ss[c + 1]), lev_index_slices(lt.n, rt.n, True), W)]
        else:
            ranges = lev_index_wave_ranges(0, lt.n, lev_index_slices(lt.n, rt.n), W)
    else:
        cand = levels_filter_pass(column(lt, "filt"), column(rt, "filt")[lane], thr)
        if part:
            cand &= (column(lt, "cat").view(np.uint64) & column(rt, "cat").view(np.uint64)[lane]) != 0
        chunk = lev_rows_per_chunk(lt.n, (rt.n + 63) // 64, part)
        ranges = [(a, min(lt.n, a + chunk)) for a in range(0, lt.n, chunk)]
    return np.flatnonzero(cand), ranges


def check_queue(case, lt, rt, kernel, straddle=False):
    """Family F: lane X receives exactly c candidates -- inside one wave's row range, or across the boundary of two."""
    p = case["premises"]
    rows, ranges = queue_geometry(case, lt, rt, kernel)
    assert len(rows) == p["depth"], f"{len(rows)} candidates for the lane, the case is named for {p['depth']}"
    assert np.array_equal(rows, p["first"] + np.arange(p["depth"])), "the candidates are not where the case puts them"
    inside = [rg for rg in ranges if rg[0] <= rows[0] and rows[-1] < rg[1]]
    if straddle:
        assert not inside and any(rows[0] < rg[0] <= rows[-1] for rg in ranges), "the candidates do not straddle a boundary"
    else:
        assert len(inside) == 1, "the candidates are not inside one wave's row range"
    if p["all_lanes"]:
        for lane in (0, 31, 63):
            q = dict(case, premises=dict(p, lane=lane))
            assert np.array_equal(queue_geometry(q, lt, rt, kernel)[0], rows), "a lane's queue is not as deep as lane X's"
    return {"rows": (int(rows[0]), int(rows[-1])), "ranges": ranges[:8]}


def check_queue_hits(case, want):
    p = case["premises"]
    c = p["depth"]
    on_lane = want[want["j"] == p["lane"]] if not p["all_lanes"] else want
    assert len(on_lane) == c - c // 2 and c // 2 > 0, "copies that hit / near copies that fail the exact score"
    assert len(want) == c - c // 2


def check_runs(case, lt, rt):
    """Family G: the run lengths of the left size classes inside the first chunk, from the built cnt column."""
    W, thr, p = case["width"], case["thr"], case["premises"]
    cnt, rcnt = column(lt, "cnt"), column(rt, "cnt")
    chunk = jac_rows_per_chunk(lt.n, (rt.n + 63) // 64)
    assert chunk == 128 and lt.n > chunk
    runs = {}
    for size, n in p["runs"].items():
        at = np.flatnonzero(cnt == size)
        assert len(at) == n and (n == 0 or (at[-1] - at[0] == n - 1)), f"size {size}: not one run of {n} rows"
        if n:
            runs[size] = (int(at[0]), int(at[-1]))
    assert {n for s, n in p["runs"].items() if s != p["cut_size"]} == set(G_RUNS)
    assert all(b < chunk for s, (a, b) in runs.items() if s != p["cut_size"]), "a run leaves the first chunk"
    a, b = runs[p["cut_size"]]
    assert a < chunk <= b, "the chunk boundary cuts no size class"
    assert not any(weak(W, thr, int(x), int(y)) for x in np.unique(cnt) for y in np.unique(rcnt)), "a size pair is weak: no prune"
    return {"runs": runs, "chunk": chunk}


def check_runs_hits(case, want, lt, runs):
    orig = column(lt, "orig")
    hit = set(want["i"].tolist())
    for size, (a, b) in runs.items():
        assert int(orig[a]) in hit and int(orig[b]) in hit, f"size {size}: no hit in the first / last row of its run"
    assert len(hit) < lt.n


def queue_straddle_cases(W, c=33):
    """(kernel whose boundary is straddled, case): c candidates across the first quarter's end of the index kernel, across
    the first chunk's end of the signature kernel, and -- with a category partition -- inside a segment that the chunk's end
    cuts.  The boundaries come from the model."""
    n = 600
    quarter_end = lev_index_wave_ranges(0, n, lev_index_slices(n, 64), W)[0][1]
    chunk = lev_rows_per_chunk(n, 1)
    return [("index", queue_case(W, c, "alone", front=quarter_end - c // 2, n_left=n)),
            ("signature", queue_case(W, c, "alone", front=chunk - c // 2, n_left=n)),
            ("signature", queue_case(W, c, "alone", front=lev_rows_per_chunk(1000, 1, True) - 300 - c // 2, n_left=1000, cut=True))]


def build_right(case, device, index=None, compact=True):
    """The right table alone (another posting format, or no global index, beside an already built left table)."""
    from napkon_string_matching_amd import tables

    W = case["width"]
    keep = tables.COMPACT_POSTINGS
    tables.COMPACT_POSTINGS = bool(compact)
    try:
        if case["kind"] == "raw":
            return tables.SetTable.from_padded(case["right"], "right", device, width=W, validate=False, index=index)
        ri, rp, rn = case["right"]
        return tables.SetTable.from_nested_arrays(ri, rp, rn, "right", device, categories=case.get("rcat"), width=W,
                                                  category_mode=case.get("mode", CAT_NONE),
                                                  partition=case.get("partition", False), index=index)
    finally:
        tables.COMPACT_POSTINGS = keep
