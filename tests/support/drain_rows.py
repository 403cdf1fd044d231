"""Host-side model of the stack entries and the drain of the two-stage RAW fuzzy kernel (csrc/indel_raw_coarse.hpp), and
the inputs of tests/test_cpu_indel_raw_drain_rows.py and tests/test_gpu_indel_raw_drain_rows.py.

The scan pushes one entry per LANE whose folded result passes: the lane holds 16 rows of a block of 32 left rows,
(k & 3) + 8 (k >> 2) + 4 (lane >> 5) for k = 0 .. 15, against right string tile * 32 + (lane & 31) of its wave.  An entry is

    high word   (block's first row - chunk's first row) << 15 | la << 8 | tile << 6 | lane
    low word    the number of rows of the block that exist, min(32, class or chunk end - block's first row)

and the drain runs the exact 32-bucket test (min(la, lb) >= need and L1 <= la + lb - 2 need) on the rows of the entry that
exist.  Everything here is restated from that description in plain Python: nothing is read from the library.

The strings are SORTED RUNS over at most 32 symbols, one histogram bucket each, so that LCS = sum of the bucket minima and a
pair can be put exactly at need or at need - 1.
"""
import itertools
import random

SYMS = "".join(sorted("abcdefghijklmnopqrstuvwxyzABCDEF"))  # 32 symbols
NT, CAP, BLOCK, WAVE = 4, 3, 32, 64
RIGHTS = NT * BLOCK           # right strings per wave
DRAIN_AT = 2 * WAVE           # the drain runs when MORE than this many entries wait at a check
STACK = (NT + 3) * WAVE       # entries the stack has room for
NEVER = 255


def runs(counts):
    """c0^a0 c1^a1 ... over SYMS (ascending)."""
    assert len(counts) <= 32
    return "".join(s * a for s, a in zip(SYMS, counts))


def counts(x):
    return [x.count(s) for s in SYMS]


def need(thr, s):
    """The smallest LCS with which strings of la + lb = s reach ``thr`` (csrc/indel_score.hpp, the same doubles), or NEVER."""
    if s < 2 or s > 128:
        return NEVER
    for lcs in range(s // 2 + 1):
        if (1.0 - float(s - 2 * lcs) / float(s)) * 100.0 / 100.0 >= thr:
            return lcs
    return NEVER


def need_of(thr, la, lb):
    if la == 0 or lb == 0:
        return 0 if 0.0 >= thr else NEVER
    return need(thr, la + lb)


# --- the entry and the rows of a lane --------------------------------------------------------------------------------------


def pack_entry(row_rel, la, tile, lane, n_rows):
    assert 0 <= row_rel < (1 << 15) and 0 <= la <= 64 and 0 <= tile < NT and 0 <= lane < WAVE and 1 <= n_rows <= BLOCK
    return (row_rel << 15) | (la << 8) | (tile << 6) | lane, n_rows


def unpack_entry(hi, lo):
    """(row_rel, la, tile, lane, n_rows)"""
    return hi >> 15, (hi >> 8) & 127, (hi >> 6) & 3, hi & 63, lo


def lane_row(lane, k):
    """Row of the block behind bit k of a lane's mask (the C layout of the 32x32 MFMA)."""
    return (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5)


def drain_rows(lane, n_rows):
    """The rows of the block whose verdict the drain keeps for an entry of scan lane ``lane``: drain lane m = 0 .. 3 of the
    entry's four has rows 8 g + 4 (lane >> 5) + m, g = 0 .. 3, and drops those at or past the entry's row count."""
    return [8 * g + 4 * (lane >> 5) + m for m in range(4) for g in range(4) if 8 * g + 4 * (lane >> 5) + m < n_rows]


def place(e, g, m):
    """(drain lane, bit of its mask) of row 8 g + 4 eh + m of the e-th entry of a pass: quarter e >> 4 of the pass, lanes
    4 (e & 15) .. + 3."""
    return 4 * (e & 15) + m, 4 * (e >> 4) + g


def walk_decode(lane, pos, scan_lane):
    """What the LCS walk makes of bit ``pos`` of drain lane ``lane``: (entry of the pass, row of its block), the entry's scan
    lane (read again from the stack) giving the lane half."""
    return 16 * (pos >> 2) + (lane >> 2), 8 * (pos & 3) + 4 * (scan_lane >> 5) + (lane & 3)


# --- the launch geometry -----------------------------------------------------------------------------------------------------


def rows_per_chunk(n_left, n_right):
    """csrc/indel_raw.hip: pick_rows_per_chunk, rounded up to whole blocks."""
    n_tiles = (n_right + RIGHTS - 1) // RIGHTS
    chunks = max(1, (16 * 256 * 32 + n_tiles - 1) // n_tiles)
    rows = min(4096, max(64, (n_left + chunks - 1) // chunks))
    return (rows + BLOCK - 1) // BLOCK * BLOCK


def table_order(strings):
    """Rows of a string table: length descending, ties in input order."""
    return sorted(range(len(strings)), key=lambda i: -len(strings[i]))


# --- the kernel, pair by pair ------------------------------------------------------------------------------------------------


class Model:
    """What the kernel does with ``left`` x ``right`` at ``thr``, in table rows: ``entries`` (wave, chunk, hi, lo),
    ``lcs_pairs`` [(row, right row)] in the order of the drain's enumeration, one per LCS call, ``fold_lanes`` the plain
    description of the same lanes for the test's own loop, and ``waiting`` the stack's level at every drain check."""

    def __init__(self, left, right, thr):
        assert len(set("".join(left) + "".join(right))) <= 32  # one bucket per symbol, whichever code it gets
        self.thr = thr
        self.lorder, self.rorder = table_order(left), table_order(right)
        self.lrows = [left[i] for i in self.lorder]
        self.rrows = [right[j] for j in self.rorder]
        self.lh = [counts(x) for x in self.lrows]
        self.rh = [counts(y) for y in self.rrows]
        self.chunk_rows = rows_per_chunk(len(left), len(right))
        self.entries, self.lcs_pairs, self.fold_lanes, self.waiting = [], [], [], []
        for wave in range((len(right) + RIGHTS - 1) // RIGHTS):
            for chunk in range((len(left) + self.chunk_rows - 1) // self.chunk_rows):
                self._wave(wave, chunk)

    def coarse(self, row, j):
        """The scan's bound D of a pair (per bucket min(a, r) where r < CAP, a where r >= CAP)."""
        return sum(min(a, r) if r < CAP else a for a, r in zip(self.lh[row], self.rh[j]))

    def exact(self, row, j):
        la, lb = len(self.lrows[row]), len(self.rrows[j])
        nd = need_of(self.thr, la, lb)
        l1 = sum(abs(a - r) for a, r in zip(self.lh[row], self.rh[j]))
        return min(la, lb) >= nd and l1 <= la + lb - 2 * nd

    def _wave(self, wave, chunk):
        i0 = chunk * self.chunk_rows
        i1 = min(len(self.lrows), i0 + self.chunk_rows)
        j0 = wave * RIGHTS
        q = 0
        stack = []
        lengths = sorted({len(x) for x in self.lrows[i0:i1]}, reverse=True)
        for la in lengths:
            a = max(i0, min(i for i, x in enumerate(self.lrows) if len(x) == la))
            b = min(i1, 1 + max(i for i, x in enumerate(self.lrows) if len(x) == la))
            nm = {}  # right row -> need of the class, where the lengths fit
            for j in range(j0, min(j0 + RIGHTS, len(self.rrows))):
                nd = need_of(self.thr, la, len(self.rrows[j]))
                if min(la, len(self.rrows[j])) >= nd:
                    nm[j] = nd
            if not nm:
                continue
            self.waiting.append(q)  # the check at the start of a class
            if q > DRAIN_AT:
                q = self._drain(stack, q % WAVE)
            for i in range(a, b, BLOCK):
                flush = False
                for t in range(NT):
                    if t == NT - 1:  # the check in front of a block's last tile, whose entries are still pushed
                        self.waiting.append(q)
                        flush = q > DRAIN_AT
                    for lane in range(WAVE):
                        j = j0 + t * BLOCK + (lane & 31)
                        if j not in nm:
                            continue
                        rows = [min(i + lane_row(lane, k), b - 1) for k in range(16)]  # (the last row again past the end)
                        if any(self.coarse(row, j) >= nm[j] for row in rows):
                            stack.append((wave, chunk, *pack_entry(i - i0, la, t, lane, min(BLOCK, b - i))))
                            self.fold_lanes.append((i, min(i + BLOCK, b), lane >> 5, j))
                            q += 1
                    assert q <= STACK
                if flush:
                    q = self._drain(stack, q % WAVE)
        self._drain(stack, 0)

    def _drain(self, stack, keep):
        """Full passes from the top of the stack until ``keep`` entries are left."""
        while len(stack) > keep:
            n = min(len(stack), WAVE)
            batch, stack[len(stack) - n:] = stack[len(stack) - n:], []
            masks = [0] * WAVE  # the drain lanes' masks of the pass
            for e, (wave, chunk, hi, lo) in enumerate(batch):
                self.entries.append((wave, chunk, hi, lo))
                row_rel, la, tile, lane, n_rows = unpack_entry(hi, lo)
                j = wave * RIGHTS + tile * BLOCK + (lane & 31)
                for g, m in itertools.product(range(4), range(4)):
                    r = 8 * g + 4 * (lane >> 5) + m
                    if r < n_rows and self.exact(chunk * self.chunk_rows + row_rel + r, j):
                        dl, bit = place(e, g, m)
                        masks[dl] |= 1 << bit
            for dl in range(WAVE):  # the LCS walk: lane by lane, a lane's bits from the highest down
                for pos in range(15, -1, -1):
                    if (masks[dl] >> pos) & 1:
                        wave, chunk, hi, lo = batch[16 * (pos >> 2) + (dl >> 2)]
                        row_rel, la, tile, lane, n_rows = unpack_entry(hi, lo)
                        e, r = walk_decode(dl, pos, lane)
                        row = chunk * self.chunk_rows + row_rel + r
                        assert batch[e] == (wave, chunk, hi, lo) and r < n_rows and len(self.lrows[row]) == la
                        self.lcs_pairs.append((row, wave * RIGHTS + tile * BLOCK + (lane & 31)))
        return keep

    def hits(self):
        """The pairs of ``lcs_pairs`` whose LCS (sorted runs: the sum of the bucket minima) reaches need, as (left, right)
        input indices."""
        out = []
        for row, j in self.lcs_pairs:
            nd = need_of(self.thr, len(self.lrows[row]), len(self.rrows[j]))
            if sum(map(min, self.lh[row], self.rh[j])) >= nd:
                out.append((self.lorder[row], self.rorder[j]))
        return out


# --- the inputs ----------------------------------------------------------------------------------------------------------------
# Tagged rows.  Symbols 0 .. 5 carry a base of 30 units that every tagged string has, symbols 6 .. 21 are the 16 positions
# p = (row >> 3) * 4 + (row & 3) of a row within its lane, symbols 22 and 23 the two lane halves (row >> 2) & 1, symbol 24
# pads left rows and symbol 25 right rows.  A left row carries its position and its half once each; a right string carries
# a SET of positions and one half (or both).  LCS = 30 + [half in common] + [position in the set]: 32 where both hold, 31 for
# the other rows of the same lane.

_BASE = [5] * 6


def tagged_left(r, pad):
    c = _BASE + [0] * 26
    c[6 + (r >> 3) * 4 + (r & 3)] = 1
    c[22 + ((r >> 2) & 1)] = 1
    c[24] = pad
    return runs(c)


def tagged_right(rows, pad, both_halves=False):
    """A right string that the rows ``rows`` (all of one lane half unless ``both_halves``) reach need with."""
    c = _BASE + [0] * 26
    halves = {(r >> 2) & 1 for r in rows}
    assert len(halves) == 1 or both_halves
    for r in rows:
        c[6 + (r >> 3) * 4 + (r & 3)] = 1
    for h in (0, 1) if both_halves else halves:
        c[22 + h] = 1
    c[25] = pad
    return runs(c)


def case_row_positions():
    """32 left rows of 40 units (one block) x 128 right strings of 40 units (four tiles); right string 32 t + c is at
    need = 32 with row (c + 5 t) % 32 alone and at need - 1 with the other 15 rows of that row's lane."""
    left = [tagged_left(r, 8) for r in range(32)]
    right = [tagged_right([(c + 5 * t) % 32], 8) for t in range(4) for c in range(32)]
    want = {((c + 5 * t) % 32, 32 * t + c) for t in range(4) for c in range(32)}
    return left, right, want


def case_many_rows():
    """32 left rows of 33 units x 40 right strings of 47 units (need 32): lanes with 2, 5 and all 16 of their rows at need
    with one right string, one right string with three rows in either lane half, the rest far from everything."""
    left = [tagged_left(r, 1) for r in range(32)]
    lanes = {0: [1, 26], 17: [0, 3, 9, 18, 27], 35: [lane_row(32, k) for k in range(16)]}
    right, want = [], set()
    for j in range(40):
        if j in lanes:
            right.append(tagged_right(lanes[j], 16 - len(lanes[j])))
            want |= {(r, j) for r in lanes[j]}
        elif j == 5:
            rows = [2, 6, 11, 15, 24, 28]
            right.append(tagged_right(rows, 16 - 3 - 1, both_halves=True))
            want |= {(r, j) for r in rows}
        else:
            right.append(SYMS[25] * 47)
    return left, right, want


def perturbed(base, rng):
    c = list(base)
    up = rng.randrange(len(c))
    down = rng.choice([s for s in range(len(c)) if s != up and c[s] > 0])
    c[up] += 1
    c[down] -= 1
    return c


def _near(length):
    c = [5] * 8
    for u in range(abs(length - 40)):
        c[u % 8] += 1 if length > 40 else -1
    return c


def _far(length, rng):
    return runs([0] * 8 + perturbed([length // 8 + (1 if u < length % 8 else 0) for u in range(8)], rng))


def case_short_blocks():
    """Length classes of 32, 31, 1, 65 and 33 rows x 33 right strings of 40 units: the LAST row of every class is near all
    of them and every other row, the second to last among them, shares no symbol with them.  In this order the chunks of 64
    rows end where blocks end anyway (after 32 + 31 + 1 rows and after 64 of the 65), so the last blocks have 32, 31, 1, 1
    and 1 rows."""
    rng = random.Random(101)
    right = [runs(perturbed([5] * 8, rng)) for _ in range(33)]
    left, hitting = [], []
    for length, rows in ((44, 32), (43, 31), (42, 1), (41, 65), (40, 33)):
        for k in range(rows):
            if k == rows - 1:
                hitting.append(len(left))
                left.append(runs(perturbed(_near(length), rng)))
            else:
                left.append(_far(length, rng))
            assert len(left[-1]) == length
    return left, right, set(itertools.product(hitting, range(33)))


def case_chunk_ends():
    """200 left rows of 40 units x 33 right strings: chunks of 64 rows, so the one class crosses three chunk ends; the last
    row before each and the first row after it are near every right string."""
    rng = random.Random(102)
    right = [runs(perturbed([5] * 8, rng)) for _ in range(33)]
    hitting = [63, 64, 127, 128, 191, 192]
    left = [runs(perturbed(_near(40), rng)) if i in hitting else _far(40, rng) for i in range(200)]
    return left, right, set(itertools.product(hitting, range(33)))


def case_ragged(n_right):
    """70 left rows of 36 .. 44 units, every third near the right strings, x 1, 33 or 129 right strings."""
    rng = random.Random(103 + n_right)
    right = [runs(perturbed(perturbed([5] * 8, rng), rng)) for _ in range(n_right)]
    left = []
    for i in range(70):
        length = 36 + i % 9
        left.append(runs(perturbed(_near(length), rng)) if i % 3 == 0 else _far(length, rng))
    return left, right


def case_zero_and_one():
    """40 x 40 with empty strings on both sides (threshold 0: every pair is a hit) and equal strings (threshold 1.0)."""
    rng = random.Random(104)
    word = lambda: runs([rng.randint(0, 2) for _ in range(32)])
    left = [word() for _ in range(37)] + ["", "", SYMS[3] * 64]
    right = ["", SYMS[3] * 64] + left[:6] + [word() for _ in range(32)]
    return left, right


def case_edge_lengths(which):
    """Right strings that fit ONE length class of the left chunk, its longest ("long": left rows of 30 .. 34 units, right
    strings of 51; need(85) = 34, need(84) = 34 > 33) or its shortest ("short": left rows of 40 .. 44 units, right strings
    of 27; need(67) = 27, need(68) = 28), and a last wave of right strings that fit none (19 and 12 units).  Every fourth
    right string contains, or is contained in, a row of the class it fits: a hit with the shorter string as the LCS."""
    rng = random.Random(106 + len(which))
    spread = lambda n: perturbed(perturbed([n // 8 + (1 if u < n % 8 else 0) for u in range(8)], rng), rng)
    lens, lb, short = ((30, 31, 32, 33, 34), 51, 19) if which == "long" else ((40, 41, 42, 43, 44), 27, 12)
    left = [runs(spread(n)) for n in lens for _ in range(9)]
    fit = [x for x in left if len(x) == (34 if which == "long" else 40)]
    right = []
    for j in range(128):
        c = counts(fit[j % len(fit)])[:8]
        if j % 4:
            c = spread(lb)
        else:
            for _ in range(abs(lb - sum(c))):
                u = rng.choice([s for s in range(8) if which == "long" or c[s] > 0])
                c[u] += 1 if which == "long" else -1
        right.append(runs(c))
        assert len(right[-1]) == lb
    return left, right + [runs(spread(short)) for _ in range(33)]


def case_four_letters():
    """96 left rows of 40 units (three blocks of one class) x 161 right strings (two waves) over four letters: most pairs
    pass the scan's bound."""
    rng = random.Random(105)
    word = lambda n: "".join(sorted(rng.choice(SYMS[:4]) for _ in range(n)))
    return [word(40) for _ in range(96)], [word(rng.randint(30, 52)) for _ in range(161)]
