"""The work items of the persistent packed scan (csrc/indel_raw_coarse.hpp: c3p_prepass_kernel and the PERSIST scan), restated
in plain Python.

Both tables are sorted by length, descending; ``lstart[c]`` is the first left row of length 64 - c (66 entries).  A right
TILE is 128 consecutive right strings.  The left lengths that fit a right string of ``lb`` units under ``lcsmin`` are
``la_lo[lb] .. la_hi[lb]`` (65 and 0: none).  A tile's left lengths are the HULL of its strings' ranges, taken over every
length between its last and its first string's; its rows are ``[lstart[64 - hi], lstart[64 - lo + 1])``.  Where empty strings
score (``zero_need == 0``) the interval is every row.  The hull may hold rows that fit nothing: the scan only relies on it
holding every row that does.

The interval is cut into WINDOWS of 2^15 rows from its first row and a window into items of at most ``item_rows`` rows;
an item is ``(tile, first row, end row, base row)``, the base its window's first row.  Items are listed in tile-major order.

A wave pulls a RANGE of consecutive items with one atomic add on the head: its grain is half of what a (possibly stale)
read of the head says is left, divided among the waves, at least one, and the range is clipped to the item count.
"""
NEVER = 255
TILE = 128
WINDOW = 1 << 15


def need_of(la, lb, lcsmin, zero_need):
    return zero_need if la == 0 or lb == 0 else lcsmin[la + lb]


def fits(la, lb, lcsmin, zero_need):
    """The scan's exact length filter: LCS <= min(la, lb)."""
    return min(la, lb) >= need_of(la, lb, lcsmin, zero_need)


def lcsmin_of(threshold):
    """lcsmin[s], s = la + lb: the smallest LCS whose Indel ratio 2 LCS / s reaches the threshold (NEVER: none)."""
    out = [NEVER] * 132
    for s in range(2, 129):
        for lcs in range(0, s // 2 + 1):
            if (1.0 - (s - 2 * lcs) / s) * 100.0 / 100.0 >= threshold:
                out[s] = lcs
                break
    return out, (0 if 0.0 >= threshold else NEVER)


def length_ranges(lcsmin):
    """(la_lo, la_hi) by right length 0 .. 64, as the host tabulates them: left lengths 1 .. 64 only."""
    lo, hi = [65] * 65, [0] * 65
    for lb in range(1, 65):
        for la in range(1, 65):
            if min(la, lb) >= lcsmin[la + lb]:
                if lo[lb] == 65:
                    lo[lb] = la
                hi[lb] = la
    return lo, hi


def tile_interval(t, rlen, lstart, n_left, lcsmin, zero_need):
    """(first row, rows) of tile t."""
    if zero_need == 0:
        return 0, n_left
    la_lo, la_hi = length_ranges(lcsmin)
    a, b = rlen[t * TILE], rlen[min(t * TILE + TILE, len(rlen)) - 1]
    a, b = min(max(a, 0), 64), min(max(b, 0), 64)
    lo, hi = 65, 0
    for lb in range(min(a, b), max(a, b) + 1):
        lo, hi = min(lo, la_lo[lb]), max(hi, la_hi[lb])
    if hi < lo:
        return 0, 0
    return lstart[64 - hi], lstart[64 - lo + 1] - lstart[64 - hi]


def items_of(rows, item_rows):
    per_window = -(-WINDOW // item_rows)
    return (rows >> 15) * per_window + -(-(rows & (WINDOW - 1)) // item_rows)


def tile_items(t, r0, rows, item_rows):
    per_window = -(-WINDOW // item_rows)
    out = []
    for k in range(items_of(rows, item_rows)):
        base = r0 + (k // per_window) * WINDOW
        first = base + (k % per_window) * item_rows
        out.append((t, first, min(first + item_rows, base + WINDOW, r0 + rows), base))
    return out


def item_list(rlen, lstart, n_left, lcsmin, zero_need, item_rows):
    assert item_rows % 32 == 0 and 0 < item_rows <= WINDOW
    out = []
    for t in range(-(-len(rlen) // TILE)):
        r0, rows = tile_interval(t, rlen, lstart, n_left, lcsmin, zero_need)
        out += tile_items(t, r0, rows, item_rows)
    return out


def guided_pulls(n_items, n_waves, order, stale=0):
    """The ranges the waves take, in the order ``order`` yields wave numbers (a wave that found the list empty is done and
    is skipped); ``stale``: how far behind the head a wave's plain read of it is.  Returns {wave: [(start, end), ...]}."""
    head, done, taken = 0, set(), {}
    for w in order:
        if w in done:
            if len(done) == n_waves:
                break
            continue
        seen = max(0, head - stale)
        left = n_items - seen if seen < n_items else 0
        grain = max(1, left // (2 * n_waves))
        start, head = head, head + grain
        if start >= n_items:
            done.add(w)
            continue
        taken.setdefault(w, []).append((start, min(start + grain, n_items)))
    assert len(done) == n_waves, "every wave must reach the end of the list"
    return taken
