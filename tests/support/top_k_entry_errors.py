"""Malformed calls to the six ``nsm_*_top_k*`` entries, made without a device: every call here ends in the argument
checks (or at an empty side), before any allocation or launch.  The test modules hold the tables of cases with the exact
(status, ``nsm_last_error()``) each one answers; which check speaks first when two faults meet is part of the ABI."""
import ctypes

OK, BADARG, UNSUPPORTED = 0, 10001, 10002
FAKE = 16  # column pointers are never dereferenced on the host
NULL = None  # (as a table: a null struct pointer)


def _struct(cls, defaults, over):
    if over is NULL:
        return None
    return cls(**{**defaults, **over})


def str_table(over):
    from napkon_string_matching_amd import _lib

    return _struct(_lib.NsmStrTable, dict(codes=FAKE, len=FAKE, orig=FAKE, len_start=FAKE, n=5000, stride=64, alphabet=10), over)


def set_table(over):
    from napkon_string_matching_amd import _lib

    return _struct(_lib.NsmSetTable, dict(ids=FAKE, cnt=FAKE, orig=FAKE, size_start=FAKE, nlev=FAKE, plen=FAKE, n=5000, width=16,
                                          max_levels=4), over)


def level_items(over):
    from napkon_string_matching_amd import _lib

    return _struct(_lib.NsmLevelItems, dict(first=FAKE, nlev=FAKE, orig=FAKE, n=5000), over)


def call(entry, k=3, left={}, right={}, left_strings={}, right_strings={}, group=FAKE, category_mode=0, banned=(None, None),
         out=True, out_count=True):
    """(status, message) of ``entry`` on tables that are valid but for the given overrides (a dict of struct fields, or
    NULL for a null table pointer).  The message of a call that succeeds is None (``nsm_last_error()`` is then stale)."""
    from napkon_string_matching_amd import _lib

    lib = _lib.load()
    hit, cnt = _lib.NsmHit(), ctypes.c_ulonglong(0)
    tail = (ctypes.addressof(hit) if out else None, ctypes.addressof(cnt) if out_count else None, None, None)
    if entry.startswith("nsm_indel_raw"):
        args = (str_table(left), str_table(right)) + ((group,) if entry.endswith("grouped") else ()) + (0.5, k, 1)
    elif entry.startswith("nsm_jaccard_raw"):
        args = (set_table(left), set_table(right)) + ((group,) if entry.endswith("grouped") else ()) + (0.5, k, 1)
    elif entry == "nsm_indel_levels_top_k":
        args = (level_items(left), str_table(left_strings), level_items(right), str_table(right_strings), 0.5, k, category_mode,
                1) + tuple(banned)
    else:
        args = (set_table(left), set_table(right), 0.5, k, category_mode, 1) + tuple(banned)
    rc = getattr(lib, entry)(*args, *tail)
    assert cnt.value == 0
    return rc, (lib.nsm_last_error().decode() if rc else None)


def check_table(entries, cases):
    """``cases``: (label, keyword arguments of ``call``, status, message with ``{who}`` for the entry's name)."""
    for entry in entries:
        for label, kw, status, message in cases:
            want = (status, None if message is None else message.format(who=entry))
            assert call(entry, **kw) == want, (entry, label)
