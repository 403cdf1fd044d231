"""ctypes binding of ``libnsm_hip.so`` (C ABI: include/nsm_hip.h).  Fails loudly."""
import ctypes
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("NSM_HIP_LIBRARY", _HERE.parent / "csrc" / "libnsm_hip.so"))

ABI_VERSION = 5
FLAG_PRUNE = 1
FLAG_WAVE_WIDE = 2  # nsm_indel_levels_grid without the block-cooperative parking (A/B runs, tests)
FLAG_INDEX, FLAG_NO_INDEX = 4, 8  # nsm_jaccard_raw_grid: force / forbid the inverted-index kernels
FLAG_TILE_INDEX = 64  # with FLAG_INDEX: the per-tile LDS index even when the right table carries a global one
FLAG_RAW_SCORE = 32  # nsm_*_any_grid: the RAW plugin call instead of compare_terms
FLAG_ONE_STAGE = 1024  # nsm_indel_raw_grid: the 32-bucket histogram test for every pair (not the two-stage kernel)
FLAG_PACK, FLAG_NO_PACK = 2048, 4096  # nsm_indel_raw_grid, two-stage: force / forbid the once-per-call left operand words
FLAG_ONE_GROUP = 8192  # nsm_indel_raw_grid, where it packs: the persistent (item-pulling) scan, ONE workgroup (tests)
FLAG_SPLIT, FLAG_TILE, FLAG_PROBE = 128, 256, 512 # nsm_indel_levels_grid, one-word strings: force the split path / the tile kernel; scan only
FLAG_PARK = 16  # nsm_indel_levels_grid, strings > 64 code units: the round-2 park kernel instead of the shared-tile kernel
BUILD_PARTITION, BUILD_VALIDATE, BUILD_SORT = 1, 2, 4
ASSIGN_ROUNDS_ONLY, ASSIGN_STREAM_ONLY = 1, 2  # nsm_assign_hits (include/nsm_hip_assign.h): one stage only (A/B runs, tests)
GROUP_CONTINUE = 1  # nsm_group_hits (include/nsm_hip_groups.h): `label` holds a forest, link the lists into it
SPAN_NO_COMPACT = 1  # nsm_span_hits (include/nsm_hip_span.h): every round visits every edge (accepted; the only route)
CAT_NONE, CAT_INTERSECT, CAT_INTERSECT_OR_BOTH_EMPTY = 0, 1, 2
# include/nsm_hip_measures.h: the token-set measure of the nsm_set_* entries
MEASURE_UNION, MEASURE_MEAN, MEASURE_SMALLER, MEASURE_LEFT = 0, 1, 2, 3
MEASURES = {"union": MEASURE_UNION, "mean": MEASURE_MEAN, "smaller": MEASURE_SMALLER, "left": MEASURE_LEFT}
# include/nsm_hip_edit.h: the string metric of the nsm_edit_* entries
METRIC_INDEL, METRIC_EDIT, METRIC_EDIT_WITHIN = 0, 1, 2
METRICS = {"indel": METRIC_INDEL, "edit": METRIC_EDIT, "edit_within": METRIC_EDIT_WITHIN}

c_i32p = ctypes.c_void_p  # device pointers travel as integers
c_u64 = ctypes.c_uint64


class NsmHit(ctypes.Structure):
    _fields_ = [("score", ctypes.c_double), ("i", ctypes.c_int32), ("j", ctypes.c_int32)]


class NsmHitList(ctypes.Structure):
    _fields_ = [("hits", ctypes.c_void_p), ("n", ctypes.c_uint64), ("left_base", ctypes.c_int32), ("left_ids", ctypes.c_int32),
                ("right_base", ctypes.c_int32), ("right_ids", ctypes.c_int32)]


class NsmSetTable(ctypes.Structure):
    _fields_ = [
        ("ids", ctypes.c_void_p),
        ("cnt", ctypes.c_void_p),
        ("sig", ctypes.c_void_p),
        ("sig2", ctypes.c_void_p),
        ("orig", ctypes.c_void_p),
        ("size_start", ctypes.c_void_p),
        ("nlev", ctypes.c_void_p),
        ("plen", ctypes.c_void_p),
        ("cat", ctypes.c_void_p),
        ("filt", ctypes.c_void_p),
        ("seg", ctypes.c_void_p),
        ("seg_start", ctypes.c_void_p),
        ("n", ctypes.c_int32),
        ("width", ctypes.c_int32),
        ("max_levels", ctypes.c_int32),
        ("vocab", ctypes.c_int32),
        ("post", ctypes.c_void_p),
        ("post_start", ctypes.c_void_p),
        ("post_sq", ctypes.c_uint64 * 5),
        ("post_row_bits", ctypes.c_int32),
        ("post_format", ctypes.c_int32),
    ]


class NsmStrTable(ctypes.Structure):
    _fields_ = [
        ("codes", ctypes.c_void_p),
        ("len", ctypes.c_void_p),
        ("orig", ctypes.c_void_p),
        ("len_start", ctypes.c_void_p),
        ("hist", ctypes.c_void_p),
        ("n", ctypes.c_int32),
        ("stride", ctypes.c_int32),
        ("alphabet", ctypes.c_int32),
        ("hist16", ctypes.c_void_p),
    ]


class NsmAnyStrings(ctypes.Structure):
    _fields_ = [("codes", ctypes.c_void_p), ("offset", ctypes.c_void_p), ("n_rows", ctypes.c_int32),
                ("alphabet", ctypes.c_int32), ("max_len", ctypes.c_int32)]


class NsmAnyItems(ctypes.Structure):
    _fields_ = [("first", ctypes.c_void_p), ("nlev", ctypes.c_void_p), ("orig", ctypes.c_void_p), ("cat", ctypes.c_void_p),
                ("n", ctypes.c_int32)]


class NsmAnySets(ctypes.Structure):
    _fields_ = [("ids", ctypes.c_void_p), ("lv", ctypes.c_void_p), ("offset", ctypes.c_void_p), ("nlev", ctypes.c_void_p),
                ("plen", ctypes.c_void_p), ("orig", ctypes.c_void_p), ("cat", ctypes.c_void_p), ("n", ctypes.c_int32),
                ("max_levels", ctypes.c_int32), ("max_ids", ctypes.c_int32), ("first", ctypes.c_void_p)]


class NsmLevelItems(ctypes.Structure):
    _fields_ = [
        ("first", ctypes.c_void_p),
        ("nlev", ctypes.c_void_p),
        ("orig", ctypes.c_void_p),
        ("cat", ctypes.c_void_p),
        ("seg", ctypes.c_void_p),
        ("seg_start", ctypes.c_void_p),
        ("n", ctypes.c_int32),
    ]


EXPORTS = (
    "nsm_abi_version",
    "nsm_last_error",
    "nsm_jaccard_raw_grid",
    "nsm_jaccard_levels_grid",
    "nsm_indel_raw_grid",
    "nsm_indel_levels_grid",
    "nsm_indel_levels_workspace_bytes",
    "nsm_release",
    "nsm_release_all",
    "nsm_sort_hits",
    "nsm_build_set_table",
    "nsm_build_str_table",
    "nsm_build_level_items",
    "nsm_indel_any_grid",
    "nsm_jaccard_any_grid",
    "nsm_indel_raw_top_k",
    "nsm_jaccard_raw_top_k",
    "nsm_indel_levels_top_k",
    "nsm_jaccard_levels_top_k",
    "nsm_indel_raw_top_k_grouped",
    "nsm_jaccard_raw_top_k_grouped",
    "nsm_indel_raw_profile",
    "nsm_jaccard_raw_profile",
    "nsm_indel_levels_profile",
    "nsm_jaccard_levels_profile",
    "nsm_indel_raw_pairs",
    "nsm_jaccard_raw_pairs",
    "nsm_indel_levels_pairs",
    "nsm_jaccard_levels_pairs",
    "nsm_indel_raw_floor_grid",
    "nsm_jaccard_raw_floor_grid",
    "nsm_indel_levels_floor_grid",
    "nsm_jaccard_levels_floor_grid",
)

# include/nsm_hip_assign.h: additive entries, bound when the library has them (a call without one raises NsmLibraryError)
ASSIGN_EXPORTS = ("nsm_assign_hits",)
# include/nsm_hip_groups.h, likewise
GROUP_EXPORTS = ("nsm_group_hits",)

# include/nsm_hip_span.h, likewise
SPAN_EXPORTS = ("nsm_span_hits",)
# include/nsm_hip_measures.h, likewise: every nsm_jaccard_* per-item entry with `measure` after `right`
MEASURE_EXPORTS = (
    "nsm_set_raw_top_k",
    "nsm_set_raw_top_k_grouped",
    "nsm_set_raw_profile",
    "nsm_set_raw_floor_grid",
    "nsm_set_raw_pairs",
    "nsm_set_levels_top_k",
    "nsm_set_levels_profile",
    "nsm_set_levels_floor_grid",
    "nsm_set_levels_pairs",
)

# include/nsm_hip_edit.h, likewise: every nsm_indel_* per-item entry with `metric` after the tables
EDIT_EXPORTS = (
    "nsm_edit_raw_top_k",
    "nsm_edit_raw_top_k_grouped",
    "nsm_edit_raw_profile",
    "nsm_edit_raw_floor_grid",
    "nsm_edit_raw_pairs",
    "nsm_edit_levels_top_k",
    "nsm_edit_levels_profile",
    "nsm_edit_levels_floor_grid",
    "nsm_edit_levels_pairs",
)

# include/nsm_hip_support.h, likewise
SUPPORT_EXPORTS = ("nsm_support_hits",)

_lib = None


class NsmLibraryError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load the in-tree HIP library once.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NsmLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the match loop."
        )
    lib = ctypes.CDLL(str(LIB_PATH))
    lib.nsm_abi_version.restype = ctypes.c_int
    lib.nsm_last_error.restype = ctypes.c_char_p
    if lib.nsm_abi_version() != ABI_VERSION:
        raise NsmLibraryError(f"{LIB_PATH}: ABI {lib.nsm_abi_version()} != expected {ABI_VERSION}")
    P = ctypes.POINTER
    grid_tail = [ctypes.c_void_p, c_u64, ctypes.c_void_p, ctypes.c_void_p]  # hits, capacity, hit_count, stream
    lib.nsm_jaccard_raw_grid.argtypes = [P(NsmSetTable), P(NsmSetTable), ctypes.c_double, ctypes.c_uint32] + grid_tail
    lib.nsm_jaccard_levels_grid.argtypes = [
        P(NsmSetTable), P(NsmSetTable), ctypes.c_double, ctypes.c_int32, ctypes.c_uint32] + grid_tail
    lib.nsm_indel_raw_grid.argtypes = [P(NsmStrTable), P(NsmStrTable), ctypes.c_double, ctypes.c_uint32] + grid_tail
    # hits, capacity, hit_count, workspace, workspace_bytes, expected_survivors, stream
    lib.nsm_indel_levels_grid.argtypes = [
        P(NsmLevelItems), P(NsmStrTable), P(NsmLevelItems), P(NsmStrTable),
        ctypes.c_double, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, c_u64, ctypes.c_void_p, ctypes.c_void_p, c_u64,
        ctypes.c_double, ctypes.c_void_p]
    lib.nsm_indel_levels_workspace_bytes.argtypes = [
        P(NsmLevelItems), P(NsmStrTable), P(NsmLevelItems), P(NsmStrTable), ctypes.c_double, ctypes.c_uint32, ctypes.c_double]
    lib.nsm_release.argtypes = [ctypes.c_void_p]
    lib.nsm_release_all.argtypes = []
    lib.nsm_indel_any_grid.argtypes = [
        P(NsmAnyItems), P(NsmAnyStrings), P(NsmAnyItems), P(NsmAnyStrings), ctypes.c_double, ctypes.c_int32,
        ctypes.c_uint32] + grid_tail
    lib.nsm_jaccard_any_grid.argtypes = [P(NsmAnySets), P(NsmAnySets), ctypes.c_double, ctypes.c_int32, ctypes.c_uint32] + grid_tail
    # threshold, k, flags, out, out_count, stats, stream
    top_k_tail = [ctypes.c_double, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_void_p]
    lib.nsm_indel_raw_top_k.argtypes = [P(NsmStrTable), P(NsmStrTable)] + top_k_tail
    lib.nsm_jaccard_raw_top_k.argtypes = [P(NsmSetTable), P(NsmSetTable)] + top_k_tail
    # (right_group in front of the tail)
    lib.nsm_indel_raw_top_k_grouped.argtypes = [P(NsmStrTable), P(NsmStrTable), ctypes.c_void_p] + top_k_tail
    lib.nsm_jaccard_raw_top_k_grouped.argtypes = [P(NsmSetTable), P(NsmSetTable), ctypes.c_void_p] + top_k_tail
    # threshold, k, category_mode, flags, banned_start, banned_j, out, out_count, stats, stream
    levels_top_k_tail = [ctypes.c_double, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.nsm_indel_levels_top_k.argtypes = [P(NsmLevelItems), P(NsmStrTable), P(NsmLevelItems), P(NsmStrTable)] + levels_top_k_tail
    lib.nsm_jaccard_levels_top_k.argtypes = [P(NsmSetTable), P(NsmSetTable)] + levels_top_k_tail
    # thresholds (host), n_thresholds, flags, pairs, left_best, right_best, stats, stream
    profile_tail = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                    ctypes.c_void_p, ctypes.c_void_p]
    lib.nsm_indel_raw_profile.argtypes = [P(NsmStrTable), P(NsmStrTable)] + profile_tail
    lib.nsm_jaccard_raw_profile.argtypes = [P(NsmSetTable), P(NsmSetTable)] + profile_tail
    # thresholds (host), n_thresholds, category_mode, flags, banned_start, banned_j, pairs, left_best, right_best, stats, stream
    levels_profile_tail = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.nsm_indel_levels_profile.argtypes = [P(NsmLevelItems), P(NsmStrTable), P(NsmLevelItems), P(NsmStrTable)] + levels_profile_tail
    lib.nsm_jaccard_levels_profile.argtypes = [P(NsmSetTable), P(NsmSetTable)] + levels_profile_tail
    # left_row, left_ids, right_row, right_ids, pairs, n_pairs, stream
    pairs_tail = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, c_u64, ctypes.c_void_p]
    lib.nsm_indel_raw_pairs.argtypes = [P(NsmStrTable), P(NsmStrTable)] + pairs_tail
    lib.nsm_jaccard_raw_pairs.argtypes = [P(NsmSetTable), P(NsmSetTable)] + pairs_tail
    lib.nsm_indel_levels_pairs.argtypes = [P(NsmLevelItems), P(NsmStrTable), P(NsmLevelItems), P(NsmStrTable)] + pairs_tail
    lib.nsm_jaccard_levels_pairs.argtypes = [P(NsmSetTable), P(NsmSetTable)] + pairs_tail
    # threshold, left_floor, right_floor, flags, hits, capacity, hit_count, stats, stream
    floor_tail = [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, c_u64, ctypes.c_void_p,
                  ctypes.c_void_p, ctypes.c_void_p]
    lib.nsm_indel_raw_floor_grid.argtypes = [P(NsmStrTable), P(NsmStrTable)] + floor_tail
    lib.nsm_jaccard_raw_floor_grid.argtypes = [P(NsmSetTable), P(NsmSetTable)] + floor_tail
    # threshold, left_floor, right_floor, category_mode, flags, banned_start, banned_j, hits, capacity, hit_count, stats, stream
    levels_floor_tail = [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p,
                         ctypes.c_void_p, ctypes.c_void_p, c_u64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.nsm_indel_levels_floor_grid.argtypes = [P(NsmLevelItems), P(NsmStrTable), P(NsmLevelItems), P(NsmStrTable)] + levels_floor_tail
    lib.nsm_jaccard_levels_floor_grid.argtypes = [P(NsmSetTable), P(NsmSetTable)] + levels_floor_tail
    # hits, scratch, capacity, hit_count, n_hint, id_limit, stream
    lib.nsm_sort_hits.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_u64, ctypes.c_void_p, c_u64, ctypes.c_uint32,
                                  ctypes.c_void_p]
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    lib.nsm_build_set_table.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, u32, P(NsmSetTable), vp]
    lib.nsm_build_str_table.argtypes = [vp, vp, vp, i32, u32, P(NsmStrTable), vp]
    lib.nsm_build_level_items.argtypes = [vp, vp, vp, vp, i32, i32, u32, P(NsmLevelItems), vp]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("nsm_last_error", "nsm_indel_levels_workspace_bytes"):
            fn.restype = ctypes.c_int
    lib.nsm_indel_levels_workspace_bytes.restype = c_u64
    lib.nsm_last_error.restype = ctypes.c_char_p
    # hits, n, left_ids, right_ids, flags, out, out_count, stats, stream
    assign_args = {"nsm_assign_hits": [vp, c_u64, i32, i32, u32, vp, vp, vp, vp]}
    # lists (host), n_lists, nodes, min_score, flags, label, stats, stream
    group_args = {"nsm_group_hits": [P(NsmHitList), i32, i32, ctypes.c_double, u32, vp, vp, vp]}
    # lists (host), n_lists, nodes, min_score, flags, forest, forest_count, label, stats, stream
    span_args = {"nsm_span_hits": [P(NsmHitList), i32, i32, ctypes.c_double, u32, vp, vp, vp, vp, vp]}
    # lists (host), n_lists, nodes, min_score, min_support, support (host array of device pointers), stats, stream
    support_args = {"nsm_support_hits": [P(NsmHitList), i32, i32, ctypes.c_double, i32, P(ctypes.c_void_p), vp, vp]}
    sets = [P(NsmSetTable), P(NsmSetTable), i32]  # left, right, measure; then the tail of the nsm_jaccard_* counterpart
    measure_args = {
        "nsm_set_raw_top_k": sets + top_k_tail,
        "nsm_set_raw_top_k_grouped": sets + [vp] + top_k_tail,
        "nsm_set_raw_profile": sets + profile_tail,
        "nsm_set_raw_floor_grid": sets + floor_tail,
        "nsm_set_raw_pairs": sets + pairs_tail,
        "nsm_set_levels_top_k": sets + levels_top_k_tail,
        "nsm_set_levels_profile": sets + levels_profile_tail,
        "nsm_set_levels_floor_grid": sets + levels_floor_tail,
        "nsm_set_levels_pairs": sets + pairs_tail,
    }
    strs = [P(NsmStrTable), P(NsmStrTable), i32]  # left, right, metric; then the tail of the nsm_indel_* counterpart
    levs = [P(NsmLevelItems), P(NsmStrTable), P(NsmLevelItems), P(NsmStrTable), i32]
    edit_args = {
        "nsm_edit_raw_top_k": strs + top_k_tail,
        "nsm_edit_raw_top_k_grouped": strs + [vp] + top_k_tail,
        "nsm_edit_raw_profile": strs + profile_tail,
        "nsm_edit_raw_floor_grid": strs + floor_tail,
        "nsm_edit_raw_pairs": strs + pairs_tail,
        "nsm_edit_levels_top_k": levs + levels_top_k_tail,
        "nsm_edit_levels_profile": levs + levels_profile_tail,
        "nsm_edit_levels_floor_grid": levs + levels_floor_tail,
        "nsm_edit_levels_pairs": levs + pairs_tail,
    }
    for names, args in ((ASSIGN_EXPORTS, assign_args), (GROUP_EXPORTS, group_args), (SPAN_EXPORTS, span_args),
                        (MEASURE_EXPORTS, measure_args), (EDIT_EXPORTS, edit_args), (SUPPORT_EXPORTS, support_args)):
        for name in names:
            try:
                fn = getattr(lib, name)
            except AttributeError:  # an older library: everything else still works
                continue
            fn.argtypes, fn.restype = args[name], ctypes.c_int
    _lib = lib
    return lib


def entry(name: str):
    """A C entry of the loaded library; ``NsmLibraryError`` when this build of the library lacks it."""
    try:
        return getattr(load(), name)
    except AttributeError:
        raise NsmLibraryError(f"{LIB_PATH} has no {name}: rebuild it (python -c 'import __graft_entry__ as g; g.build()')") from None


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().nsm_last_error().decode("utf-8", "replace")
        if status == 10002:
            raise NotImplementedError(f"{what}: {msg}")
        raise NsmLibraryError(f"{what} failed with status {status}: {msg}")
