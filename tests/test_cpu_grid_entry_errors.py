"""The four ``nsm_*_grid`` entries and ``nsm_indel_levels_workspace_bytes``: status and exact ``nsm_last_error()`` text of
malformed calls, and which check speaks first when two faults meet (no GPU needed).

Every case ends in host code before the entry's first HIP call -- read off the entries (csrc/indel_levels.hip,
indel_raw.hip, jaccard_raw_api.hip, jaccard_levels_api.hip), not found by running.  Left out because they cannot be
shown to stop there: every call that passes the checks (it launches); the tile and the park kernel's "needs ... bytes of
LDS" answers (unreachable: the largest alphabet, 255, at the widest stride, 512, still fits -- two 32 KiB text images
and a wave's four 18 KiB mask tables in the tile kernel's 160 KiB, 62 KiB in the park kernel's 64); nsm_indel_raw_grid's
"left rows per chunk" answer (it needs more than 2^31 left rows); a null ``len_start`` / ``size_start`` on the RIGHT
table of the RAW grids (not a fault there)."""
import pytest

from support.grid_entry_errors import call, check_table, workspace_bytes
from support.top_k_entry_errors import BADARG, FAKE, NULL, OK, UNSUPPORTED

PRUNE, WAVE_WIDE, PARK, SPLIT, TILE, PROBE = 1, 2, 16, 128, 256, 512
NULL_ARG = "{who}: null argument"
EMPTY = dict(n=0)


def _null_columns(message, left_columns, right_columns, key=("left", "right")):
    return [(f"{side} {col} null", {side_key: {col: None}}, BADARG, message if isinstance(message, str) else message[side])
            for side, side_key, cols in (("left", key[0], left_columns), ("right", key[1], right_columns)) for col in cols]


# ---------------------------------------------------------------------------------------------- nsm_indel_levels_grid
LEVELS_STRIDE = "{who}: stride %d/%d unsupported (both sides 64, 128, 256 or 512 code units)"
LEVELS_ALPHABET = "{who}: alphabets differ or exceed 255"
LEVELS_PARTITION = "{who}: a category partition needs seg/seg_start/cat on both sides and NSM_CAT_INTERSECT"
LEVELS_COLUMN = "{who}: table has a null column"
SEG = dict(seg=FAKE, seg_start=FAKE, cat=FAKE)

INDEL_LEVELS_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    ("left_strings null", dict(left_strings=NULL), BADARG, NULL_ARG),
    ("right_strings null", dict(right_strings=NULL), BADARG, NULL_ARG),
    ("hit_count null", dict(hit_count=False), BADARG, NULL_ARG),
    ("hits null with capacity", dict(hits=False, capacity=1), BADARG, NULL_ARG),
    ("hits null without capacity, empty side", dict(hits=False, capacity=0, left=EMPTY), OK, None),
    ("stride 64 vs 128", dict(right_strings=dict(stride=128)), UNSUPPORTED, LEVELS_STRIDE % (64, 128)),
    ("stride 96", dict(left_strings=dict(stride=96), right_strings=dict(stride=96)), UNSUPPORTED, LEVELS_STRIDE % (96, 96)),
    ("alphabets differ", dict(right_strings=dict(alphabet=11)), BADARG, LEVELS_ALPHABET),
    ("alphabet 0", dict(left_strings=dict(alphabet=0), right_strings=dict(alphabet=0)), BADARG, LEVELS_ALPHABET),
    ("alphabet 256", dict(left_strings=dict(alphabet=256), right_strings=dict(alphabet=256)), BADARG, LEVELS_ALPHABET),
    ("stride and alphabet: the stride speaks first", dict(left_strings=dict(stride=96, alphabet=0)), UNSUPPORTED,
     LEVELS_STRIDE % (96, 64)),
    ("category mode 7", dict(category_mode=7), BADARG, "{who}: unknown category mode 7"),
    ("alphabet before category mode", dict(category_mode=7, right_strings=dict(alphabet=11)), BADARG, LEVELS_ALPHABET),
    ("negative n left", dict(left=dict(n=-1)), BADARG, "{who}: negative row count"),
    ("negative n right", dict(right=dict(n=-3)), BADARG, "{who}: negative row count"),
    ("negative n before empty side", dict(left=EMPTY, right=dict(n=-1)), BADARG, "{who}: negative row count"),
    # an empty side answers before the workspace alignment, the partition and the null columns are looked at
    ("empty left: null columns, misaligned workspace", dict(left=dict(n=0, first=None, nlev=None, orig=None), workspace=20,
                                                            workspace_bytes=4096), OK, None),
    ("empty right: half a partition, cat missing", dict(right=dict(n=0, seg=FAKE), category_mode=1), OK, None),
    ("workspace not 8-byte aligned", dict(workspace=20, workspace_bytes=4096), BADARG, "{who}: workspace must be 8-byte aligned"),
    ("workspace alignment before the partition", dict(workspace=4, left=dict(seg=FAKE)), BADARG,
     "{who}: workspace must be 8-byte aligned"),
    ("seg on the left only", dict(left=SEG, right=dict(cat=FAKE), category_mode=1), BADARG, LEVELS_PARTITION),
    ("seg on the right only", dict(left=dict(cat=FAKE), right=SEG, category_mode=1), BADARG, LEVELS_PARTITION),
    ("seg without seg_start", dict(left=dict(seg=FAKE, cat=FAKE), right=SEG, category_mode=1), BADARG, LEVELS_PARTITION),
    ("seg without cat", dict(left=SEG, right=dict(seg=FAKE, seg_start=FAKE), category_mode=1), BADARG, LEVELS_PARTITION),
    ("seg with NSM_CAT_NONE", dict(left=SEG, right=SEG, category_mode=0), BADARG, LEVELS_PARTITION),
    ("seg with INTERSECT_OR_BOTH_EMPTY", dict(left=SEG, right=SEG, category_mode=2), BADARG, LEVELS_PARTITION),
    ("partition before null columns", dict(left=dict(seg=FAKE, first=None)), BADARG, LEVELS_PARTITION),
    *_null_columns(LEVELS_COLUMN, ("first", "nlev", "orig"), ("first", "nlev", "orig")),
    *_null_columns(LEVELS_COLUMN, ("codes", "len"), ("codes", "len"), key=("left_strings", "right_strings")),
    ("cat missing on the left under a category mode", dict(right=dict(cat=FAKE), category_mode=1), BADARG, LEVELS_COLUMN),
    ("cat missing on the right under a category mode", dict(left=dict(cat=FAKE), category_mode=2), BADARG, LEVELS_COLUMN),
    # past the checks, still before any HIP call: the router's and the geometry's own answers
    ("NSM_FLAG_PROBE without a workspace", dict(threshold=0.8, flags=PROBE), BADARG,
     "{who}: NSM_FLAG_PROBE needs NSM_FLAG_SPLIT, a workspace and a grid the split path takes (strings up to 64 code units "
     "with histograms, NSM_FLAG_PRUNE)"),
    ("NSM_FLAG_PROBE | NSM_FLAG_SPLIT without a workspace", dict(threshold=0.8, flags=PROBE | SPLIT | PRUNE), BADARG,
     "{who}: NSM_FLAG_PROBE needs NSM_FLAG_SPLIT, a workspace and a grid the split path takes (strings up to 64 code units "
     "with histograms, NSM_FLAG_PRUNE)"),
]


def test_indel_levels_grid_answers():
    check_table("nsm_indel_levels_grid", INDEL_LEVELS_CASES)


# ------------------------------------------------------------------------------------ nsm_indel_levels_workspace_bytes
HIST_NONE = dict(hist=None)


@pytest.mark.parametrize("label, kw", [
    ("left null", dict(left=NULL)),
    ("right null", dict(right=NULL)),
    ("left_strings null", dict(left_strings=NULL)),
    ("right_strings null", dict(right_strings=NULL)),
    ("left stride 128", dict(left_strings=dict(stride=128))),
    ("right stride 128", dict(right_strings=dict(stride=128))),
    ("alphabets differ", dict(right_strings=dict(alphabet=11))),
    ("alphabet 0", dict(left_strings=dict(alphabet=0), right_strings=dict(alphabet=0))),
    ("NSM_FLAG_PARK", dict(flags=PRUNE | PARK)),
    ("NSM_FLAG_WAVE_WIDE", dict(flags=PRUNE | WAVE_WIDE)),
    ("no NSM_FLAG_PRUNE", dict(flags=0)),
    ("left histograms missing", dict(left_strings=HIST_NONE)),
    ("right histograms missing", dict(right_strings=HIST_NONE)),
    ("threshold below 0.7 without NSM_FLAG_SPLIT", dict(threshold=0.69)),
    ("NSM_FLAG_TILE", dict(flags=PRUNE | TILE)),
    ("alphabet 64: mask tables beyond 64 entries", dict(left_strings=dict(alphabet=64), right_strings=dict(alphabet=64))),
    ("empty left", dict(left=EMPTY)),
    ("empty right", dict(right=EMPTY)),
    ("2^24 left rows", dict(left=dict(n=1 << 24))),
    ("2^24 right rows", dict(right=dict(n=1 << 24))),
])
def test_workspace_bytes_is_zero_off_the_split_path(label, kw):
    assert workspace_bytes(**kw) == 0, label


def test_workspace_bytes_of_an_eligible_grid():
    # 64 control words, then two queue halves of (expected survivors + 2^16) 8-byte entries; 2 % of 5000 x 5000 pairs
    assert workspace_bytes() == 64 * 8 + 2 * (500000 + 65536) * 8 == 9049088
    assert workspace_bytes(expected_survivors=0.0) == 9049088
    assert workspace_bytes(expected_survivors=1000.0) == 64 * 8 + 2 * (1000 + 65536) * 8 == 1065088
    # a partition visits 1/16 of the grid; NSM_FLAG_SPLIT takes a threshold below 0.7; alphabet 63 still fits
    assert workspace_bytes(left=dict(seg=FAKE)) == 64 * 8 + 2 * (31250 + 65536) * 8
    assert workspace_bytes(threshold=0.5, flags=PRUNE | SPLIT) == 9049088
    assert workspace_bytes(left_strings=dict(alphabet=63), right_strings=dict(alphabet=63)) == 9049088
    assert workspace_bytes(left=dict(n=(1 << 24) - 1), right=dict(n=1), expected_survivors=1.0) == 64 * 8 + 2 * 65537 * 8


# ------------------------------------------------------------------------------------------------- nsm_indel_raw_grid
RAW_STRIDE = LEVELS_STRIDE
INDEL_RAW_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    ("hit_count null", dict(hit_count=False), BADARG, NULL_ARG),
    ("hits null with capacity", dict(hits=False, capacity=1), BADARG, NULL_ARG),
    ("hits null without capacity, empty side", dict(hits=False, capacity=0, right=EMPTY), OK, None),
    ("stride 64 vs 128", dict(right=dict(stride=128)), UNSUPPORTED, RAW_STRIDE % (64, 128)),
    ("stride 96", dict(left=dict(stride=96), right=dict(stride=96)), UNSUPPORTED, RAW_STRIDE % (96, 96)),
    ("alphabets differ", dict(right=dict(alphabet=11)), BADARG, "{who}: alphabets differ or exceed 255 (10, 11)"),
    ("alphabet 0", dict(left=dict(alphabet=0), right=dict(alphabet=0)), BADARG, "{who}: alphabets differ or exceed 255 (0, 0)"),
    ("alphabet 256", dict(left=dict(alphabet=256), right=dict(alphabet=256)), BADARG,
     "{who}: alphabets differ or exceed 255 (256, 256)"),
    ("stride and alphabet: the stride speaks first", dict(left=dict(stride=96, alphabet=0)), UNSUPPORTED, RAW_STRIDE % (96, 64)),
    ("negative n", dict(right=dict(n=-1)), BADARG, "{who}: negative row count"),
    ("negative n before empty side", dict(left=dict(n=-1), right=EMPTY), BADARG, "{who}: negative row count"),
    ("empty left before null columns", dict(left=dict(n=0, codes=None, len=None)), OK, None),
    ("empty right before null columns", dict(right=dict(n=0, orig=None), left=dict(len_start=None)), OK, None),
    *_null_columns("{who}: table has a null column", ("codes", "len", "orig", "len_start"), ("codes", "len", "orig")),
    ("null column at stride 256", dict(left=dict(stride=256, codes=None), right=dict(stride=256)), BADARG,
     "{who}: table has a null column"),
    ("hist16 not 16-byte aligned", dict(left=dict(hist=FAKE, hist16=FAKE + 4), right=dict(hist=FAKE, hist16=FAKE), flags=PRUNE),
     BADARG, "{who}: hist16 must be 16-byte aligned (rows are read as one 128-bit word)"),
]


def test_indel_raw_grid_answers():
    check_table("nsm_indel_raw_grid", INDEL_RAW_CASES)


# ----------------------------------------------------------------------------------------------- nsm_jaccard_raw_grid
WIDTHS_DIFFER = "{who}: left width 16 != right width 32"
WIDTH_48 = "{who}: width 48 not in {{16, 32, 64}}"
JACCARD_RAW_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    ("hit_count null", dict(hit_count=False), BADARG, NULL_ARG),
    ("hits null with capacity", dict(hits=False, capacity=1), BADARG, NULL_ARG),
    ("widths differ", dict(right=dict(width=32)), BADARG, WIDTHS_DIFFER),
    ("widths differ before negative n", dict(left=dict(n=-1), right=dict(width=32)), BADARG, WIDTHS_DIFFER),
    ("negative n", dict(left=dict(n=-1)), BADARG, "{who}: negative row count"),
    ("empty left before null columns", dict(left=dict(n=0, ids=None, cnt=None)), OK, None),
    ("empty right before null columns and the width", dict(left=dict(width=48, size_start=None), right=dict(width=48, n=0)), OK,
     None),
    *_null_columns("{who}: table has a null column", ("ids", "cnt", "orig", "size_start"), ("ids", "cnt", "orig")),
    ("width 48", dict(left=dict(width=48), right=dict(width=48)), UNSUPPORTED, WIDTH_48),
    ("null column before the width", dict(left=dict(width=48, ids=None), right=dict(width=48)), BADARG,
     "{who}: table has a null column"),
]


def test_jaccard_raw_grid_answers():
    check_table("nsm_jaccard_raw_grid", JACCARD_RAW_CASES)


# -------------------------------------------------------------------------------------------- nsm_jaccard_levels_grid
SET_COLUMN = {"left": "{who}: left table has a null column", "right": "{who}: right table has a null column"}
SET_PARTITION = "{who}: a category partition needs seg/seg_start on both sides and NSM_CAT_INTERSECT"
SET_ROWS = "{who}: bad row count or level stride"
SET_SEG = dict(seg=FAKE, seg_start=FAKE, cat=FAKE)
SET_COLUMNS = ("ids", "cnt", "sig", "orig", "nlev", "plen", "filt")
JACCARD_LEVELS_CASES = [
    ("left null", dict(left=NULL), BADARG, NULL_ARG),
    ("right null", dict(right=NULL), BADARG, NULL_ARG),
    ("hit_count null", dict(hit_count=False), BADARG, NULL_ARG),
    ("hits null with capacity", dict(hits=False, capacity=1), BADARG, NULL_ARG),
    ("widths differ", dict(right=dict(width=32)), BADARG, WIDTHS_DIFFER),
    ("negative n", dict(right=dict(n=-1)), BADARG, SET_ROWS),
    ("max_levels 0", dict(left=dict(max_levels=0)), BADARG, SET_ROWS),
    ("category mode 7", dict(category_mode=7), BADARG, "{who}: unknown category mode 7"),
    ("rows before category mode", dict(category_mode=7, left=dict(n=-1)), BADARG, SET_ROWS),
    ("category mode before empty side", dict(category_mode=7, left=EMPTY), BADARG, "{who}: unknown category mode 7"),
    ("empty left before null columns", dict(left=dict(n=0, ids=None, sig=None)), OK, None),
    ("empty right before null columns, the partition and the width",
     dict(left=dict(width=48, seg=FAKE), right=dict(width=48, n=0, filt=None), category_mode=1), OK, None),
    *_null_columns(SET_COLUMN, SET_COLUMNS, SET_COLUMNS),
    ("cat missing on the left under a category mode", dict(right=dict(cat=FAKE), category_mode=1), BADARG, SET_COLUMN["left"]),
    ("cat missing on the right under a category mode", dict(left=dict(cat=FAKE), category_mode=2), BADARG, SET_COLUMN["right"]),
    ("both sides: the left speaks first", dict(left=dict(plen=None), right=dict(ids=None)), BADARG, SET_COLUMN["left"]),
    ("seg on the left only", dict(left=SET_SEG, right=dict(cat=FAKE), category_mode=1), BADARG, SET_PARTITION),
    ("seg on the right only", dict(left=dict(cat=FAKE), right=SET_SEG, category_mode=1), BADARG, SET_PARTITION),
    ("seg without seg_start", dict(left=dict(seg=FAKE, cat=FAKE), right=SET_SEG, category_mode=1), BADARG, SET_PARTITION),
    ("seg with NSM_CAT_NONE", dict(left=SET_SEG, right=SET_SEG, category_mode=0), BADARG, SET_PARTITION),
    ("seg with INTERSECT_OR_BOTH_EMPTY", dict(left=SET_SEG, right=SET_SEG, category_mode=2), BADARG, SET_PARTITION),
    ("null column before the partition", dict(left=dict(seg=FAKE, ids=None)), BADARG, SET_COLUMN["left"]),
    ("width 48", dict(left=dict(width=48), right=dict(width=48)), UNSUPPORTED, WIDTH_48),
    ("width 48 with NSM_FLAG_INDEX", dict(left=dict(width=48), right=dict(width=48), flags=4), UNSUPPORTED, WIDTH_48),
]


def test_jaccard_levels_grid_answers():
    check_table("nsm_jaccard_levels_grid", JACCARD_LEVELS_CASES)


def test_every_case_is_an_error_or_an_empty_side():
    """A table entry that expects success must have an empty side: any other successful call would have launched."""
    for cases in (INDEL_LEVELS_CASES, INDEL_RAW_CASES, JACCARD_RAW_CASES, JACCARD_LEVELS_CASES):
        for label, kw, status, message in cases:
            if status == OK:
                assert message is None and any((kw.get(side) or {}).get("n") == 0 for side in ("left", "right")), label
            else:
                assert status in (BADARG, UNSUPPORTED) and message, label
