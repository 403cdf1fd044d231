"""The oracle's gen_comparable and compare against what THE REFERENCE ITSELF returned on random cohort frames.
tests/golden/random_frames.json.gz holds the reference's outcome per seed (tests/golden/make_golden.py section 7:
the reference imported with the inert rapidfuzz / nltk stand-ins, so only intersection_vs_union is exercised --
fuzzy_match stays unpinned); the inputs are regenerated here from the same seeds.
The same generator drives tools/fuzz_api.py, which compares the GPU package with the oracle."""
import gzip
import json
import random
from pathlib import Path

import pandas as pd
import pytest

FIXTURE = Path(__file__).resolve().parent / "golden" / "random_frames.json.gz"


@pytest.fixture(scope="module")
def reference_outcomes():
    return json.loads(gzip.decompress(FIXTURE.read_bytes()).decode("utf-8"))


def _expected(entry, inputs):
    """(frame, exception type name) the reference produced for ``inputs``."""
    from support import random_frames as rf

    assert entry["inputs_crc32"] == rf.inputs_crc32(*inputs), (
        f"seed {entry['seed']}: tests/support/random_frames.py no longer draws the inputs the fixture was made from")
    if "raises" in entry:
        return None, entry["raises"]
    f = entry["frame"]
    return pd.DataFrame(f["rows"], index=f["index"], columns=f["columns"]), None


def _run(fn):
    try:
        return fn(), None
    except Exception as exc:  # the exception TYPE is part of the contract
        return None, exc


def test_oracle_gen_comparable_matches_reference(reference_outcomes):
    from oracle import compare as oc
    from support import random_frames as rf

    cases = reference_outcomes["gen_comparable"]
    assert [c["seed"] for c in cases] == list(range(1, 1501))
    outcomes = {"frames": 0, "rows": 0}
    for entry in cases:
        seed = entry["seed"]
        left, right, wl, bl, kw, _kinds = rf.case(seed, score_funcs=("intersection_vs_union",), sizes=(0, 1, 4, 4, 12, 12, 25, 25))
        want, want_exc = _expected(entry, (left, right, wl, bl, kw))
        got, got_exc = _run(lambda: oc.gen_comparable(left.copy(), right.copy(), wl, bl, **kw))
        assert (want_exc is None) == (got_exc is None) and want_exc in (None, type(got_exc).__name__), (
            f"seed {seed}: reference {want_exc} / oracle {got_exc!r}")
        if want_exc is not None:
            outcomes[want_exc] = outcomes.get(want_exc, 0) + 1
            continue
        problem = rf.frames_differ(got, want, 0.0)
        assert problem is None, f"seed {seed}: {problem}"
        outcomes["frames"] += 1
        outcomes["rows"] += len(want)
    assert outcomes["frames"] > 400 and outcomes["rows"] > 4000 and outcomes.get("KeyError", 0) > 20, outcomes
    print(outcomes)


def test_oracle_compare_matches_reference(reference_outcomes):
    """``compare``: score at ``cache_threshold or score_threshold``, keep ``>= score_threshold``, order by
    score descending (the order of equal scores is the reference's quicksort's business: not compared)."""
    from oracle import compare as oc
    from support import random_frames as rf

    cases = reference_outcomes["compare"]
    assert [c["seed"] for c in cases] == list(range(2001, 2401))
    frames = rows = 0
    for entry in cases:
        seed = entry["seed"]
        left, right, wl, bl, kw, _kinds = rf.case(seed, score_funcs=("intersection_vs_union",), sizes=(1, 4, 12, 25))
        kw["cache_threshold"] = random.Random(seed).choice([None, 0.05, 0.3, 0.6])
        want, want_exc = _expected(entry, (left, right, wl, bl, kw))
        got, got_exc = _run(lambda: oc.compare(left.copy(), right.copy(), wl, bl, **kw))
        assert (want_exc is None) == (got_exc is None) and want_exc in (None, type(got_exc).__name__), (
            f"seed {seed}: reference {want_exc} / oracle {got_exc!r}")
        if want_exc is not None:
            continue
        scores = list(want["MatchScore"])
        assert all(a >= b for a, b in zip(scores, scores[1:])), f"seed {seed}: reference order"
        canon = want.iloc[sorted(range(len(want)), key=lambda k: (-scores[k], want.index[k]))]
        problem = rf.frames_differ(got, canon, 0.0)
        assert problem is None, f"seed {seed}: {problem}"
        frames += 1
        rows += len(want)
    assert frames > 100 and rows > 1000, (frames, rows)
