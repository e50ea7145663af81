"""The CPU twins of tests/test_compaction_gpu.py: the references alone on the inputs of tests/compaction_cases.py, and what every
case is there to exercise, so that none of them can go vacuous: rows that take part in front of a count that cuts a thread's run
and rows with a good flag behind it, flags that flip inside a run, the single last row, the 64 / 65 detections of the tracker."""
import numpy as np
import pytest

from tests import compaction_cases as C
from tests import trackeval_ref as ER

CASES = [(R, p) for R in C.SIZES for p in C.EVAL_PATTERNS]
TRACK_CASES = [(R, p) for R in C.SIZES for p in C.TRACK_PATTERNS]


def test_rows_per_thread():
    assert [C.chunk(R) for R in C.SIZES] == [2, 3]
    assert 128 * C.chunk(257) == 256 and 200 * C.chunk(600) == 600          # thread 128 owns row 256 alone; 200 threads of three rows


def _assert_pattern(flags, count, pattern, dense):
    """the properties of the pattern, whatever function the case feeds"""
    R = flags.shape[1]
    p = C.properties(flags, count)
    assert p["flip_inside_a_run"] and (p["several_hits_in_a_run"] or not dense), p
    if pattern == "cut":
        assert count[0, 0] == R and p["cut_inside_a_run"][1] and p["hits_before_the_cut"][1] > 0 and p["hits_behind_the_cut"][1] > 0, p
        assert p["last_row_takes_part"][0]
    elif pattern == "zero":
        assert count[0, 0] == 0 and p["hits_before_the_cut"][0] == 0 and p["hits_behind_the_cut"][0] > 0, p
        assert p["cut_inside_a_run"][1] and p["hits_before_the_cut"][1] > 0 and p["hits_behind_the_cut"][1] > 0, p
    else:
        assert count is None and all(p["last_row_takes_part"]), p
    return p


@pytest.mark.parametrize("R,pattern", CASES)
def test_eval_match_reference(R, pattern):
    case = C.eval_case(R, pattern)
    p = _assert_pattern(case["flags"], case["count"], pattern, dense=True)
    want, part = case["want"], C.taking_part(case["flags"], case["count"])
    assert len(want["mpjpe"]) == sum(p["hits_before_the_cut"]) and want["total_gt"] == C.B * C.EVAL_G
    # the known answer: the row's own person, 13 mm a step, in row order
    rows = [(b, i) for b in range(C.B) for i in part[b]]
    assert want["gt_id"].tolist() == [C.EVAL_G * b + int(case["person"][b, i]) for b, i in rows]
    assert want["mpjpe"].tolist() == [13.0 * int(case["steps"][b, i]) for b, i in rows]
    assert want["score"].tolist() == [float(case["dets"][b, i, 0, 4]) for b, i in rows]


@pytest.mark.parametrize("R,pattern", TRACK_CASES)
def test_track_update_reference(R, pattern):
    case = C.track_case(R, pattern)
    n = []
    for dets, count, flags in case["frames"]:
        if pattern in C.EVAL_PATTERNS:
            _assert_pattern(flags, count, pattern, dense=pattern == "null")
        n.append([len(x) for x in C.taking_part(flags, count)])
    first, second = case["want"]
    T = C.TRACK["T"]
    state = dict(zip(C.TR.STATE, second["state"].tolist()))
    assert first["state"][2] == sum(min(k, T) for k in n[0]) and state["frames"] == 2 and state["matches"] > 0
    assert state["dropped"] == sum(max(k - C.TR.TRACK_MAX_D, 0) for f in n for k in f)
    if pattern == "null":
        assert min(n[0]) > 100 and state["dropped"] > 100                     # far more rows than the tracker takes
    if pattern in ("n64", "n65"):
        assert n == [[int(pattern[1:])] * C.B] * 2 and state["dropped"] == (2 * C.B if pattern == "n65" else 0)
        for snap in case["want"]:                                             # the row R - 1 is detection 63 / 64
            assert ((snap["slots"][:, R - 1] >= 0) == (pattern == "n64")).all(), snap["slots"][:, R - 1]
        assert state["matches"] == 64 * C.B                                   # every track finds its person in frame 1


@pytest.mark.parametrize("R,pattern", TRACK_CASES)
def test_track_eval_reference(R, pattern):
    case = C.score_case(R, pattern)
    hyp = unreported = dropped = 0
    for dets, count, ids, flags in case["frames"]:
        if pattern in C.EVAL_PATTERNS:
            _assert_pattern(flags, count, pattern, dense=pattern == "null")
        for b, rows in enumerate(C.taking_part(flags, count)):
            with_id = sum(1 for i in rows if ids[b, i] >= 0)
            hyp, unreported, dropped = hyp + min(with_id, ER.MAX_HYP), unreported + len(rows) - with_id, dropped + max(with_id - ER.MAX_HYP, 0)
    got = ER.counters(case["want"][-1])
    assert (got["hyp"], got["unreported"], got["dropped"]) == (hyp, unreported, dropped), got
    assert got["matches"] > 0 and got["frames"] == 2 * C.B and case["want"][-1]["dist_sum"].max() > 0
    if pattern == "null":
        assert dropped >= 40 and unreported >= 100                             # tens of rows past the 64 in every element and frame
    elif pattern in ("n64", "n65"):
        assert dropped == (2 * C.B if pattern == "n65" else 0) and hyp == 2 * C.B * 64 and unreported == 0
    else:
        assert unreported > 0 and hyp > 0
