"""The rules of mvg_track_eval (include/mvg_decoder.h) on the CPU: the plain-Python restatement (tests/trackeval_ref.py), driven by
the tracker restatement's ids (tests/track_ref.py), against answers known by construction of the sequences
(tests/trackeval_cases.py); the ratios through tracking.TrackEvaluator.report on host buffers; the host assignment routine
against brute force."""
import functools
import math

import numpy as np
import pytest
import torch

from mvgformer_amd.tracking import TrackEvaluator, max_weight_assignment
from tests import trackeval_cases as EC
from tests import trackeval_ref as ER


@functools.lru_cache(maxsize=None)
def _run(name):
    case = EC.cases()[name]
    return case, ER.run(case, ER.host_ids(case))


def _report(case, buf):
    """TrackEvaluator.report on the restatement's buffers"""
    ev = TrackEvaluator(batch=buf["counters"].shape[0], max_persons=case["P"], max_ids=case["K"], dist_thr=case["dist_thr"],
                        device="cpu")
    for k, t in ev.buffers.items():
        t.copy_(torch.from_numpy(buf[k]))
    return ev.report()


def _final(name):
    case, snaps = _run(name)
    rep = _report(case, snaps[-1])
    return ER.counters(snaps[-1]), rep["total"], snaps


def test_perfect_tracking():
    c, total, _ = _final("perfect")
    assert (c["misses"], c["false_pos"], c["switches"]) == (0, 0, 0)
    assert (c["frames"], c["gt"], c["hyp"], c["matches"], c["kept"]) == (8, 24, 24, 24, 21)
    assert total["mota"] == 1.0 and total["idf1"] == 1.0 and total["idtp"] == 24
    assert 0.0 < total["motp"] < 10.0                                           # 5 mm noise per coordinate
    assert (total["identities"], total["mostly_tracked"], total["mostly_lost"]) == (3, 3, 0)


def test_occlusion_counts_one_switch():
    c, total, snaps = _final("occlusion")
    assert (c["gt"], c["hyp"], c["misses"], c["switches"], c["false_pos"]) == (24, 19, 5, 1, 0)
    assert total["mota"] == 0.75 and total["idtp"] == 18 and total["idf1"] == 36.0 / 43.0
    first, last = snaps[0]["last_track"][0, :3].tolist(), snaps[-1]["last_track"][0, :3].tolist()
    assert sorted(first) == [0, 1, 2]                                           # ids in the order of the first frame's scores
    assert last == [first[0], 3, first[2]]                                      # person 1 came back as the stream's fourth track
    assert snaps[-1]["seen"][0, :3].tolist() == [8, 8, 8] and snaps[-1]["covered"][0, :3].tolist() == [6, 5, 8]
    assert (total["mostly_tracked"], total["mostly_lost"]) == (1, 0)


def test_min_hits_rows_are_unreported_not_false_positives():
    c, total, _ = _final("min_hits")
    assert (c["unreported"], c["misses"], c["false_pos"], c["hyp"], c["switches"]) == (6, 6, 0, 18, 0)
    assert total["mota"] == 0.75 and total["idf1"] == 36.0 / 42.0


def test_ghost_detection_is_a_false_positive():
    c, total, _ = _final("ghost")
    assert (c["false_pos"], c["misses"], c["switches"], c["matches"], c["kept"], c["hyp"]) == (3, 0, 0, 24, 21, 27)
    assert total["idf1"] == 48.0 / 51.0 and total["mota"] == 1.0 - 3.0 / 24.0


def test_kept_correspondence_beats_the_cheaper_assignment():
    c, _, snaps = _final("kept_pairs")
    assert (c["switches"], c["kept"], c["matches"], c["misses"]) == (0, 2, 4, 0)
    assert snaps[1]["last_track"][0].tolist() == snaps[0]["last_track"][0].tolist() == [0, 1]
    c, _, snaps = _final("kept_pairs_cleared")
    assert (c["switches"], c["kept"], c["matches"]) == (0, 0, 4)                # nothing to switch from: last_track was cleared
    assert snaps[0]["last_track"][0].tolist() == [0, 1] and snaps[1]["last_track"][0].tolist() == [1, 0]
    # the kept pairs pay 2 sqrt(200^2 + 100^2), the swap 2 sqrt(100^2 + 100^2), on top of frame 0's 200 + 200
    # (one add per match, in person order; a distance is the mean of 15 equal joint distances, added one by one)
    def mean(x):
        total = 0.0
        for _ in range(EC.J):
            total += x
        return total / float(EC.J)
    assert _final("kept_pairs")[2][1]["dist_sum"][0] == ((200.0 + 200.0) + mean(math.sqrt(50000.0))) + mean(math.sqrt(50000.0))
    assert snaps[1]["dist_sum"][0] == ((200.0 + 200.0) + mean(math.sqrt(20000.0))) + mean(math.sqrt(20000.0))


def test_contested_track_goes_to_the_lower_slot():
    c, _, snaps = _final("contested")
    assert snaps[1]["last_track"][0].tolist() == [0, 0]                         # both persons name id 0
    assert snaps[2]["last_track"][0].tolist() == [0, 1]
    assert (c["gt"], c["hyp"], c["matches"], c["misses"], c["false_pos"], c["switches"], c["kept"]) == (5, 4, 4, 1, 0, 1, 1)
    assert snaps[2]["dist_sum"][0] == ((0.0 + 150.0) + 160.0) + 30.0


def test_distance_on_the_threshold():
    c, total, snaps = _final("threshold_on")
    assert (c["matches"], c["misses"], c["false_pos"]) == (1, 0, 0) and snaps[0]["dist_sum"][0] == 512.0
    assert snaps[0]["overlap"][0, 0, 0] == 1
    c, total, snaps = _final("threshold_off")
    assert (c["matches"], c["misses"], c["false_pos"]) == (0, 1, 1) and snaps[0]["dist_sum"][0] == 0.0
    assert snaps[0]["overlap"].sum() == 0 and total["mota"] == -1.0 and math.isnan(total["motp"])


def test_visibility_selects_the_joints():
    c, _, snaps = _final("visibility")
    assert (c["gt"], c["hyp"], c["matches"], c["false_pos"], c["misses"], c["bad_id"]) == (1, 2, 1, 1, 0, 0)
    assert snaps[0]["dist_sum"][0] == ((8.0 + 32.0) + 40.0) / 3.0
    assert snaps[0]["seen"][0].tolist() == [1, 0]


def test_nan_detection_is_a_false_positive_and_a_miss():
    c, total, snaps = _final("nan_detection")
    # the NaN row opens a track of its own, which no later row continues: one false positive in all
    assert (c["gt"], c["hyp"], c["matches"], c["misses"], c["false_pos"]) == (8, 8, 7, 1, 1)
    assert all(math.isfinite(float(s["dist_sum"][0])) for s in snaps)
    per_frame = [ER.counters(s) for s in snaps]
    assert per_frame[2]["misses"] - per_frame[1]["misses"] == 1 and per_frame[2]["false_pos"] - per_frame[1]["false_pos"] == 1


def test_frames_without_annotation_and_empty_frames():
    _, _, snaps = _final("annotation")
    assert all(snaps[1][k].tobytes() == snaps[0][k].tobytes() for k in snaps[0])              # num_person = -1 changes nothing
    before, after = ER.counters(snaps[1]), ER.counters(snaps[2])
    assert after["frames"] - before["frames"] == 1 and after["gt"] == before["gt"] and after["matches"] == before["matches"]
    assert after["false_pos"] - before["false_pos"] == after["hyp"] - before["hyp"] == 2     # num_person = 0: all false positives
    assert ER.counters(snaps[3])["frames"] == 3


def test_person_ids_permuted_out_of_range_and_repeated():
    c, _, snaps = _final("identities")
    assert c["bad_id"] == 4 and c["gt"] == 8 and c["matches"] == 8 and c["false_pos"] == 4
    assert snaps[1]["seen"][0].tolist() == [2, 0, 2, 0]                        # slots 0, 1 are the identities 2, 0
    assert snaps[3]["seen"][0].tolist() == [2, 2, 4, 0]                        # then slots 0, 2 are the identities 2, 1
    assert c["switches"] == 0


def test_table_too_small_for_the_ids():
    case, snaps = _run("small_table")
    rep = _report(case, snaps[-1])
    assert rep["total"]["id_overflow"] > 0 and rep["total"]["idf1"] is None and "max_ids" in rep["note"]
    assert rep["max_ids_needed"] is None and "None" not in rep["note"]          # no tracker was seen: its next_id is not known
    assert rep["total"]["mota"] == 0.75                                         # the CLEAR-MOT counts do not need the table


@pytest.mark.parametrize("name", sorted(EC.cases()))
def test_identities_of_the_counts(name):
    case, snaps = _run(name)
    rep = _report(case, snaps[-1])
    for b, s in enumerate(rep["streams"]):
        assert s["matches"] + s["misses"] == s["gt"] and s["matches"] + s["false_pos"] == s["hyp"], (name, b, s)
        assert s["idtp"] <= s["matches"] and s["kept"] <= s["matches"], (name, b, s)
        assert int(snaps[-1]["seen"][b].sum()) == s["gt"] and int(snaps[-1]["covered"][b].sum()) == s["matches"]
        assert int(snaps[-1]["overlap"][b].sum()) + s["id_overflow"] >= s["matches"]
    total = rep["total"]
    assert total["gt"] == sum(s["gt"] for s in rep["streams"]) and total["reserved"] == 0


def test_two_streams_are_scored_apart():
    case, snaps = _run("two_streams")
    rep = _report(case, snaps[-1])
    a, b = rep["streams"]
    assert (a["frames"], a["gt"], a["misses"], a["mota"]) == (5, 15, 0, 1.0)
    assert (b["frames"], b["gt"], b["misses"], b["false_pos"]) == (4, 8, 2, 0)      # frame 3 of stream 1 has no annotation
    assert rep["total"]["idtp"] == a["idtp"] + b["idtp"] and rep["total"]["motp"] == (a["dist_sum"] + b["dist_sum"]) / 21


def test_host_assignment_equals_brute_force():
    rng = np.random.default_rng(40)
    shapes = [(1, 1), (2, 3), (3, 2), (4, 4), (5, 7), (6, 7), (6, 2), (1, 7), (6, 6)]
    for n, m in shapes:
        for hi in (2, 10, 1000):
            table = rng.integers(0, hi, size=(n, m))
            total, col = max_weight_assignment(table)
            assert total == ER.best_assignment(table), (n, m, table)
            live = [c for c in col if c >= 0]
            assert len(live) == min(n, m) == len(set(live))
            assert total == sum(int(table[r, c]) for r, c in enumerate(col) if c >= 0)
    assert max_weight_assignment(np.zeros((3, 0), np.int64))[0] == 0
    assert max_weight_assignment(np.zeros((3, 5), np.int64))[0] == 0
