"""Inputs of tests/test_compaction_cpu.py and tests/test_compaction_gpu.py: rows-per-thread cases for the ordered compaction that
mvg_eval_match, mvg_track_update and mvg_track_eval share (scan_rows in csrc/exact_dev.h), and the references on them.

A workgroup of 256 threads gives thread t the rows [t * chunk, (t + 1) * chunk) with chunk = ceil(R / 256).  R = 257: two rows a
thread, thread 128 owns the single last row, threads 129 .. 255 none.  R = 600: three rows a thread.  B = 2, J = 15.  Patterns:
  cut    count = [R, a value inside a thread's run]; the flags flip inside the runs; the rows behind the count carry flag 0, so
         that only the count keeps them out
  zero   count = [0, another value inside a run]
  null   count = None: every row is looked at, the last one takes part
  n64    (the tracker and its scoring) exactly 64 participating rows, the last one on row R - 1
  n65    65 of them: the row R - 1 is the one past MVG_TRACK_MAX_D, dropped = 1

Every pose is a skeleton of integer coordinates moved by an integer multiple of (3, 4, 12), so every joint distance is an exact
multiple of 13 and every sum of them is exact in fp64: the value does not depend on the order of a sum (numpy's np.mean in
oracle/eval_ref.py adds pairwise) nor on whether a product is fused into a sum, and the comparison can be bit for bit."""
import functools

import numpy as np

from oracle import eval_ref
from tests import track_ref as TR
from tests import trackeval_ref as ER

B, J, THREADS = 2, 15, 256
SIZES = (257, 600)
STEP = np.array([3.0, 4.0, 12.0])                      # |STEP| = 13
FAR = 4000                                             # persons are FAR steps apart: 52 m
SKELETON = np.stack([np.arange(J) * 10.0, (np.arange(J) * 7) % 50 * 1.0, np.arange(J) * 5.0], axis=1)
EVAL_PATTERNS = ("cut", "zero", "null")
TRACK_PATTERNS = EVAL_PATTERNS + ("n64", "n65")


def chunk(R):
    return (R + THREADS - 1) // THREADS


def _counts(R, pattern):
    """count[:, 0] of the pattern: the cuts lie strictly inside a thread's run"""
    c = chunk(R)
    cut = {"cut": [R, c * 100 + 1], "zero": [0, c * 57 + c - 1]}.get(pattern)
    return None if cut is None else np.array([[cut[0], 0], [cut[1], 0]], np.int32)


def _flags(R, pattern, seed, density):
    """(B, R) bool: the rows whose flag is >= 0"""
    rng = np.random.default_rng(1000 * R + seed)
    if pattern in ("n64", "n65"):
        n = int(pattern[1:])
        flags = np.zeros((B, R), bool)
        for b in range(B):
            flags[b, rng.choice(R - 1, size=n - 1, replace=False)] = True
            flags[b, R - 1] = True
        return flags
    flags = rng.uniform(size=(B, R)) < density
    flags[:, R - 1] = True
    return flags


def taking_part(flags, count):
    """per element the rows that take part, in row order"""
    R = flags.shape[1]
    rows = [R if count is None else min(max(int(count[b, 0]), 0), R) for b in range(B)]
    return [[i for i in range(rows[b]) if flags[b, i]] for b in range(B)]


def properties(flags, count):
    """what a case is meant to exercise, read from its inputs"""
    R = flags.shape[1]
    c = chunk(R)
    part = taking_part(flags, count)
    rows = [R if count is None else int(count[b, 0]) for b in range(B)]
    runs = [flags[b, :R // c * c].reshape(-1, c) for b in range(B)]
    return dict(flip_inside_a_run=all(bool((r.any(1) & ~r.all(1)).any()) for r in runs),
                several_hits_in_a_run=all(bool((r.sum(1) >= 2).any()) for r in runs),
                cut_inside_a_run=[rows[b] % c != 0 for b in range(B)],
                hits_before_the_cut=[len(part[b]) for b in range(B)],
                hits_behind_the_cut=[int(flags[b, rows[b]:].sum()) for b in range(B)],
                last_row_takes_part=[bool(part[b]) and part[b][-1] == R - 1 for b in range(B)])


def _dets(flags, person_of_row, steps_of_row):
    """(B, R, J, 5) fp32: row i stands steps_of_row[b, i] steps of (3, 4, 12) from person person_of_row[b, i]"""
    R = flags.shape[1]
    dets = np.zeros((B, R, J, 5), np.float32)
    off = (person_of_row * FAR + steps_of_row)[..., None, None] * STEP
    dets[..., :3] = SKELETON + off
    dets[..., 3] = np.where(flags, 0.0, -1.0)[..., None]
    dets[..., 4] = ((np.arange(R) * 29 % 97) / 128.0)[None, :, None]
    assert np.abs(dets[..., :3]).max() < 2 ** 24
    return dets


# ---- mvg_eval_match -----------------------------------------------------------------------------------------------------------------
EVAL_G, EVAL_GMAX = 3, 4


@functools.lru_cache(maxsize=None)
def eval_case(R, pattern):
    """inputs of one mvg_eval_match call and the list oracle/eval_ref.py makes of them"""
    flags, count = _flags(R, pattern, 1, 0.5), _counts(R, pattern)
    i = np.arange(R)
    person = np.broadcast_to(i % EVAL_G, (B, R))
    steps = np.stack([1 + (i * 37 + 11 * b) % 251 for b in range(B)])           # < FAR / 2: the row's own person is the nearest
    dets = _dets(flags, person, steps)
    j3d = np.zeros((B, EVAL_GMAX, J, 3), np.float32)
    j3d[:, :EVAL_G] = SKELETON + (np.arange(EVAL_G) * FAR)[:, None, None] * STEP
    vis = (np.random.default_rng(R).uniform(size=(B, EVAL_GMAX, J)) > 0.4).astype(np.float32)
    vis[:, :, 0] = 1.0
    num = np.full((B,), EVAL_G, np.int32)
    rows = [R if count is None else int(count[b, 0]) for b in range(B)]
    entries, total_gt = eval_ref.match_predictions([dets[b, :rows[b]] for b in range(B)], [j3d[b, :EVAL_G] for b in range(B)],
                                                   [vis[b, :EVAL_G, :, None] for b in range(B)])
    want = dict(mpjpe=np.array([e["mpjpe"] for e in entries], np.float64), score=np.array([e["score"] for e in entries], np.float64),
                gt_id=np.array([e["gt_id"] for e in entries], np.int64), total_gt=total_gt)
    return dict(dets=dets, count=count, joints_3d=j3d, vis=vis, num_person=num, flags=flags, person=person, steps=steps, want=want)


# ---- mvg_track_update ---------------------------------------------------------------------------------------------------------------
TRACK = dict(T=64, max_dist=500.0, max_misses=2, min_hits=1)
TRACK_KEYS = ("id", "hits", "misses", "born", "score", "pose", "next_id", "state", "ids", "slots")


def live_only(buf):
    """the buffers with the pose / score / hits / misses / born of FREE slots blanked: they are whatever the last owner left"""
    out = {k: np.array(v, copy=True) for k, v in buf.items()}
    free = out["id"] < 0
    for k in ("hits", "misses", "born", "score"):
        out[k][free] = 0
    out["pose"][free] = 0
    return out


@functools.lru_cache(maxsize=None)
def track_case(R, pattern):
    """two frames of mvg_track_update and tests/track_ref.py over them: frame 0 opens the tracks, frame 1 has the same persons,
    three steps further on, in other rows"""
    frames = []
    for f in range(2):
        flags, count = _flags(R, pattern, 10 + f, 0.5 if pattern == "null" else 48.0 / R), _counts(R, pattern)
        person = np.zeros((B, R), np.int64)
        for b, hits in enumerate(taking_part(flags, count)):
            d, n = np.arange(len(hits)), min(len(hits), TR.TRACK_MAX_D)
            person[b, hits] = d if f == 0 else np.where(d < n, n - 1 - d, d)    # frame 1: the first 64 the other way round
        frames.append((_dets(flags, person, np.full((B, R), 3 * f)), count, flags))
    buf = TR.new_buffers(B, TRACK["T"], J, R)
    snaps = []
    for dets, count, _ in frames:
        TR.update(dets, count, buf, TRACK["max_dist"], TRACK["max_misses"], TRACK["min_hits"])
        snaps.append({k: np.array(v, copy=True) for k, v in buf.items()})
    return dict(frames=frames, want=snaps)


# ---- mvg_track_eval -----------------------------------------------------------------------------------------------------------------
SCORE = dict(G=8, P=8, K=640, dist_thr=500.0)
SCORE_KEYS = ("last_track", "counters", "dist_sum", "seen", "covered", "overlap")


@functools.lru_cache(maxsize=None)
def score_case(R, pattern):
    """two frames of mvg_track_eval and tests/trackeval_ref.py over them.  A participating row carries its row number as id,
    every third one none (unreported); the d-th participating row stands 1 + d steps from person d % G."""
    G = SCORE["G"]
    j3d = np.zeros((B, G, J, 3), np.float32)
    j3d[:] = SKELETON + (np.arange(G) * FAR)[:, None, None] * STEP
    vis = (np.random.default_rng(R + 1).uniform(size=(B, G, J)) > 0.4).astype(np.float32)
    vis[:, :, 0] = 1.0
    num = np.full((B,), G, np.int32)
    frames = []
    for f in range(2):
        flags, count = _flags(R, pattern, 20 + f, 0.5 if pattern == "null" else 60.0 / R), _counts(R, pattern)
        person, steps = np.zeros((B, R), np.int64), np.zeros((B, R), np.int64)
        ids = np.full((B, R), -1, np.int32)
        for b, hits in enumerate(taking_part(flags, count)):
            hits = np.array(hits, np.int64)
            person[b, hits], steps[b, hits] = np.arange(len(hits)) % G, 1 + np.arange(len(hits))
            ids[b, hits] = np.where(np.arange(len(hits)) % 3 == 2, -1, hits)
            if pattern in ("n64", "n65"):
                ids[b, hits] = hits                                            # every participating row is a hypothesis
        frames.append((_dets(flags, person, steps), count, ids, flags))
    buf = ER.new_buffers(B, SCORE["P"], SCORE["K"])
    snaps = []
    for dets, count, ids, _ in frames:
        ER.update(dets, count, ids, j3d, vis, num, buf, SCORE["dist_thr"])
        snaps.append({k: np.array(v, copy=True) for k, v in buf.items()})
    return dict(frames=frames, joints_3d=j3d, vis=vis, num_person=num, want=snaps)
