"""Decoder-side equivalent of the reference's inference entry point ``run/validate_3d.py`` (SURVEY.md section 8 b, "Entry
points"): reads the SAME YAML files, builds the decoder head behind the reference's class surface, optionally fills it from
a published checkpoint, runs the frames through the HIP path and post-processes the predictions like
``validate_3d.py:185-284`` (classification filter at every ``DECODER.inference_conf_thr``, nearby-joints NMS with the
default 0.3 m / 7 joints, AP / recall / MPJPE or PCP when ground truth is given).

    python -m mvgformer_amd.validate --cfg configs/panoptic/knn5-lr4-q1024-g8.yaml --model_path model_best.pth.tar
    python -m mvgformer_amd.validate --cfg extract:configs/panoptic/knn5-lr4-q1024-g8.yaml --frames 8        # GPU box

The backbone (PoseResNet-50) and the dataset loaders are out of scope: the frames are either a
``--frames-npz`` file holding what the backbone hands to the decoder (``feat0..feat{L-1}`` (F, V, C, H_l, W_l), the per-view
camera arrays of ``meta`` and optionally ``joints_3d`` / ``joints_3d_vis``), or seeded synthetic frames of the YAML's
geometry (``mvgformer_amd.synthetic``).  ``--cfg extract:<relative path>`` reads the values of the reference's YAML from
``mvgformer_amd/data/yaml_extract.json`` where the reference tree does not exist.

``--device-nms 1`` runs the classification filter and the NMS on the device (inside the HIP graph with ``--graph 1``);
``--device-eval 1`` on top of it scores the kept poses against the ground truth there as well (``evaluate.DeviceEvaluator``): the
frame loop then reads nothing back and the metrics are fetched once per threshold.  ``--device-track 1``, also on top of
``--device-nms 1``, follows the kept poses across the frames with a ``tracking.PoseTracker`` (inside the HIP graph with
``--graph 1``) and reports the tracker's counters per threshold; ``--device-track-motion 1`` on top of it turns on the tracker's
constant-velocity motion model.  ``--device-refine 1 --bone-lengths FILE.npy`` (on top of ``--device-nms 1``) re-solves the kept
poses under the J-1 bone lengths of the file (mm) by structural triangulation (``structural.StructuralRefiner``, inside the HIP
graph with ``--graph 1``) and reports the share of kept rows it solved and their mean absolute bone-length residual
before and after.  ``--bone-lengths track`` (with ``--device-track 1``; ``--bone-window``, ``--bone-min-frames``,
``--bone-fallback FILE.npy``) solves every kept pose under the lengths estimated over its own track instead
(``structural.BoneLengthEstimator``, one more launch between the tracker and the refiner); the report then also says which share of
the kept rows took their track's lengths, the fallback or their own, and the residual is taken against the lengths each row was
solved under.  ``--device-track-eval 1`` (on top of ``--device-track 1``) scores the track ids against the ground-truth
identities of frames that carry ``joints_3d`` (``tracking.TrackEvaluator``: CLEAR-MOT counts, MOTA, MOTP, IDF1 per threshold).
All of these stages are one ``postprocess.PostProcess`` per threshold, in both modes: the runner's (``runner.post``) with
``--graph 1``, one built from the same options and run behind the eager head with ``--graph 0``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_config(spec):
    """YAML path -> cfg namespace; ``extract:<rel>`` -> the same namespace from the committed extract of that file."""
    from .factory import load_yaml_config
    if not spec.startswith("extract:"):
        return load_yaml_config(spec)
    with open(os.path.join(ROOT, "mvgformer_amd", "data", "yaml_extract.json")) as f:
        val = json.load(f)[spec[len("extract:"):]]
    return SimpleNamespace(DECODER=SimpleNamespace(**val["DECODER"]), NETWORK=SimpleNamespace(IMAGE_SIZE=val["IMAGE_SIZE"]),
                           MULTI_PERSON=SimpleNamespace(SPACE_SIZE=val["SPACE_SIZE"], SPACE_CENTER=val["SPACE_CENTER"]),
                           DATASET=SimpleNamespace(CAMERA_NUM=val["CAMERA_NUM"]),
                           DEBUG=SimpleNamespace(VISUALIZATION_JUMP_NUM=-1))


def build_head(cfg, device, dtype):
    """DecoderHead with the YAML's hyper-parameters (dq_transformer.py:129-205 without backbone / criterion)."""
    from .caller import DecoderHead
    from .factory import build_decoder_from_cfg
    d = cfg.DECODER
    conv = getattr(d, "convert_joint_format_indices", None)
    head = DecoderHead(build_decoder_from_cfg(cfg), d.num_instance, d.num_keypoints, d.d_model,
                       cfg.MULTI_PERSON.SPACE_SIZE, cfg.MULTI_PERSON.SPACE_CENTER, conv)
    head = head.to(device).eval()
    head.decoder.set_compute_dtype(dtype)
    return head


def load_checkpoint(head, path):
    """``model.load_state_dict(torch.load(path), strict=False)`` (validate_3d.py:160-166): the decoder head takes the keys it
    owns (``decoder.*``, ``joint_embedding.*``, ``instance_embedding.*``; a DDP ``module.`` prefix is dropped)."""
    sd = torch.load(path, map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    own = set(head.state_dict())
    missing, unexpected = head.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=False)
    return sorted(missing), sorted(k for k in sd if k not in own)


def synthetic_frames(cfg, n_frames, seed=0):
    """seeded stand-ins for (backbone features, meta) of the YAML's geometry: ring cameras around the space centre"""
    from .synthetic import make_meta, make_pyramid, pyramid_shapes, ring_cameras
    V = cfg.DATASET.CAMERA_NUM
    img_wh = tuple(cfg.NETWORK.IMAGE_SIZE)
    orig_wh = (1920, 1080) if img_wh[0] >= 900 else (int(img_wh[0] * 1.29), int(img_wh[1] * 1.2763))
    shapes = pyramid_shapes(img_wh)
    for f in range(n_frames):
        cams = ring_cameras(V, orig_wh, 1400.0 * orig_wh[0] / 1920.0, 4000.0, cfg.MULTI_PERSON.SPACE_CENTER,
                            (-0.1, 0.05, 0.0), (1e-3, -1e-3), seed + f)
        yield make_pyramid(V, 1, shapes, seed=seed + f), make_meta(cams, 1, orig_wh, img_wh), None


def npz_frames(path):
    z = np.load(path)
    L = len([k for k in z.files if k.startswith("feat")])
    F, V = z["feat0"].shape[:2]
    for f in range(F):
        src = [torch.from_numpy(z["feat%d" % l][f]) for l in range(L)]
        meta = []
        for v in range(V):
            cam = {k: torch.from_numpy(np.asarray(z["camera_" + k][f, v]))[None] for k in ("R", "T", "fx", "fy", "cx", "cy", "k", "p")}
            meta.append(dict(camera=cam, center=torch.from_numpy(z["center"][f, v])[None],
                             scale=torch.from_numpy(z["scale"][f, v])[None],
                             inv_affine_trans=torch.from_numpy(z["inv_affine_trans"][f, v])[None]))
        gt = (z["joints_3d"][f], z["joints_3d_vis"][f]) if "joints_3d" in z.files else None
        yield src, meta, gt


def to_device(meta, device):
    mv = lambda t: t.to(device)
    return [{k: ({kk: mv(vv) for kk, vv in v.items()} if isinstance(v, dict) else mv(v)) for k, v in m.items()} for m in meta]


def actor_ground_truth(gts, gts_vis):
    """per-frame ground truth (G, 14, 3) + visibility -> evaluate_pcp's actor_gts: person slot g is actor g, and an actor is not
    annotated (None) in a frame where its visibility is all zero"""
    n_actor = max(len(g) for g in gts)
    return [[np.asarray(g[a], np.float64) if a < len(g) and np.any(np.asarray(v[a]) != 0) else None for g, v in zip(gts, gts_vis)]
            for a in range(n_actor)]


def device_ground_truth(frames, kind, num_joints, device):
    """--device-eval: per frame the evaluator's inputs (joints_3d (1, G, J, 3) fp32, joints_3d_vis (1, G, J) fp32, num_person (1)
    int32) on the device, built before the frame loop; G = the largest person count.  kind None (no ground truth, or none that is
    scored): num_person 0 everywhere, the evaluator only counts the kept poses.  Visibility is reduced the way the host scoring
    reads it: its first component for Panoptic (match_predictions), "some component != 0" for PCP (actor_ground_truth)."""
    scored = [f[2] for f in frames if f[2] is not None and kind is not None]
    G = max([len(gt[0]) for gt in scored] + [1])
    out = []
    for _, _, gt in frames:
        j3d, vis, n = torch.zeros((1, G, num_joints, 3)), torch.zeros((1, G, num_joints)), 0
        if gt is not None and kind is not None and len(gt[0]):
            g, v = np.asarray(gt[0]), np.asarray(gt[1])
            n = len(g)
            j3d[0, :n] = torch.from_numpy(g[..., :3].astype(np.float32))
            seen = v[..., 0] > 0 if kind == "panoptic" else (v != 0).reshape(n, num_joints, -1).any(-1)
            vis[0, :n] = torch.from_numpy(seen.astype(np.float32))
        out.append((j3d.to(device), vis.to(device), torch.tensor([n], dtype=torch.int32, device=device)))
    return G, out


def track_ground_truth(frames, gt_dev, person_ids, persons, device):
    """--device-track-eval: per frame the TrackEvaluator's inputs, the evaluator's (device_ground_truth) with num_person = -1 for a
    frame without ground truth (it is skipped, not scored as empty) and person_id (1, G) int32: slot g is identity g unless the
    npz's person_ids (F, G') says otherwise"""
    out = []
    for fi, ((_, _, gt), (j3d, vis, num)) in enumerate(zip(frames, gt_dev)):
        pid = torch.arange(persons, dtype=torch.int32)[None].clone()
        if person_ids is not None:
            given = torch.from_numpy(np.asarray(person_ids[fi]).astype(np.int32))[:persons]
            pid[0, :len(given)] = given
        out.append((j3d, vis, num if gt is not None else torch.full_like(num, -1), pid.to(device)))
    return out


def pcp_report(kept, gts, gts_vis, evaluator=None):
    """the PCP entry of a result row (Shelf.evaluate / Campus.evaluate through evaluate.evaluate_pcp, or the counters of a
    DeviceEvaluator), in percent"""
    from . import evaluate as E
    try:
        actor, avg, bones, recall = evaluator.pcp() if evaluator is not None else E.evaluate_pcp(kept, actor_ground_truth(gts, gts_vis))
    except ValueError as e:            # a frame with ground truth in which no prediction passed the classification filter
        return {"error": str(e)}
    return {"actor": [round(100 * float(a), 2) for a in actor], "average": round(100 * float(avg), 2),
            "bones": {k: [round(100 * float(x), 2) for x in v] for k, v in bones.items()},
            "recall500": round(100 * float(recall), 2)}


def parse_view_subsets(text, views):
    """--view-subsets "0,1,2;0,2,4;0,1,2,3,4" -> [(0, 1, 2), (0, 2, 4), (0, 1, 2, 3, 4)]: camera subsets of a rig of `views`
    cameras, each sorted; an empty subset, a repeated camera or one outside the rig is a ValueError"""
    out = []
    for part in text.split(";"):
        try:
            subset = [int(v) for v in part.split(",") if v.strip()]
        except ValueError:
            raise ValueError("--view-subsets: %r is not a comma-separated list of camera numbers" % part) from None
        if not subset:
            raise ValueError("--view-subsets: empty subset in %r" % text)
        if len(set(subset)) != len(subset):
            raise ValueError("--view-subsets: camera repeated in %r" % part)
        if min(subset) < 0 or max(subset) >= views:
            raise ValueError("--view-subsets: %r names a camera outside 0 .. %d" % (part, views - 1))
        out.append(tuple(sorted(subset)))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="decoder-side validate_3d")
    ap.add_argument("--cfg", required=True, help="YAML entry point of the reference, or extract:<path relative to the reference>")
    ap.add_argument("--model_path", default=None, help="checkpoint (validate_3d.py --model_path)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--frames", type=int, default=4, help="synthetic frames when no --frames-npz is given")
    ap.add_argument("--frames-npz", default=None)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--pred-out", default=None, help="save the packed predictions per threshold (TEST.PRED_FILE)")
    ap.add_argument("--graph", type=int, default=1, help="1: the decoder forward captured once as a HIP graph and replayed per "
                                                         "frame (mvgformer_amd.serving.GraphedDecoder); 0: eager launches")
    ap.add_argument("--device-nms", type=int, default=0, choices=[0, 1],
                    help="1: classification filter + NMS as one device operator (ops.pose_nms), inside the HIP graph with --graph 1 "
                         "(one count read-back per frame); 0: evaluate.filter_and_nms (host greedy loop)")
    ap.add_argument("--device-eval", type=int, default=0, choices=[0, 1],
                    help="1 (needs --device-nms 1): the kept poses are scored against the ground truth on the device "
                         "(evaluate.DeviceEvaluator), inside the HIP graph with --graph 1; the frame loop reads nothing back, the "
                         "metrics once per threshold.  Ground truth is taken as fp32.  0: evaluate.evaluate_panoptic / evaluate_pcp")
    ap.add_argument("--device-track", type=int, default=0, choices=[0, 1],
                    help="1 (needs --device-nms 1): the kept poses get person identities across the frames on the device "
                         "(tracking.PoseTracker, one launch per frame, inside the HIP graph with --graph 1); a fresh tracker per "
                         "inference_conf_thr, its counters in the report")
    ap.add_argument("--device-track-motion", type=int, default=0, choices=[0, 1],
                    help="1 (needs --device-track 1): the tracker's constant-velocity motion model with its default parameters "
                         "(tracking.PoseTracker(motion=True), two more launches per frame); the report gains the mean speed of "
                         "the live tracks")
    ap.add_argument("--device-track-eval", type=int, default=0, choices=[0, 1],
                    help="1 (needs --device-track 1 and frames with ground truth): the track ids are scored against the ground-truth "
                         "identities on the device (tracking.TrackEvaluator, one more launch per frame, inside the HIP graph with "
                         "--graph 1); every threshold's row gains \"device_track_eval\" (CLEAR-MOT counts, MOTA, MOTP, IDF1, mostly "
                         "tracked / lost).  Person slot g is identity g unless the npz holds person_ids (F, G); a frame without "
                         "ground truth is skipped")
    ap.add_argument("--device-refine", type=int, default=0, choices=[0, 1],
                    help="1 (needs --device-nms 1 and --bone-lengths): the kept poses are re-solved under fixed bone lengths on the "
                         "device (structural.StructuralRefiner, two more launches per frame, inside the HIP graph with --graph 1)")
    ap.add_argument("--bone-lengths", default=None, help=".npy file with the J-1 bone lengths in mm (entry k-1: the bone that ends "
                                                         "at joint k of structural.PANOPTIC15_PARENT) for --device-refine 1; or "
                                                         "the word \"track\" (needs --device-track 1): every person is solved "
                                                         "under the lengths estimated over its own track "
                                                         "(structural.BoneLengthEstimator, one more launch per frame)")
    ap.add_argument("--refine-steps", type=int, default=1, help="n_steps of --device-refine 1 (1 .. 8)")
    ap.add_argument("--bone-window", type=int, default=8, help="--bone-lengths track: frames of a track the median is taken over")
    ap.add_argument("--bone-min-frames", type=int, default=4, help="--bone-lengths track: samples a track needs before its rows "
                                                                   "are solved under its own lengths")
    ap.add_argument("--bone-fallback", default=None, help="--bone-lengths track: .npy file with the J-1 lengths of a row whose "
                                                          "track is younger (default: the lengths the row has itself)")
    ap.add_argument("--view-subsets", default=None,
                    help="camera subsets, e.g. \"0,1,2;0,2,4;0,1,2,3,4\" (the generalization experiment, configs/panoptic/"
                         "generalization): the frames run once per subset through ONE runner and one capture (the decoder's "
                         "live-view table, serving.GraphedDecoder(live_views=True)); a result row per threshold and subset")
    args = ap.parse_args(argv)
    if args.view_subsets and args.device_refine and not args.graph:
        ap.error("--view-subsets with --device-refine 1 gives the refiner its view weights through the runner: it requires --graph 1")
    track_lengths = args.bone_lengths == "track"
    if args.device_refine and not args.device_nms:
        ap.error("--device-refine 1 re-solves the rows of the device NMS: it requires --device-nms 1")
    if args.device_refine and not args.bone_lengths:
        ap.error("--device-refine 1 holds given bone lengths fixed: it requires --bone-lengths FILE.npy")
    if args.device_refine and track_lengths and not args.device_track:
        ap.error("--bone-lengths track estimates the lengths over the tracks of the device tracker: it requires --device-track 1")
    if args.device_track_motion and not args.device_track:
        ap.error("--device-track-motion 1 is an option of the device tracker: it requires --device-track 1")
    if args.device_track_eval and not args.device_track:
        ap.error("--device-track-eval 1 scores the ids of the device tracker: it requires --device-track 1")
    if args.device_eval and not args.device_nms:
        ap.error("--device-eval 1 scores the rows of the device NMS: it requires --device-nms 1")
    if args.device_track and not args.device_nms:
        ap.error("--device-track 1 follows the rows of the device NMS: it requires --device-nms 1")

    from . import evaluate as E
    cfg = load_config(args.cfg)
    dev = torch.device(args.device)
    if dev.type != "cuda":
        raise SystemExit("Not implemented on the CPU")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    torch.manual_seed(args.seed)
    head = build_head(cfg, dev, dtype)
    report = {"cfg": args.cfg, "dtype": args.dtype, "num_instance": cfg.DECODER.num_instance,
              "views": cfg.DATASET.CAMERA_NUM, "layers": cfg.DECODER.num_decoder_layers, "device_nms": bool(args.device_nms),
              "device_eval": bool(args.device_eval), "device_track": bool(args.device_track)}
    if args.model_path:
        missing, ignored = load_checkpoint(head, args.model_path)
        report["checkpoint"] = {"path": args.model_path, "missing_keys": missing[:8], "n_missing": len(missing),
                                "n_ignored_keys_of_other_modules": len(ignored)}
    frames = list(npz_frames(args.frames_npz) if args.frames_npz else synthetic_frames(cfg, args.frames, args.seed))
    subsets = [None]
    if args.view_subsets:
        try:
            subsets = parse_view_subsets(args.view_subsets, len(frames[0][1]))
        except ValueError as e:
            ap.error(str(e))
        report["view_subsets"] = [list(s) for s in subsets]
    results = []
    from . import caller, ops
    from .postprocess import PostProcess
    from .serving import GraphedDecoder
    conv = getattr(cfg.DECODER, "convert_joint_format_indices", None)
    evaluation, gt_dev = None, None
    j_out = head.num_joints if conv is None else len(conv)
    tracking = dict(max_tracks=32, max_dist=500.0, max_misses=10, min_hits=1) if args.device_track else None
    if args.device_track_motion:
        tracking["motion"] = True
        report["device_track_motion"] = True
    refine = None
    if args.device_refine:
        if track_lengths:
            refine = dict(bone_lengths="track", window=args.bone_window, min_frames=args.bone_min_frames, n_steps=args.refine_steps,
                          fallback=None if args.bone_fallback is None
                          else np.load(args.bone_fallback).astype(np.float32).reshape(-1))
            report["bone_lengths"] = "track"
        else:
            refine = dict(bone_lengths=np.load(args.bone_lengths).astype(np.float32).reshape(-1), n_steps=args.refine_steps)
        report["device_refine"] = True
    if args.device_eval:
        # which metric the ground truth gets (the rule of the host path below), and every frame's ground truth on the device
        with_gt = [f[2] for f in frames if f[2] is not None]
        kind = None if not with_gt else "panoptic" if conv is None else \
            "pcp" if np.asarray(with_gt[0][0]).shape[-2] == len(conv) else None
        persons, gt_dev = device_ground_truth(frames, kind, j_out, dev)
        evaluation = dict(kind=kind or "panoptic", capacity=len(frames) * head.num_instance, max_persons=persons, actors=persons)
    track_evaluation, track_gt = None, None
    if args.device_track_eval:
        if not any(f[2] is not None for f in frames):
            raise SystemExit("--device-track-eval 1 scores the track ids against ground truth: no frame has joints_3d")
        joints = {np.asarray(f[2][0]).shape[-2] for f in frames if f[2] is not None and len(f[2][0])}
        if joints - {j_out}:
            raise SystemExit("--device-track-eval 1: the ground truth has %s joints, the kept poses %d"
                             % (sorted(joints), j_out))
        if gt_dev is None:
            persons, gt_dev = device_ground_truth(frames, "panoptic" if conv is None else "pcp", j_out, dev)
        person_ids = None
        if args.frames_npz and "person_ids" in np.load(args.frames_npz).files:
            person_ids = np.load(args.frames_npz)["person_ids"]
        track_gt = track_ground_truth(frames, gt_dev, person_ids, persons, dev)
        track_evaluation = dict(dist_thr=500.0, max_persons=persons, max_ids=1024)
        report["device_track_eval"] = True
    # the device stages behind the decoder (postprocess.PostProcess; its NMS defaults are validate_3d's 0.3 m / 7 joints) and the
    # ground truth they read, per frame
    stages = dict(postprocess={} if args.device_nms else None, convert_joint_format_indices=head.convert_joint_format_indices,
                  evaluation=evaluation, tracking=tracking, refine=refine, track_evaluation=track_evaluation)
    truths = track_gt or gt_dev
    runner, post, fresh, runner_thr = None, None, None, None
    for thr, subset in [(t, s) for t in cfg.DECODER.inference_conf_thr for s in subsets]:       # validate_3d.py:185
        preds, gts, gts_vis, t_dec, n_timed = [], [], [], 0.0, 0
        kept = []
        view_live = None if subset is None else [v in subset for v in range(len(frames[0][1]))]
        if thr != runner_thr:
            runner, post, runner_thr = None, None, thr      # post: fresh stages (tracker, accumulators) per threshold pass ...
        elif runner is not None and fresh is not None:
            post.restore(fresh)                             # ... and per subset: the same runner, its stages as the capture left them
        if refine is not None:
            refine_sums = torch.zeros(4, dtype=torch.float64, device=dev)        # kept rows, solved rows, residual before, after
            source_sums = torch.zeros(3, dtype=torch.int64, device=dev)
        if args.device_nms and not args.graph:
            post = PostProcess(1, head.num_instance, head.num_joints, thr, dev, **stages)
        for fi, (src, meta, gt) in enumerate(frames):
            src = [s.to(dev) for s in src]
            meta = to_device(meta, dev)
            if args.graph and runner is None:
                # queries and initial poses do not depend on the frame (dq_transformer.py:394-432, 298-323): loaded once
                shapes, starts = caller.level_tables(src)
                runner = GraphedDecoder(head.decoder, meta, shapes, starts, 1, head.num_instance, thr, live_views=subset is not None,
                                        **stages)
                post = runner.post
                qpos, tgt = caller.person_joint_queries(head.joint_embedding.weight, head.instance_embedding.weight, 1)
                ref0 = caller.sample_space_reference_points(head.num_instance, head.space_size, head.space_center, 1, dev,
                                                            t_pose=head.t_pose)
                runner.load(tgt=tgt, query_pos=qpos, reference_points=ref0).capture()
                fresh = None if post is None else post.snapshot()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if runner is not None:
                runner.set_cameras(meta).load(src_views=src, ground_truth=truths[fi] if truths else None, view_live=view_live)
                hs, refs, r2d, p2d, cls = runner.replay()
                if args.device_nms:
                    pred = runner.pred.clone()                                   # static buffer: the next replay overwrites it
                else:
                    out = caller.decoder_outputs_to_dict(hs, refs, r2d, p2d, cls, head.num_instance, head.num_joints,
                                                         head.convert_joint_format_indices)
                    pred = caller.pack_predictions(out, thr)                     # function.py:386-396
            else:
                out, pred = head(src, meta, threshold=thr, view_live=view_live)  # function.py:372-396
            torch.cuda.synchronize()
            if fi > 0 or len(frames) == 1:          # the first frame builds the weight caches / captures the graph (one-time)
                t_dec += time.perf_counter() - t0
                n_timed += 1
            preds.extend(p for p in pred)
            if post is not None and runner is None:                              # with --graph 1 the replay has done it all
                with torch.cuda.device(dev):                                     # launches only: nothing is read back per frame
                    post.set_cameras(ops.pack_cameras(meta, head.decoder.layers[0].img_size, dev), len(meta))
                    if truths:
                        post.load_ground_truth(truths[fi])
                    post.run_packed(pred.contiguous(), out["pred_poses_2d"]["outputs_coord_2d"])
            if refine is not None:                                               # device sums, read back once per threshold
                from .structural import PANOPTIC15_PARENT, bone_lengths
                (poses, status), (dets, count, _) = post.refined, post.detections
                live = torch.arange(poses.shape[1], device=dev)[None] < count[:, :1]
                solved = live & (status == 0)
                want = post.bone_lengths.double()
                before = (bone_lengths(dets[..., :3].double(), PANOPTIC15_PARENT) - want).abs().mean(-1)
                after = (bone_lengths(poses.double(), PANOPTIC15_PARENT) - want).abs().mean(-1)
                if track_lengths:                   # a row's own lengths may be non-finite; such a row is not solved
                    before, after = (torch.where(solved, x, torch.zeros_like(x)) for x in (before, after))
                refine_sums += torch.stack([live.sum(), solved.sum(), (before * solved).sum(), (after * solved).sum()])
                if track_lengths:                                                # kept rows per source of their lengths
                    source_sums += torch.stack([(live & (post.bone_source == s)).sum() for s in (0, 1, 2)])
            if args.device_nms and not args.device_eval:
                dets, count, _ = post.detections                                 # static buffers, overwritten by the next frame
                kept.extend(dets[b, :k].clone() for b, k in enumerate(count[:, 0].tolist()))   # the frame's one read-back
            if gt is not None:
                gts.append(gt[0])
                gts_vis.append(gt[1])
        if not args.device_nms:
            kept = [E.filter_and_nms(p) for p in preds]                          # validate_3d.py:228-234 (0.3 m, 7 joints)
        row = {"inference_conf_thr": thr, "frames": len(preds),
               "candidates_above_thr": int(sum(int((p[:, 0, 3] >= 0).sum()) for p in preds)),
               "poses_after_nms": post.evaluator.state()["kept_rows"] if args.device_eval else int(sum(len(k) for k in kept)),
               "decoder_ms_per_frame": round(1e3 * t_dec / max(n_timed, 1), 3),    # host-timed, incl. the camera H2D copy
               "hip_graph": runner is not None}
        if subset is not None:
            row["view_subset"] = list(subset)
        if args.device_track:
            st = post.tracker.state()
            row["tracks"] = {k: st[k] for k in ("births", "deaths", "overflow", "dropped", "active")}
            if args.device_track_motion:                                         # mean joint speed of the live tracks, unit / frame
                speeds = [float(np.linalg.norm(vel, axis=1).mean()) for vel, _ in post.tracker.motion()[0].values()]
                row["track_motion"] = {"tracks": len(speeds), "mean_speed": round(sum(speeds) / max(len(speeds), 1), 3)}
        if args.device_track_eval:                                               # the one read-back of the tracking scores
            scores = post.track_evaluator.report()
            row["device_track_eval"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in scores["total"].items()}
            if "note" in scores:
                row["device_track_eval"]["note"] = scores["note"]
        if refine is not None:
            n_live, n_solved, before, after = refine_sums.tolist()
            row["refine"] = {"kept_rows": int(n_live), "solved_share": round(n_solved / max(n_live, 1.0), 4),
                             "bone_residual_mm_before": round(before / max(n_solved, 1.0), 4),
                             "bone_residual_mm_after": round(after / max(n_solved, 1.0), 4)}
            if track_lengths:
                row["refine"]["length_source_share"] = {
                    name: round(n / max(n_live, 1.0), 4) for name, n in zip(("track", "fallback", "own"), source_sums.tolist())}
        if gts and conv is not None:
            if np.asarray(gts[0]).shape[-2] == len(conv):
                row["PCP"] = pcp_report(kept, gts, gts_vis, post.evaluator if args.device_eval else None)   # shelf.py:255-330
        elif gts:
            aps, recs, mpjpe, recall500 = post.evaluator.panoptic() if args.device_eval else \
                E.evaluate_panoptic(kept, gts, gts_vis)                          # panoptic.py:493-574
            row.update(AP={str(t): round(100 * a, 2) for t, a in zip(E.MPJPE_THRESHOLDS, aps)},
                       recall={str(t): round(100 * r, 2) for t, r in zip(E.MPJPE_THRESHOLDS, recs)},
                       MPJPE=round(float(mpjpe), 2), recall500=round(100 * float(recall500), 2))
        if args.pred_out:
            np.save("%s-%s.npy" % (args.pred_out, thr), np.stack([p.cpu().numpy() for p in preds]))
        results.append(row)
    report["results"] = results
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
