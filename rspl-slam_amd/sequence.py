"""Keyframe sequence driver for the map-side local BA: what MapBuilder does with each new keyframe
once tracking has produced it -- Map::InsertKeyframe's bookkeeping (src/map.cc:24-103) followed
by Map::LocalMapOptimization (:105-107) on the GPU -- and the trajectory it leaves
(Map::SaveKeyframeTrajectory, :1007-1024).  Input: synthetic.map_sequence (tracking output with
ground truth) for ``run``, whose landmarks arrive ready-made; synthetic.raw_sequence for ``run_raw``, which
goes through keyframe insertion itself (the KeyframeBuilder's stereo stage, new landmarks, triangulation:
src/map_builder.cc:639-682, src/frame.cc:150-177, src/map.cc:24-109).  Tracking and keyframe selection are
not on this path.
"""
from __future__ import annotations

import time

import numpy as np

from .ba_types import OptimizationConfig
from .mapping import Map


def insert_keyframe(m: Map, kf: dict):
    """Map::InsertKeyframe bookkeeping: the frame, its new landmarks, every observation."""
    m.InsertKeyframe(kf["id"], kf["timestamp"], kf["Twc"], kf["keypoints"], kf["lines_left"], kf["lines_right"],
                     kf["lines_right_valid"], kf["points_on_lines"], kf["parent_id"])
    if kf["new_points"]:
        m.InsertMappoints([i for i, _ in kf["new_points"]], np.array([p for _, p in kf["new_points"]]))
    for i, L in kf["new_lines"]:
        m.InsertMapline(i, L)
    if kf["point_obs"]:
        ob = np.array(kf["point_obs"], np.int32)
        m.AddPointObservations(kf["id"], ob[:, 0], ob[:, 1])
    for i, j in kf["line_obs"]:
        m.AddLineObservation(i, kf["id"], j)


def run(seq: dict, ba, cfg: OptimizationConfig = OptimizationConfig(), iterations=(10, 5), on_keyframe=None):
    """Every keyframe of `seq` into a new Map, with LocalMapOptimization (GPU BA handle `ba`) from the
    second keyframe on.  Returns (map, per-keyframe reports)."""
    m = Map(seq["camera"], cfg, iterations)
    reports = []
    for k, kf in enumerate(seq["keyframes"]):
        t = time.perf_counter()
        insert_keyframe(m, kf)
        t_ins = time.perf_counter() - t
        if k >= 1:  # map.cc:29 (the first keyframe only initialises) and :105-107
            r = m.LocalMapOptimization(kf["id"], ba)
            r["insert_us"] = 1e6 * t_ins  # the keyframe's bookkeeping through the Python API
            reports.append(r)
        if on_keyframe:
            on_keyframe(k, m)
    return m, reports


def run_raw(seq: dict, ba, kf, cfg: OptimizationConfig = OptimizationConfig(), iterations=(10, 5), on_keyframe=None,
            tracker=None):
    """Every keyframe of a ``synthetic.raw_sequence`` through keyframe insertion itself: the stereo stage of
    the KeyframeBuilder ``kf`` on the device (u_right, depth, track ids, new map points; the first keyframe
    with ``init``), then Map.InsertKeyframeFull -- landmarks, observers, point triangulation on ``kf``'s
    device, line triangulation, and LocalMapOptimization on ``ba`` from the second keyframe on (``ba`` None:
    none).  ``tracker``: a Tracker whose slot 0 the stereo stage fills for every keyframe.
    Returns (map, per-keyframe reports, the stereo stage's per-keyframe results)."""
    from . import capi
    m = Map(seq["camera"], cfg, iterations)
    reports, stages = [], []
    next_tid, next_line = 0, 0

    def dev(a):
        a = np.ascontiguousarray(a)
        b = capi.DeviceBuffer(max(a.nbytes, 8))
        if a.nbytes:
            b.upload(a)
        return b

    for k, f in enumerate(seq["keyframes"]):
        n = len(f["feat_left"])
        held = f["point_slot"] >= 0
        pts, state = np.zeros((n, 3)), np.zeros(n, np.uint8)
        for i in np.flatnonzero(held):
            p, t, _ = m.GetMappoint(int(f["point_slot"][i]))
            pts[i], state[i] = p, 1 if t == 1 else 2
        fr = dict(d_features_left=dev(f["feat_left"]), d_features_right=dev(f["feat_right"]),
                  d_n_left=dev(np.array([n], np.int32)), d_n_right=dev(np.array([len(f["feat_right"])], np.int32)),
                  d_idx0=dev(f["idx0"]), d_idx1=dev(f["idx1"]), cam=seq["camera"], window=seq["window"], Twc=f["Twc"],
                  next_track_id=next_tid, init=k == 0, track_id=f["track_id"], point_slot=f["point_slot"],
                  points=pts, state=state)
        if tracker is not None:
            fr["table"] = tracker.keyframe_table(0, n)
        kf.enqueue([fr])
        s = kf.fetch()[0]
        next_tid = s["next_track_id"]
        kp = np.column_stack([f["feat_left"][:, 1:3], s["u_right"]]) if n else np.zeros((0, 3))
        tracks = dict(track_id=s["track_id"], point_slot=f["point_slot"], new_point=s["new_point"],
                      new_position=s["new_position"], line_track_id=f["line_track_id"], line_slot=f["line_slot"],
                      next_line_track_id=next_line)
        r = m.InsertKeyframeFull(f["id"], f["timestamp"], f["Twc"], kp, tracks, f["lines_left"], f["lines_right"],
                                 f["lines_right_valid"], f["points_on_lines"], f["parent_id"], kf=kf, ba=ba)
        next_line = r["next_line_track_id"]
        reports.append(r)
        stages.append(s)
        if on_keyframe:
            on_keyframe(k, m)
    return m, reports, stages


def keyframe_trajectory(m: Map, seq: dict) -> np.ndarray:
    """[n][4][4] current keyframe poses T_wc in insertion order."""
    return np.array([m.GetPose(kf["id"]) for kf in seq["keyframes"]])
