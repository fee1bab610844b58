"""Center-based multi-object tracking: the reference's `PubTracker.step_centertrack` (tools/nusc_tracking/pub_tracker.py:49-154,
tools/waymo_tracking/tracker.py:42-136) behind `transform_box` (tools/waymo_tracking/test.py:160-183), over csrc/tracking.hip.

    Tracker           up to 64 sequences (segments) stepped together in ONE launch; the track lists stay on the device
    StaticTracker     the same step on the padded, device-counted StaticDetections of CenterHead.predict_static, read where they lie: every
                      buffer allocated once, time lag and buffer parity formed on the device, one launch that a HIP graph can hold (alone
                      or behind StaticPredictPlan.run); pack_padded + step_host is its host definition
    step_host         the numpy restatement on arrays with the same state layout: the definition the tests use, the path of CPU tensors
                      and of S2D_TRACK_DEVICE=0
    PubTracker        the reference's class on lists of dictionaries (both constructor signatures), over the same association
    decision_clear    no decision of a step can flip when every distance moves by up to a margin

A step: boxes [R, 9] fp32 in the lidar frame go to the global frame with the segment's 4x4 pose in float64 (centre = R xyz + t, velocity =
R[:2, :2] (vx, vy)); labels that are no tracking class are dropped; `tracking = velocity * -1 * time_lag` in float64; the matching centre is
float32(ct + float64(float32(tracking))), a track's is float32(ct); dist = sqrt(dx * dx + dy * dy) in float32 without contraction; a pair is
invalid when dist > max_diff[detection] or the classes differ; detections in input order take the free valid track of smallest dist (lowest
index on equal dist).  New list: matched detections (the track's id, age 1, active + 1), unmatched detections (id = ++id_count, age 1,
active 1; with a score threshold only those with score > threshold, compared in float32 as numpy >= 2 compares a float32 with a Python
float), unmatched old tracks with age < max_age (age + 1, active 0, ct - tracking with the tracking of their last detection).  A frame with
no rows clears the tracks and keeps id_count; only `first` (the reference's reset()) resets it.

THE SINGLE DEVIATION: with rows present but every one filtered the reference raises IndexError at `results[0]`; here that is the ordinary
path with no detection: every track is unmatched and ages.

State per segment (capacity MAX_TRACKS): ct, tracking float64 [S, cap, 2], meta int32 [S, cap, 4] = class, id, age, active, head int32
[S, 2] = count, id_count.  Limits: 64 segments, 1024 detections per segment and step, 4096 tracks per segment (checked on the host without
a read: a segment's tracks never exceed the rows of its last max_age + 1 frames summed).  Launches per step on the device: 1, plus one
concatenation per field when the detections arrive as per-sample dictionaries; one upload (segment table and row offsets), no host read.

Out of scope: Hungarian assignment (the reference's branch names an undefined function), any state beyond the reference's, the nuScenes
JSON / Waymo .bin writers and the metric programs, HIP-graph capture of `Tracker.step` (its parity is a host integer; `StaticTracker.run`
is the capturable step)."""
import os

import numpy as np
import torch

from . import _lib

MAX_SEGMENTS, MAX_DETS, MAX_TRACKS = 64, 1024, 4096   # S2D_TRACK_MAX_SEGMENTS / _DETS / _TRACKS
STEP_LAUNCHES, STEP_HOST_READS, STEP_UPLOADS = 1, 0, 1
STATIC_STEP_LAUNCHES, STATIC_STEP_HOST_READS, STATIC_STEP_UPLOADS = 1, 0, 1   # the upload is set_frames' frame block, outside the capture

NUSCENES_TRACKING_NAMES = ["bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck"]
NUSCENE_CLS_VELOCITY_ERROR = {"car": 4, "truck": 4, "bus": 5.5, "trailer": 3, "pedestrian": 1, "motorcycle": 13, "bicycle": 3}
WAYMO_TRACKING_NAMES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]

_SEGMENT = np.dtype([("pose", np.float64, (12,)), ("time_lag", np.float64), ("first", np.int32), ("skip", np.int32), ("row_lo", np.int32),
                     ("row_hi", np.int32)])   # s2d_track_segment
assert _SEGMENT.itemsize == 120
_FRAME = np.dtype([("pose", np.float64, (12,)), ("stamp", np.float64), ("first", np.int32), ("skip", np.int32)])   # s2d_track_frame
assert _FRAME.itemsize == 112


# ---- tables and state ----------------------------------------------------------------------------------------------------------------
def class_table_of(detection_names, tracking_names, max_dist):
    """[(tracking class or -1, max_diff)] per detection label: the class is the name's index in tracking_names, as the reference's
    `label_preds` of a track"""
    return [(tracking_names.index(n), float(max_dist[n])) if n in tracking_names else (-1, 0.0) for n in detection_names]


def _table_arrays(class_table):
    cls = np.array([int(c) for c, _ in class_table], np.int32)
    diff = np.array([d for _, d in class_table], np.float32)
    if not 1 <= len(cls) <= 127 or cls.max(initial=-1) > 126:
        raise _lib.S2DError(f"class_table: {len(cls)} labels (1..127) with tracking classes up to 126")
    return np.where(cls < 0, -1, cls).astype(np.int32), diff


def new_state(segments, capacity=MAX_TRACKS):
    return dict(ct=np.zeros((segments, capacity, 2), np.float64), tracking=np.zeros((segments, capacity, 2), np.float64),
                meta=np.zeros((segments, capacity, 4), np.int32), head=np.zeros((segments, 2), np.int32))


def _poses(poses, segments):
    p = np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, np.float64)
    if p.shape not in ((segments, 4, 4), (segments, 3, 4)):
        raise ValueError(f"poses {p.shape}: [{segments}, 4, 4] (or [.., 3, 4]) float64 lidar-to-global matrices expected")
    return np.ascontiguousarray(p[:, :3, :])


def _flags(v, segments, default):
    if v is None:
        return np.full(segments, default, np.bool_)
    v = np.asarray(v, np.bool_).reshape(-1)
    if v.shape[0] != segments:
        raise ValueError(f"{v.shape[0]} flags for {segments} segments")
    return v


def _offsets(offsets, segments, rows):
    if torch.is_tensor(offsets):
        if offsets.is_cuda:
            raise TypeError("row offsets must be host values (a list, an array or a CPU tensor): the limits are checked without a host read")
        offsets = offsets.numpy()
    off = np.asarray(offsets, np.int64).reshape(-1)
    if off.shape[0] != segments + 1 or off[0] != 0 or off[-1] != rows or np.any(np.diff(off) < 0):
        raise _lib.S2DError(f"offsets: {segments + 1} non-decreasing entries from 0 to {rows} expected")
    if np.diff(off).max(initial=0) > MAX_DETS:
        raise _lib.S2DError(f"{int(np.diff(off).max())} detections in one segment: at most {MAX_DETS} per segment and step")
    return off


# ---- the association on global centres (one segment) ---------------------------------------------------------------------------------
def _centres(ct, tracking):
    """the float32 centre a detection is matched with: ct + tracking.astype(float32), rounded to float32"""
    return (ct + tracking.astype(np.float32).astype(np.float64)).astype(np.float32)


def _dist(det, trk):
    """float32 [N, M], the reference's (((tracks - dets) ** 2).sum(2)) ** 0.5"""
    d = trk[None, :, :] - det[:, None, :]
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def _associate(old, ct, tracking, cls, max_diff, score, max_age, score_thresh):
    """one reference step of one segment on the kept detections.  old: dict(ct [M, 2], tracking [M, 2], meta [M, 4]), id_count.
    Returns (new dict, id_count, tracking_id [N], active [N], sources) with sources = [("det", i) | ("trk", j)] naming where every entry
    of the new list comes from."""
    n, m = ct.shape[0], old["ct"].shape[0]
    match = np.full(n, -1, np.int64)
    if n and m:
        dist = _dist(_centres(ct, tracking), old["ct"].astype(np.float32))
        valid = (dist <= max_diff[:, None]) & (cls[:, None] == old["meta"][None, :, 0])
        dist = np.where(valid, dist, np.float32(np.inf))
        best = dist.argmin(1)
        taken = np.zeros(m, np.bool_)
        for i in range(n):
            j = best[i]
            if taken[j]:
                row = np.where(taken, np.float32(np.inf), dist[i])
                j = row.argmin()
                if not np.isfinite(row[j]):
                    continue
            elif not np.isfinite(dist[i, j]):
                continue
            taken[j], match[i] = True, j
    matched = match >= 0
    fresh = ~matched if score_thresh is None else ~matched & (score > np.float32(score_thresh))
    survive = np.ones(m, np.bool_)
    survive[match[matched]] = False
    survive &= old["meta"][:, 2] < max_age
    id_count = int(old["id_count"])
    tid, act = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    tid[matched], act[matched] = old["meta"][match[matched], 1], old["meta"][match[matched], 3] + 1
    tid[fresh], act[fresh] = id_count + 1 + np.arange(int(fresh.sum())), 1
    order = np.concatenate([np.nonzero(matched)[0], np.nonzero(fresh)[0]])
    meta_det = np.stack([cls[order], tid[order], np.ones(len(order), np.int32), act[order]], 1).astype(np.int32).reshape(-1, 4)
    kept = np.nonzero(survive)[0]
    meta_old = old["meta"][kept].copy()
    meta_old[:, 2] += 1
    meta_old[:, 3] = 0
    new = dict(ct=np.concatenate([ct[order], old["ct"][kept] - old["tracking"][kept]], 0),
               tracking=np.concatenate([tracking[order], old["tracking"][kept]], 0), meta=np.concatenate([meta_det, meta_old], 0))
    sources = [("det", int(i)) for i in order] + [("trk", int(j)) for j in kept]
    return new, id_count + int(fresh.sum()), tid, act, sources


def _to_global(boxes, pose, time_lag):
    """transform_box on the columns the tracker reads, float64: (ct [N, 2], tracking [N, 2])"""
    b = boxes.astype(np.float64)
    x, y, z, vx, vy = b[:, 0], b[:, 1], b[:, 2], b[:, 6], b[:, 7]
    ct = np.stack([((pose[0, 0] * x + pose[0, 1] * y) + pose[0, 2] * z) + pose[0, 3],
                   ((pose[1, 0] * x + pose[1, 1] * y) + pose[1, 2] * z) + pose[1, 3]], 1)
    vel = np.stack([pose[0, 0] * vx + pose[0, 1] * vy, pose[1, 0] * vx + pose[1, 1] * vy], 1)
    return ct, vel * -1 * time_lag


def _np(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def _check_boxes(shape):
    if len(shape) != 2 or shape[1] != 9:
        raise ValueError(f"boxes {tuple(shape)}: [R, 9] expected (velocity in columns 6 and 7, which the reference's driver indexes; "
                         "7-column boxes carry none)")


def _segment_inputs(state, seg, boxes, labels, offsets, poses, time_lags, first, cls_of, diff_of):
    """(old lists of the segment after `first`, kept rows, ct, tracking, cls, max_diff) of one segment that is not skipped"""
    lo, hi = int(offsets[seg]), int(offsets[seg + 1])
    count, id_count = (0, 0) if first[seg] else (int(state["head"][seg, 0]), int(state["head"][seg, 1]))
    old = dict(ct=state["ct"][seg, :count], tracking=state["tracking"][seg, :count], meta=state["meta"][seg, :count], id_count=id_count)
    lab = labels[lo:hi]
    ok = (lab >= 0) & (lab < len(cls_of))
    cls = np.where(ok, cls_of[np.where(ok, lab, 0)], -1)
    rows = lo + np.nonzero(cls >= 0)[0]
    ct, tracking = _to_global(boxes[rows], poses[seg], time_lags[seg])
    return old, rows, ct, tracking, cls[cls >= 0].astype(np.int32), diff_of[labels[rows]]


def step_host(state, boxes, labels, scores, offsets, poses, time_lags, first, skip, class_table, max_age, score_thresh=None):
    """One step of every segment in numpy; `state` (new_state) is updated in place.  boxes [R, 9] fp32, labels [R], scores [R],
    offsets [S + 1], poses [S, 4, 4] float64, time_lags [S] float64, first / skip [S] bool.  Returns (tracking_id [R], active [R]) int32."""
    segments = state["head"].shape[0]
    boxes, labels, scores = _np(boxes, np.float32), _np(labels, np.int64), _np(scores, np.float32)
    _check_boxes(boxes.shape)
    offsets = _offsets(offsets, segments, boxes.shape[0])
    poses, time_lags = _poses(poses, segments), np.asarray(time_lags, np.float64).reshape(-1)
    first, skip = _flags(first, segments, False), _flags(skip, segments, False)
    cls_of, diff_of = _table_arrays(class_table)
    tid, act = np.full(boxes.shape[0], -1, np.int32), np.zeros(boxes.shape[0], np.int32)
    for seg in range(segments):
        if skip[seg]:
            continue
        if offsets[seg + 1] == offsets[seg]:
            state["head"][seg] = (0, 0 if first[seg] else state["head"][seg, 1])
            continue
        old, rows, ct, tracking, cls, diff = _segment_inputs(state, seg, boxes, labels, offsets, poses, time_lags, first, cls_of, diff_of)
        new, id_count, tid[rows], act[rows], _ = _associate(old, ct, tracking, cls, diff, scores[rows], max_age, score_thresh)
        count = new["ct"].shape[0]
        if count > state["ct"].shape[1]:
            raise _lib.S2DError(f"segment {seg}: {count} tracks, at most {state['ct'].shape[1]}")
        state["ct"][seg, :count], state["tracking"][seg, :count], state["meta"][seg, :count] = new["ct"], new["tracking"], new["meta"]
        state["head"][seg] = (count, id_count)
    return tid, act


def decision_clear(state, boxes, labels, offsets, poses, time_lags, first, skip, class_table, margin):
    """True when no decision of the step that `step_host` would take from `state` can flip if every distance moves by up to `margin`:
    every same-class pair keeps |dist - max_diff| > margin, and every detection's best and second-best valid distances differ by more
    than margin or are exactly equal (an exact tie is decided by index).  The analogue of prep.collision_clear; float64 on the float32
    centres."""
    segments = state["head"].shape[0]
    boxes, labels = _np(boxes, np.float32), _np(labels, np.int64)
    offsets = _offsets(offsets, segments, boxes.shape[0])
    poses, time_lags = _poses(poses, segments), np.asarray(time_lags, np.float64).reshape(-1)
    first, skip = _flags(first, segments, False), _flags(skip, segments, False)
    cls_of, diff_of = _table_arrays(class_table)
    for seg in range(segments):
        if skip[seg] or offsets[seg + 1] == offsets[seg]:
            continue
        old, _, ct, tracking, cls, diff = _segment_inputs(state, seg, boxes, labels, offsets, poses, time_lags, first, cls_of, diff_of)
        if not len(cls) or not len(old["ct"]):
            continue
        det, trk = _centres(ct, tracking).astype(np.float64), old["ct"].astype(np.float32).astype(np.float64)
        dist = np.sqrt(((trk[None] - det[:, None]) ** 2).sum(2))
        same = cls[:, None] == old["meta"][None, :, 0]
        gate = diff.astype(np.float64)[:, None]
        if np.any(same & (np.abs(dist - gate) <= margin)):
            return False
        ranked = np.sort(np.where(same & (dist <= gate), dist, np.inf), 1)
        if ranked.shape[1] >= 2:
            two = np.isfinite(ranked[:, 1])
            gap = ranked[two, 1] - ranked[two, 0]
            if np.any((gap != 0) & (gap <= margin)):
                return False
    return True


# ---- the device tracker --------------------------------------------------------------------------------------------------------------
def _stream(dev):
    return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())


class Tracker:
    """`segments` sequences tracked side by side.  class_table: per detection label (tracking class or -1, max_diff); score_thresh None:
    every unmatched detection starts a track (nuScenes), a number: only those with score > score_thresh (Waymo).  device: a CUDA device
    runs csrc/tracking.hip and keeps the state there; "cpu" (and S2D_TRACK_DEVICE=0) runs step_host."""

    def __init__(self, segments, class_table, max_age, score_thresh=None, device=None, hungarian=False):
        if hungarian:
            raise NotImplementedError("Tracker: hungarian=True: the reference's branch calls linear_assignment, which it never defines")
        if not 1 <= segments <= MAX_SEGMENTS:
            raise _lib.S2DError(f"{segments} segments: 1..{MAX_SEGMENTS}")
        if max_age < 0:
            raise ValueError("max_age >= 0 expected")
        self.segments, self.max_age = int(segments), int(max_age)
        self.score_thresh = None if score_thresh is None else float(score_thresh)
        self.class_table = [(int(c), float(d)) for c, d in class_table]
        cls_of, diff_of = _table_arrays(self.class_table)
        device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.on_device = device.type == "cuda" and os.environ.get("S2D_TRACK_DEVICE") != "0"
        self._stamp = np.zeros(self.segments, np.float64)
        self._started = np.zeros(self.segments, np.bool_)
        self._history = [[] for _ in range(self.segments)]   # row counts of the last max_age + 1 frames: the bound on the tracks
        if self.on_device:
            table = np.zeros((len(cls_of), 2), np.int32)
            table[:, 0], table[:, 1] = cls_of, diff_of.view(np.int32)
            self._table = torch.from_numpy(table).to(device)
            z = lambda *shape, dtype: torch.zeros((2, self.segments) + shape, dtype=dtype, device=device)
            self._ct, self._tracking = z(MAX_TRACKS, 2, dtype=torch.float64), z(MAX_TRACKS, 2, dtype=torch.float64)
            self._meta, self._head = z(MAX_TRACKS, 4, dtype=torch.int32), z(2, dtype=torch.int32)
            self._cur = 0
        else:
            self._host = new_state(self.segments)

    @classmethod
    def waymo(cls, max_dist, max_age=3, score_thresh=0.75, segments=1, device=None):
        """labels 0 VEHICLE, 1 PEDESTRIAN, 2 CYCLIST; max_dist: name -> metres (the reference's --vehicle / --pedestrian / --cyclist)"""
        return cls(segments, class_table_of(WAYMO_TRACKING_NAMES, WAYMO_TRACKING_NAMES, max_dist), max_age, score_thresh, device)

    @classmethod
    def nuscenes(cls, max_age=3, segments=1, device=None, hungarian=False):
        """labels in the class order of waymo_configs.NUSC_TASKS; seven of the ten classes are tracked, with NUSCENE_CLS_VELOCITY_ERROR"""
        from .waymo_configs import NUSC_TASKS
        names = [n for t in NUSC_TASKS for n in t["class_names"]]
        return cls(segments, class_table_of(names, NUSCENES_TRACKING_NAMES, NUSCENE_CLS_VELOCITY_ERROR), max_age, None, device, hungarian)

    # -- inputs
    def _pack(self, dets):
        if isinstance(dets, tuple):
            if len(dets) != 4:
                raise TypeError("dets: the per-sample dictionaries of predict, or (boxes, labels, scores, offsets)")
            boxes, labels, scores, offsets = dets
            _check_boxes(boxes.shape)
            return boxes, labels, scores, _offsets(offsets, self.segments, boxes.shape[0])
        if len(dets) != self.segments:
            raise ValueError(f"{len(dets)} samples for {self.segments} segments")
        for d in dets:
            _check_boxes(d["box3d_lidar"].shape)
        offsets = np.cumsum([0] + [int(d["box3d_lidar"].shape[0]) for d in dets])
        cat = lambda k: dets[0][k] if len(dets) == 1 else torch.cat([d[k] for d in dets], 0)
        return cat("box3d_lidar"), cat("label_preds"), cat("scores"), _offsets(offsets, self.segments, int(offsets[-1]))

    def _bound(self, counts, first, skip):
        """refuses a step after which a segment could hold more than MAX_TRACKS tracks, from row counts alone"""
        history = [list(h) for h in self._history]
        for s in range(self.segments):
            if skip[s]:
                continue
            if first[s] or counts[s] == 0:   # reset, or an empty frame: the tracks are cleared
                history[s] = []
            history[s] = (history[s] + [int(counts[s])])[-(self.max_age + 1):]
            if sum(history[s]) > MAX_TRACKS:
                raise _lib.S2DError(f"segment {s}: up to {sum(history[s])} tracks (the rows of its last {len(history[s])} frames): at most "
                                    f"{MAX_TRACKS} per segment")
        return history

    def step(self, dets, poses, stamps, first=None, skip=None):
        """dets: the list of per-sample dictionaries `predict` returns (one per segment), or (boxes [R, 9], labels [R], scores [R],
        offsets [S + 1] on the host).  poses [S, 4, 4] float64 lidar-to-global, stamps [S] in seconds, first / skip [S] (first defaults to
        "the segment has not been stepped yet").  Returns (tracking_id [R], active [R], offsets [S + 1]) int32 on the inputs' device:
        tracking_id -1 for rows that are filtered or dropped.  No host read on the device path."""
        boxes, labels, scores, offsets = self._pack(dets)
        poses = _poses(poses, self.segments)
        stamps = np.asarray(stamps, np.float64).reshape(-1)
        if stamps.shape[0] != self.segments:
            raise ValueError(f"{stamps.shape[0]} timestamps for {self.segments} segments")
        skip = _flags(skip, self.segments, False)
        first = _flags(first, self.segments, False) if first is not None else ~self._started & ~skip
        if np.any(~first & ~skip & ~self._started):
            raise ValueError("a segment's first step must have first=True (the reference's reset())")
        history = self._bound(np.diff(offsets), first, skip)
        lag = np.where(first, 0.0, stamps - self._stamp)
        if self.on_device and torch.is_tensor(boxes) and boxes.is_cuda:
            out = self._step_device(boxes, labels, scores, offsets, poses, lag, first, skip)
        else:
            out = self._step_host(boxes, labels, scores, offsets, poses, lag, first, skip)
        self._history = history
        self._stamp = np.where(skip, self._stamp, stamps)
        self._started |= ~skip
        return out

    def _step_host(self, boxes, labels, scores, offsets, poses, lag, first, skip):
        if self.on_device:
            raise _lib.S2DError("Tracker: this tracker's state is on the device: CUDA detections expected (S2D_TRACK_DEVICE=0 or "
                                "device='cpu' selects the host path)")
        tid, act = step_host(self._host, boxes, labels, scores, offsets, poses, lag, first, skip, self.class_table, self.max_age,
                             self.score_thresh)
        dev = boxes.device if torch.is_tensor(boxes) else torch.device("cpu")
        return torch.from_numpy(tid).to(dev), torch.from_numpy(act).to(dev), torch.from_numpy(offsets.astype(np.int32)).to(dev)

    def _step_device(self, boxes, labels, scores, offsets, poses, lag, first, skip):
        dev, s, rows = self.device, self.segments, int(boxes.shape[0])
        same = lambda t, dtype: t if t.dtype == dtype and t.is_contiguous() and t.device == dev else t.to(dev, dtype).contiguous()
        boxes, labels, scores = same(boxes, torch.float32), same(labels, torch.int64), same(scores, torch.float32)
        if labels.shape[0] != rows or scores.shape[0] != rows:
            raise ValueError("boxes, labels and scores must have one row per detection")
        table = np.zeros(s, _SEGMENT)
        table["pose"], table["time_lag"], table["first"], table["skip"] = poses.reshape(s, 12), lag, first, skip
        table["row_lo"], table["row_hi"] = offsets[:-1], offsets[1:]
        upload = np.concatenate([table.view(np.uint8).reshape(-1), offsets.astype(np.int32).view(np.uint8)])
        upload = torch.from_numpy(upload).to(dev)   # the step's one upload: the segment table, then the row offsets
        tid = torch.empty(rows, dtype=torch.int32, device=dev)
        act = torch.empty(rows, dtype=torch.int32, device=dev)
        old, new = self._cur, 1 - self._cur
        ptr = lambda t: t.data_ptr() if t.numel() else None
        _lib.check(_lib.load().s2d_track_step(ptr(boxes), ptr(labels), ptr(scores), rows, s, upload.data_ptr(), self._table.data_ptr(),
                                              self._table.shape[0], self.max_age, -1.0 if self.score_thresh is None else self.score_thresh,
                                              self._ct[old].data_ptr(), self._tracking[old].data_ptr(), self._meta[old].data_ptr(),
                                              self._head[old].data_ptr(), self._ct[new].data_ptr(), self._tracking[new].data_ptr(),
                                              self._meta[new].data_ptr(), self._head[new].data_ptr(), ptr(tid), ptr(act), _stream(dev)),
                   "s2d_track_step")
        self._cur = new
        return tid, act, upload[s * _SEGMENT.itemsize:].view(torch.int32)

    # -- results
    def buffers(self):
        """the current state buffers (ct, tracking, meta, head), [S, ...] each: device tensors or numpy arrays"""
        if self.on_device:
            return self._ct[self._cur], self._tracking[self._cur], self._meta[self._cur], self._head[self._cur]
        return self._host["ct"], self._host["tracking"], self._host["meta"], self._host["head"]

    def state(self, segment):
        """one segment's track list on the host (a copy; for tests and for writing results): ids, classes, ages, active, ct, tracking,
        id_count"""
        ct, tracking, meta, head = self.buffers()
        if self.on_device:
            count, id_count = head[segment].tolist()
            ct, tracking, meta = ct[segment, :count].cpu().numpy(), tracking[segment, :count].cpu().numpy(), meta[segment, :count].cpu().numpy()
        else:
            count, id_count = (int(v) for v in head[segment])
            ct, tracking, meta = ct[segment, :count].copy(), tracking[segment, :count].copy(), meta[segment, :count].copy()
        return dict(ids=meta[:, 1], classes=meta[:, 0], ages=meta[:, 2], active=meta[:, 3], ct=ct, tracking=tracking, id_count=id_count)


# ---- the static device tracker: padded rows, device counts, device parity; one launch, capturable ---------------------------------------
def pack_padded(boxes, labels, scores, counts):
    """padded rows (boxes [S, cap, 9], labels [S, cap], scores [S, cap], counts [S]) as the packed rows of `step_host`:
    (boxes [R, 9], labels [R], scores [R], offsets [S + 1]) with the first clamp(counts[s], 0, cap) rows of every segment.  numpy only:
    the host definition of the static step is step_host on these rows."""
    boxes, labels, scores = _np(boxes, np.float32), _np(labels, np.int64), _np(scores, np.float32)
    if boxes.ndim != 3:
        raise ValueError(f"boxes {boxes.shape}: [S, cap, 9] expected")
    _check_boxes(boxes.shape[1:])
    segments, cap = boxes.shape[:2]
    counts = np.clip(_np(counts, np.int64).reshape(-1), 0, cap)
    if labels.shape != (segments, cap) or scores.shape != (segments, cap) or counts.shape[0] != segments:
        raise ValueError("labels and scores [S, cap] and counts [S] expected beside boxes [S, cap, 9]")
    keep = np.arange(cap)[None, :] < counts[:, None]
    return boxes[keep], labels[keep], scores[keep], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


class StaticTracks:
    """Padded results of `StaticTracker.run`, on the device and owned by the tracker (the next run overwrites them): tracking_id, active
    int32 [S, cap]; -1 / 0 for filtered rows, for the rows at or behind the sample's count and for every row of a skipped sample."""
    __slots__ = ("tracking_id", "active")

    def __init__(self, tracking_id, active):
        self.tracking_id, self.active = tracking_id, active

    def __iter__(self):
        return iter((self.tracking_id, self.active))

    def as_list(self, det, metadata=None):
        """`predict`'s dictionaries (box3d_lidar, scores, label_preds, metadata) of the detections `det` (a StaticDetections, or (boxes,
        labels, scores, counts)) with tracking_id and active per sample: views into the padded buffers.  The ONE host read: the counts."""
        boxes, labels, scores, counts = _static_inputs(det)
        return [dict(box3d_lidar=boxes[b, :n], scores=scores[b, :n], label_preds=labels[b, :n], metadata=metadata[b] if metadata else None,
                     tracking_id=self.tracking_id[b, :n], active=self.active[b, :n]) for b, n in enumerate(counts.tolist())]


def _static_inputs(det):
    if isinstance(det, tuple):
        if len(det) != 4:
            raise TypeError("det: a StaticDetections, or (boxes, labels, scores, counts)")
        return det
    return det.boxes, det.labels, det.scores, det.counts


class StaticTracker:
    """`samples` sequences tracked side by side on the padded, device-resident results of `CenterHead.predict_static` (StaticDetections):
    boxes [samples, cap, 9], labels, scores [samples, cap] and counts [samples] are read where they lie.  Every buffer is allocated here,
    once; `run` is one launch of s2d_track_step_static on the current stream with no host read, no allocation and no torch operator, and
    the parity of the doubled state is kept on the device, so `run` can be captured into a HIP graph (alone, or behind
    StaticPredictPlan.run) and replayed: each replay is the next step.  `set_frames` puts the poses, stamps and flags of the next run into
    the frame block with one host-to-device copy, outside the capture.  The association is `Tracker`'s: the same device code.
    cap * (max_age + 1) <= 4096 is the static form of Tracker's bound on a segment's tracks."""

    def __init__(self, samples, cap, class_table, max_age, score_thresh=None, device=None, hungarian=False):
        if hungarian:
            raise NotImplementedError("StaticTracker: hungarian=True: the reference's branch calls linear_assignment, which it never defines")
        if not 1 <= samples <= MAX_SEGMENTS:
            raise _lib.S2DError(f"StaticTracker: {samples} samples: 1..{MAX_SEGMENTS}")
        if not 1 <= cap <= MAX_DETS:
            raise _lib.S2DError(f"StaticTracker: cap {cap}: 1..{MAX_DETS} rows per sample")
        if max_age < 0:
            raise ValueError("max_age >= 0 expected")
        if cap * (max_age + 1) > MAX_TRACKS:
            raise _lib.S2DError(f"StaticTracker: cap {cap} x (max_age {max_age} + 1) = {cap * (max_age + 1)} tracks: at most {MAX_TRACKS} per sample")
        self.samples, self.cap, self.max_age = int(samples), int(cap), int(max_age)
        self.score_thresh = None if score_thresh is None else float(score_thresh)
        self.class_table = [(int(c), float(d)) for c, d in class_table]
        cls_of, diff_of = _table_arrays(self.class_table)
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda":
            raise _lib.S2DError("StaticTracker: a CUDA device expected (no CPU fallback; Tracker has the host path)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        _lib.load()
        table = np.zeros((len(cls_of), 2), np.int32)
        table[:, 0], table[:, 1] = cls_of, diff_of.view(np.int32)
        self._table = torch.from_numpy(table).to(device)
        z = lambda *shape, dtype: torch.zeros(shape, dtype=dtype, device=device)
        s = self.samples
        self._ct, self._tracking = z(2, s, MAX_TRACKS, 2, dtype=torch.float64), z(2, s, MAX_TRACKS, 2, dtype=torch.float64)
        self._meta, self._head = z(2, s, MAX_TRACKS, 4, dtype=torch.int32), z(2, s, 2, dtype=torch.int32)
        self._parity, self._prev_stamp = z(s, dtype=torch.int32), z(s, dtype=torch.float64)
        self.frames = z(s, _FRAME.itemsize, dtype=torch.uint8)   # s2d_track_frame [samples]; set_frames fills it, or the caller does
        self.out = StaticTracks(z(s, self.cap, dtype=torch.int32), z(s, self.cap, dtype=torch.int32))
        self.out.tracking_id.fill_(-1)
        self._started = np.zeros(s, np.bool_)

    @classmethod
    def waymo(cls, max_dist, cap, max_age=3, score_thresh=0.75, samples=1, device=None):
        """labels 0 VEHICLE, 1 PEDESTRIAN, 2 CYCLIST; max_dist: name -> metres (as Tracker.waymo)"""
        return cls(samples, cap, class_table_of(WAYMO_TRACKING_NAMES, WAYMO_TRACKING_NAMES, max_dist), max_age, score_thresh, device)

    @classmethod
    def nuscenes(cls, cap, max_age=3, samples=1, device=None, hungarian=False):
        """labels in the class order of waymo_configs.NUSC_TASKS (as Tracker.nuscenes)"""
        from .waymo_configs import NUSC_TASKS
        names = [n for t in NUSC_TASKS for n in t["class_names"]]
        return cls(samples, cap, class_table_of(names, NUSCENES_TRACKING_NAMES, NUSCENE_CLS_VELOCITY_ERROR), max_age, None, device, hungarian)

    def set_frames(self, poses, stamps, first=None, skip=None):
        """the frame block of the NEXT run, from host values: poses [S, 4, 4] float64 lidar-to-global, stamps [S] in seconds, first / skip
        [S] (first defaults to "the sample has not been stepped yet").  One host-to-device copy on the current stream; call it once per
        run, outside any capture."""
        s = self.samples
        poses = _poses(poses, s)
        stamps = np.asarray(stamps, np.float64).reshape(-1)
        if stamps.shape[0] != s:
            raise ValueError(f"{stamps.shape[0]} timestamps for {s} samples")
        skip = _flags(skip, s, False)
        first = _flags(first, s, False) if first is not None else ~self._started & ~skip
        if np.any(~first & ~skip & ~self._started):
            raise ValueError("a sample's first step must have first=True (the reference's reset())")
        block = np.zeros(s, _FRAME)
        block["pose"], block["stamp"], block["first"], block["skip"] = poses.reshape(s, 12), stamps, first, skip
        self.frames.copy_(torch.from_numpy(block.view(np.uint8).reshape(s, _FRAME.itemsize)))   # the step's one upload
        self._started |= ~skip

    def _check(self, det):
        boxes, labels, scores, counts = _static_inputs(det)
        if boxes.dim() != 3:
            raise ValueError(f"boxes {tuple(boxes.shape)}: [{self.samples}, {self.cap}, 9] expected")
        _check_boxes(boxes.shape[1:])
        if tuple(boxes.shape) != (self.samples, self.cap, 9):
            raise _lib.S2DError(f"StaticTracker.run: boxes {tuple(boxes.shape)}, the tracker was built for {(self.samples, self.cap, 9)} "
                                "(samples, cap of the plan, 9)")
        for name, t, dtype, shape in (("boxes", boxes, torch.float32, boxes.shape), ("labels", labels, torch.int64, (self.samples, self.cap)),
                                      ("scores", scores, torch.float32, (self.samples, self.cap)), ("counts", counts, torch.int32, (self.samples,))):
            if t.device != self.device or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
                raise _lib.S2DError(f"StaticTracker.run: {name} is {t.dtype} {tuple(t.shape)} on {t.device}"
                                    f"{'' if t.is_contiguous() else ', not contiguous'}: contiguous {dtype} {tuple(shape)} on {self.device} expected "
                                    "(the static step neither copies nor converts)")
        return boxes, labels, scores, counts

    def run(self, det):
        """det: the StaticDetections of a plan with this tracker's samples and cap, or (boxes, labels, scores, counts) device tensors.
        One launch on the current stream; returns the tracker's `StaticTracks` (the same tensors at every call)."""
        boxes, labels, scores, counts = self._check(det)   # host only
        ptr = lambda t: t.data_ptr()
        _lib.check(_lib.load().s2d_track_step_static(ptr(boxes), ptr(labels), ptr(scores), ptr(counts), self.samples, self.cap, ptr(self.frames),
                                                     ptr(self._table), self._table.shape[0], self.max_age,
                                                     -1.0 if self.score_thresh is None else self.score_thresh, ptr(self._ct), ptr(self._tracking),
                                                     ptr(self._meta), ptr(self._head), ptr(self._parity), ptr(self._prev_stamp),
                                                     ptr(self.out.tracking_id), ptr(self.out.active), _stream(self.device)), "s2d_track_step_static")
        return self.out

    # -- results
    def all_buffers(self):
        """every device buffer of the tracker by name (none is ever reallocated)"""
        return dict(table=self._table, ct=self._ct, tracking=self._tracking, meta=self._meta, head=self._head, parity=self._parity,
                    prev_stamp=self._prev_stamp, frames=self.frames, tracking_id=self.out.tracking_id, active=self.out.active)

    def buffers(self):
        """the current state (ct, tracking, meta, head), [S, ...] each, as on Tracker: every sample's current half (the one its parity
        names) gathered into new tensors.  Torch operators and allocations: for tests and result writers, not for the step."""
        at = (self._parity.to(torch.int64), torch.arange(self.samples, device=self.device))
        return self._ct[at], self._tracking[at], self._meta[at], self._head[at]

    def state(self, segment):
        """one sample's track list on the host, as Tracker.state (a copy; for tests and for writing results)"""
        half = int(self._parity[segment].item())
        count, id_count = self._head[half, segment].tolist()
        ct, tracking = self._ct[half, segment, :count].cpu().numpy(), self._tracking[half, segment, :count].cpu().numpy()
        meta = self._meta[half, segment, :count].cpu().numpy()
        return dict(ids=meta[:, 1], classes=meta[:, 0], ages=meta[:, 2], active=meta[:, 3], ct=ct, tracking=tracking, id_count=id_count)


# ---- the reference's class -----------------------------------------------------------------------------------------------------------
class PubTracker:
    """The reference's PubTracker on lists of dictionaries, with either of its constructor signatures:

        PubTracker(hungarian=False, max_age=0)                    tools/nusc_tracking/pub_tracker.py (NUSCENE_CLS_VELOCITY_ERROR)
        PubTracker(max_age=0, max_dist={}, score_thresh=0.1)      tools/waymo_tracking/tracker.py

    The Waymo form is taken when max_dist or score_thresh is given (or a second positional argument is a dictionary).
    step_centertrack(results, time_lag) reads translation, velocity, detection_name (and score) of every dictionary, writes ct, tracking,
    label_preds, tracking_id, age and active into the kept ones as the reference does, and returns the new track list, which `tracks`
    holds; `id_count` and `reset()` as in the reference."""

    def __init__(self, *args, **kwargs):
        waymo = "max_dist" in kwargs or "score_thresh" in kwargs or (len(args) >= 2 and isinstance(args[1], dict))
        if waymo:
            names = ("max_age", "max_dist", "score_thresh")
            given = dict(zip(names, args), **kwargs)
            self.max_age, self.score_thresh = given.get("max_age", 0), given.get("score_thresh", 0.1)
            self.names, self.max_dist, self.hungarian = WAYMO_TRACKING_NAMES, given.get("max_dist", {}), False
        else:
            given = dict(zip(("hungarian", "max_age"), args), **kwargs)
            self.hungarian, self.max_age, self.score_thresh = given.get("hungarian", False), given.get("max_age", 0), None
            self.names, self.max_dist = NUSCENES_TRACKING_NAMES, NUSCENE_CLS_VELOCITY_ERROR
        if set(given) - {"hungarian", "max_age", "max_dist", "score_thresh"} or len(args) > 3:
            raise TypeError(f"PubTracker: unexpected arguments {args} {kwargs}")
        if self.hungarian:
            raise NotImplementedError("PubTracker: hungarian=True: the reference's branch calls linear_assignment, which it never defines")
        self.reset()

    def reset(self):
        self.id_count = 0
        self.tracks = []

    def step_centertrack(self, results, time_lag):
        if len(results) == 0:
            self.tracks = []
            return []
        kept = [det for det in results if det["detection_name"] in self.names]
        for det in kept:
            det["ct"] = np.array(det["translation"][:2])
            det["tracking"] = np.array(det["velocity"][:2]) * -1 * time_lag
            det["label_preds"] = self.names.index(det["detection_name"])
        as2d = lambda rows: np.array(rows, np.float64).reshape(-1, 2)
        old = dict(ct=as2d([t["ct"] for t in self.tracks]), tracking=as2d([t["tracking"] for t in self.tracks]),
                   meta=np.array([[t["label_preds"], t["tracking_id"], t["age"], t["active"]] for t in self.tracks], np.int32).reshape(-1, 4),
                   id_count=self.id_count)
        score = np.array([det.get("score", 0.0) for det in kept], np.float32)
        new, self.id_count, _, _, sources = _associate(
            old, as2d([det["ct"] for det in kept]), as2d([det["tracking"] for det in kept]),
            np.array([det["label_preds"] for det in kept], np.int32), np.array([self.max_dist[det["detection_name"]] for det in kept], np.float32),
            score, self.max_age, self.score_thresh)
        ret = []
        for k, (kind, i) in enumerate(sources):
            track = kept[i] if kind == "det" else self.tracks[i]
            track["tracking_id"], track["age"], track["active"] = int(new["meta"][k, 1]), int(new["meta"][k, 2]), int(new["meta"][k, 3])
            if kind == "trk":
                track["ct"] = new["ct"][k]
            ret.append(track)
        self.tracks = ret
        return ret
