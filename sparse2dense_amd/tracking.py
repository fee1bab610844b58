"""Center-based multi-object tracking: the reference's `PubTracker.step_centertrack` (tools/nusc_tracking/pub_tracker.py:49-154,
tools/waymo_tracking/tracker.py:42-136) behind `transform_box` (tools/waymo_tracking/test.py:160-183), over csrc/tracking.hip.

    Tracker           up to 64 sequences (segments) stepped together in ONE launch; the track lists stay on the device
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
JSON / Waymo .bin writers and the metric programs, HIP-graph capture of the step."""
import os

import numpy as np
import torch

from . import _lib

MAX_SEGMENTS, MAX_DETS, MAX_TRACKS = 64, 1024, 4096   # S2D_TRACK_MAX_SEGMENTS / _DETS / _TRACKS
STEP_LAUNCHES, STEP_HOST_READS, STEP_UPLOADS = 1, 0, 1

NUSCENES_TRACKING_NAMES = ["bicycle", "bus", "car", "motorcycle", "pedestrian", "trailer", "truck"]
NUSCENE_CLS_VELOCITY_ERROR = {"car": 4, "truck": 4, "bus": 5.5, "trailer": 3, "pedestrian": 1, "motorcycle": 13, "bicycle": 3}
WAYMO_TRACKING_NAMES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]

_SEGMENT = np.dtype([("pose", np.float64, (12,)), ("time_lag", np.float64), ("first", np.int32), ("skip", np.int32), ("row_lo", np.int32),
                     ("row_hi", np.int32)])   # s2d_track_segment
assert _SEGMENT.itemsize == 120


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
