#!/usr/bin/env python
"""One tracker step on the device (tracking.Tracker over csrc/tracking.hip) beside the two host routes, from the same track state on the
same detections, alternating in one process.

    python tools/tracking_bench.py [--runs 20] [--warmup 5] [--out profiles/tracking_bench.txt]

Rows: online (1 segment, about 300 boxes over about 600 tracks), offline (64 segments of that size in one launch), worst case (1024 boxes
of one class over the 3072 tracks that three frames of 1024 rows leave with max_age 3; the boxes and the 1024 tracks of the first frame
are packed inside one gate, so that most detections find their first choice taken and scan all 3072 tracks again; 4096 tracks cannot be
followed by a frame of 1024 rows: the host bound refuses it).
Paths: the device step; "copy the boxes to the host + step_host + ids back to the device" (a Tracker with device="cpu" on the same CUDA
tensors); the dictionary API (one PubTracker per segment on dictionaries built from the host copies, the boxes moved to the global frame
by numpy).  Before every measured call the trackers are put back to the same state (not timed).  HIP events around the call and the
host's wall time of it, median (min) of `runs` after `warmup`; launches and blocking copies from a profiler trace of one extra call.
The outputs of the three paths are asserted equal (tracking ids and active counts of every row)."""
import argparse
import copy
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_predict_bench import counts_of  # noqa: E402
from prep_bench import med, timed  # noqa: E402
from sparse2dense_amd import tracking as T  # noqa: E402

GRID = 1.0 / 64
NAMES = ["VEHICLE", "PEDESTRIAN", "CYCLIST"]
snap = lambda a: np.round(np.asarray(a, np.float64) / GRID) * GRID


def scene_frames(seed, rows, pool, frames, field, max_dist, apart=0.0):
    """frames of one segment: `rows` of `pool` constant-velocity objects a frame on a square of `field` m (grid coordinates, exact poses);
    with `apart` every frame but the last is moved `apart` m further along x (its tracks match nothing), the last one lies on frame 0"""
    rng = np.random.RandomState(seed)
    xy, vel = snap(rng.uniform(0, field, (pool, 2))), snap(rng.uniform(-0.5, 0.5, (pool, 2)))
    labels = rng.randint(0, len(max_dist), pool)
    out = []
    for f in range(frames):
        pick = rng.permutation(pool)[:rows]
        pose = np.eye(4)
        pose[:3, 3] = snap(rng.uniform(-500, 500, 3))
        boxes = np.zeros((rows, 9), np.float32)
        boxes[:, :2] = xy[pick] + vel[pick] * 0.5 * f + snap(rng.uniform(-0.1, 0.1, (rows, 2))) - pose[:2, 3]
        boxes[:, 0] += apart * (f if f < frames - 1 else 0)
        boxes[:, 3:6], boxes[:, 6:8] = 1.0, vel[pick]
        out.append(dict(boxes=boxes, labels=labels[pick].astype(np.int64), scores=rng.uniform(0.3, 1.0, rows).astype(np.float32), pose=pose,
                        stamp=0.5 * f))
    return out


def pack(frames):
    off = np.cumsum([0] + [len(f["boxes"]) for f in frames])
    cat = lambda k: np.concatenate([f[k] for f in frames], 0)
    return cat("boxes"), cat("labels"), cat("scores"), off, np.stack([f["pose"] for f in frames]), np.array([f["stamp"] for f in frames])


class Row:
    """the three trackers of one row, driven to the state in front of the measured step"""

    def __init__(self, segments, rows, pool, frames, field, max_dist, max_age, thresh, dev, apart=0.0):
        self.segments, self.max_dist = segments, max_dist
        table = T.class_table_of(NAMES[:len(max_dist)], NAMES[:len(max_dist)], dict(zip(NAMES, max_dist)))
        seqs = [scene_frames(100 + s, rows, pool, frames, field, max_dist, apart) for s in range(segments)]
        self.device, self.host = T.Tracker(segments, table, max_age, thresh, device=dev), T.Tracker(segments, table, max_age, thresh, device="cpu")
        kw = dict(max_age=max_age, max_dist=dict(zip(NAMES, max_dist)), score_thresh=thresh if thresh is not None else -1.0)
        self.pubs = [T.PubTracker(**kw) for _ in range(segments)]
        for k in range(frames - 1):
            boxes, labels, scores, off, poses, stamps = pack([q[k] for q in seqs])
            for trk in (self.device, self.host):
                trk.step((torch.from_numpy(boxes).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(scores).to(dev), off), poses, stamps)
            self._pub_step(boxes, labels, scores, off, poses, [0.0 if k == 0 else 0.5] * segments)
        boxes, labels, scores, self.off, self.poses, self.stamps = pack([q[-1] for q in seqs])
        self.dets = (torch.from_numpy(boxes).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(scores).to(dev), self.off)
        self.tracks = int(self.host.buffers()[3][:, 0].max())
        self.saved = (self._snapshot(self.device), self._snapshot(self.host), copy.deepcopy([(p.tracks, p.id_count) for p in self.pubs]))

    @staticmethod
    def _snapshot(trk):
        keep = {k: copy.deepcopy(getattr(trk, k)) for k in ("_stamp", "_started", "_history")}
        if trk.on_device:
            keep.update(_cur=trk._cur, bufs=[t.clone() for t in (trk._ct, trk._tracking, trk._meta, trk._head)])
        else:
            keep["_host"] = copy.deepcopy(trk._host)
        return keep

    @staticmethod
    def _restore(trk, keep):
        for k in ("_stamp", "_started", "_history"):
            setattr(trk, k, copy.deepcopy(keep[k]))
        if trk.on_device:
            trk._cur = keep["_cur"]
            for t, b in zip((trk._ct, trk._tracking, trk._meta, trk._head), keep["bufs"]):
                t.copy_(b)
        else:
            trk._host = copy.deepcopy(keep["_host"])

    def restore(self):
        self._restore(self.device, self.saved[0])
        self._restore(self.host, self.saved[1])
        for p, (tracks, id_count) in zip(self.pubs, copy.deepcopy(self.saved[2])):
            p.tracks, p.id_count = tracks, id_count
        torch.cuda.synchronize()

    def _pub_step(self, boxes, labels, scores, off, poses, lags):
        tid, act = np.full(len(boxes), -1, np.int32), np.zeros(len(boxes), np.int32)
        for s, pub in enumerate(self.pubs):
            lo, hi = off[s], off[s + 1]
            b = boxes[lo:hi].astype(np.float64)
            centre = b[:, :3] @ poses[s][:3, :3].T + poses[s][:3, 3]
            vel = b[:, 6:8] @ poses[s][:2, :2].T
            annos = [dict(translation=centre[i], velocity=vel[i], detection_name=NAMES[labels[lo + i]], score=scores[lo + i], box_id=lo + i)
                     for i in range(hi - lo)]
            for o in pub.step_centertrack(annos, lags[s]):
                if o["active"] > 0:
                    tid[o["box_id"]], act[o["box_id"]] = o["tracking_id"], o["active"]
        return tid, act

    def run_device(self):
        return self.device.step(self.dets, self.poses, self.stamps)[:2]

    def run_host(self):
        return self.host.step(self.dets, self.poses, self.stamps)[:2]

    def run_pub(self):
        boxes, labels, scores = (t.cpu().numpy() for t in self.dets[:3])
        tid, act = self._pub_step(boxes, labels, scores, self.off, self.poses, [0.5] * self.segments)
        dev = self.dets[0].device
        return torch.from_numpy(tid).to(dev), torch.from_numpy(act).to(dev)


def measure(row, runs, warmup):
    paths = [("device step", row.run_device), ("copy to host + step_host + ids back", row.run_host), ("PubTracker.step_centertrack", row.run_pub)]
    ev, wall, outs = {n: [] for n, _ in paths}, {n: [] for n, _ in paths}, {}
    for k in range(warmup + runs):   # the paths alternate: every round runs all three from the same state
        for name, fn in paths:
            row.restore()
            e, w, out = timed(fn)
            if k >= warmup:
                ev[name].append(e)
                wall[name].append(w)
            outs[name] = out
    ref = outs[paths[0][0]]
    for name, _ in paths[1:]:
        assert torch.equal(ref[0], outs[name][0]) and torch.equal(ref[1], outs[name][1]), f"{name} and the device step disagree"
    lines = []
    for name, fn in paths:
        row.restore()
        try:
            kernels, d2h, blocking = counts_of(fn)
            cnt = f"{kernels} launches, {d2h} device-to-host copies, blocking calls {dict(blocking)}"
        except Exception as exc:   # the counts are a side figure: the timing stands without them
            cnt = f"launch count not taken ({type(exc).__name__})"
        lines.append(f"  {name:38s} events {med(ev[name])}   host wall {med(wall[name])}   {cnt}")
    before = row.saved[1]["_host"]["head"][:, 1][np.repeat(np.arange(row.segments), np.diff(row.off))]   # id_count in front of the step
    tid = ref[0].cpu().numpy()
    matched = int(((tid > 0) & (tid <= before)).sum())
    return lines, matched, statistics.median(ev[paths[0][0]]), statistics.median(ev[paths[1][0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tracking_bench: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = [f"# tracker step (tracking.Tracker, csrc/tracking.hip) beside the host routes from the same state on the same detections, alternating; "
             f"median (min) of {args.runs} calls after {args.warmup} warm-ups, HIP events around the call and the host's wall time of it; device "
             f"{torch.cuda.get_device_name(0)}",
             f"# stated plan: device step {T.STEP_LAUNCHES} launch, {T.STEP_UPLOADS} upload (segment table + row offsets), {T.STEP_HOST_READS} host reads; "
             f"counted below from a profiler trace; all three paths give the same ids and active counts (asserted)"]
    specs = [("online", dict(segments=1, rows=300, pool=600, frames=5, field=150.0, max_dist=[0.8, 0.4, 0.6], max_age=3, thresh=0.5)),
             ("offline", dict(segments=64, rows=300, pool=600, frames=5, field=150.0, max_dist=[0.8, 0.4, 0.6], max_age=3, thresh=0.5)),
             ("worst case", dict(segments=1, rows=1024, pool=4096, frames=4, field=8.0, max_dist=[16.0], max_age=3, thresh=None, apart=128.0))]
    for name, spec in specs:
        row = Row(dev=dev, **spec)
        body, matched, t_dev, t_host = measure(row, args.runs, args.warmup)
        verdict = "device not slower" if t_dev <= t_host else "DEVICE SLOWER than the copy-to-host route"
        lines.append(f"{name}: {spec['segments']} segment(s) x {spec['rows']} boxes over up to {row.tracks} tracks, {matched} rows matched - {verdict}")
        lines += body
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
