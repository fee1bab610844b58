#!/usr/bin/env python
"""Maps -> detections -> track ids, three routes alternating in one process on the same maps:

    (a) head.predict + Tracker.step on its dictionaries            the route without the static classes: the yardstick
    (b) StaticPredictPlan.run + StaticTracker.run, eager           launches only, one upload (the frame block)
    (c) one torch.cuda.graph holding both, replayed                the same launches from one graph

    python tools/static_track_bench.py [--runs 20] [--warmup 5] [--out profiles/static_track_bench.txt]

Inputs: the maps of tools/center_predict_bench.py with a velocity branch (nuScenes, six tasks, 180 x 180, rotated NMS), B = 1 (online)
and B = 4.  Every route owns a tracker; a round steps all three once on the same maps, poses and stamps (0.5 s apart), so the three track
lists stay in step and the ids and active counts of every round are asserted equal.  HIP events around the call and the host's wall time
of it, median (min) of `runs` rounds after `warmup`; launches, device-to-host copies and blocking runtime calls of one extra round from a
profiler trace.  No time is fixed in advance: the rows stand next to route (a)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_predict_bench import NUSC, SIX, U, counts_of, head_of  # noqa: E402
from prep_bench import med, timed  # noqa: E402
from sparse2dense_amd import center_predict, tracking as T  # noqa: E402

SIZE, MAX_AGE = 180, 3


class Routes:
    def __init__(self, samples, peaks, dev):
        self.samples, self.cfg = samples, dict(NUSC)
        self.maps = [{k: v.cuda() for k, v in U.seeded_task_maps(c, 7000 + i, SIZE, SIZE, samples, False, vel=True, peaks=peaks).items()}
                     for i, c in enumerate(SIX)]
        self.head = head_of(SIX, True)
        self.plan = center_predict.StaticPredictPlan(self.cfg, self.head.num_classes, samples, SIZE, SIZE, True, dev)
        self.tracker = T.Tracker.nuscenes(MAX_AGE, segments=samples, device=dev)
        self.eager = T.StaticTracker.nuscenes(self.plan.cap, MAX_AGE, samples=samples, device=dev)
        self.graphed = T.StaticTracker.nuscenes(self.plan.cap, MAX_AGE, samples=samples, device=dev)
        self.poses = np.stack([np.eye(4)] * samples)
        self.poses[:, :2, 3] = [[100.0 + 10.0 * s, -50.0] for s in range(samples)]
        self.stamp = 0.0
        # capture: warm up on a side stream with every sample skipped (nothing is stepped), then record predict + track once
        self.graphed.set_frames(self.poses, [0.0] * samples, skip=[True] * samples)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self.graphed.run(self.plan.run(self.maps))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.graphed.run(self.plan.run(self.maps))

    def stamps(self):
        return [self.stamp + 7.0 * s for s in range(self.samples)]

    def route_a(self):
        return self.tracker.step(self.head.predict({}, self.maps, self.cfg), self.poses, self.stamps())

    def route_b(self):
        self.eager.set_frames(self.poses, self.stamps())
        return self.eager.run(self.plan.run(self.maps))

    def route_c(self):
        self.graphed.set_frames(self.poses, self.stamps())
        self.graph.replay()
        return self.graphed.out

    def check(self, a, b, c):
        """the ids and active counts of the three routes, on the rows below the counts (the padding is -1 / 0)"""
        tid, act, off = a
        off, counts = off.tolist(), self.plan.out.counts.tolist()
        assert counts == [off[s + 1] - off[s] for s in range(self.samples)], "predict and predict_static disagree on the counts"
        for out, name in ((b, "eager"), (c, "graph")):
            for s, n in enumerate(counts):
                ok = torch.equal(out.tracking_id[s, :n], tid[off[s]:off[s + 1]]) and torch.equal(out.active[s, :n], act[off[s]:off[s + 1]])
                assert ok and bool((out.tracking_id[s, n:] == -1).all()), f"route {name} and Tracker.step disagree (sample {s})"
        return sum(counts), int((act >= 2).sum())


def measure(r, runs, warmup):
    paths = [("(a) predict + Tracker.step", r.route_a), ("(b) plan.run + StaticTracker.run", r.route_b), ("(c) one graph replay", r.route_c)]
    ev, wall = {n: [] for n, _ in paths}, {n: [] for n, _ in paths}
    rows = matched = 0
    for k in range(warmup + runs):   # the routes alternate: every round steps all three trackers once
        r.stamp += 0.5
        outs = []
        for name, fn in paths:
            e, w, out = timed(fn)
            outs.append(out)
            if k >= warmup:
                ev[name].append(e)
                wall[name].append(w)
        rows, matched = r.check(*outs)
    r.stamp += 0.5
    lines = []
    for name, fn in paths:   # one extra round under the profiler
        try:
            kernels, d2h, blocking = counts_of(fn)
            cnt = f"{kernels} launches, {d2h} device-to-host copies, blocking calls {dict(blocking) or 'none'}"
        except Exception as exc:   # the counts are a side figure: the timing stands without them
            cnt = f"launch count not taken ({type(exc).__name__})"
        lines.append(f"  {name:34s} events {med(ev[name])}   host wall {med(wall[name])}   {cnt}")
    return lines, rows, matched, int(max(r.tracker.buffers()[3][:, 0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--peaks", type=int, default=400, help="heat-map peaks per (task, sample); about three quarters pass the threshold")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_track_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("static_track_bench: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    lines = [f"# maps -> detections -> track ids (nuScenes 6 tasks with velocity, {SIZE}x{SIZE}, rotated NMS, {args.peaks} peaks per segment, max_age "
             f"{MAX_AGE}): three routes alternating on the same maps, one tracker each, ids and active counts asserted equal every round; median (min) "
             f"of {args.runs} rounds after {args.warmup} warm-ups, HIP events around the call and the host's wall time of it; device "
             f"{torch.cuda.get_device_name(0)}",
             f"# stated plan of the static step: {T.STATIC_STEP_LAUNCHES} launch, {T.STATIC_STEP_UPLOADS} upload (the frame block, set_frames), "
             f"{T.STATIC_STEP_HOST_READS} host reads; counted below from a profiler trace of one extra round.  Route (a) is the yardstick"]
    for samples, title in ((1, "online"), (4, "B = 4")):
        r = Routes(samples, args.peaks, dev)
        body, rows, matched, tracks = measure(r, args.runs, args.warmup)
        lines.append(f"{title}: {samples} sample(s), cap {r.plan.cap}, {rows} boxes in the last round, {matched} of them matched, up to {tracks} tracks")
        lines += body
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
