#!/usr/bin/env python
"""Head maps + neck map -> refined detections of the two-stage detector, three routes alternating in one process on the same inputs:

    (a) head.predict + TwoStageDetector._forward_device        the route without the static classes: the yardstick
    (b) StaticPredictPlan.run + StaticRoIPlan.run, eager       launches only, no host read, no copy
    (c) one torch.cuda.graph holding both, replayed            the same launches from one graph

    python tools/static_two_stage_bench.py [--runs 20] [--warmup 5] [--out profiles/static_two_stage_bench.txt]

Shape: that of tools/two_stage_bench.py - the Waymo head (one task, three classes, 188 x 188 maps, rotated NMS, 4096 candidates, 500
kept), B = 4, a 188 x 188 x 512 channels_last bf16 neck map, cap 500, num_point 5, the two-stage configuration's RoI head (2560 -> 256 ->
256 -> 2 x (256 -> 256 -> 1 | 7)).  The first stage in front of the head maps is not run.  HIP events around the call and the host's wall
time of it, median (min) of `runs` rounds after `warmup`; the boxes, scores and labels of the three routes are asserted bit-equal every
round; launches, device-to-host copy records and blocking runtime calls of one extra round from a profiler trace.  No time is fixed in
advance: the rows stand next to route (a)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_predict_bench import WAYMO, U, counts_of, head_of  # noqa: E402
from prep_bench import med, timed  # noqa: E402
from sparse2dense_amd import center_predict, registry, second_stage as S, waymo_configs  # noqa: E402

B, C, SIZE, CAP = 4, 512, 188, 500


class Routes:
    def __init__(self, peaks, dev):
        self.cfg = dict(WAYMO)
        self.maps = [{k: v.to(dev) for k, v in U.seeded_task_maps(3, 7000, SIZE, SIZE, B, False, vel=False, peaks=peaks).items()}]
        g = torch.Generator().manual_seed(1)
        self.bev = torch.randn(B, SIZE, SIZE, C, generator=g).to(torch.bfloat16).to(dev).permute(0, 3, 1, 2)   # channels_last, as the bf16 neck leaves it
        self.head = head_of([3], False)
        cfg = waymo_configs.two_stage_voxelnet()
        self.det = registry.build_detector(cfg).to(dev).eval()   # (the first stage is built but never run)
        assert self.det.NMS_POST_MAXSIZE == CAP and self.det.num_point == 5
        with torch.no_grad():
            plans = lambda: (center_predict.StaticPredictPlan(self.cfg, self.head.num_classes, B, SIZE, SIZE, False, dev),
                             S.StaticRoIPlan(self.det.roi_head, self.det.second_stage, 5, B, CAP, CAP, C, self.bev.dtype, dev))
            (self.predict, self.roi), (self.predict_g, self.roi_g) = plans(), plans()   # the eager and the captured route own their buffers
            assert self.predict.cap == CAP
            run = lambda: self.roi_g.run(self.predict_g.run(self.maps), self.bev)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    run()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                run()

    @torch.no_grad()
    def route_a(self):
        return self.det._forward_device(self.head.predict({}, self.maps, self.cfg), self.bev, {}, False)

    @torch.no_grad()
    def route_b(self):
        out = self.roi.run(self.predict.run(self.maps), self.bev)
        return [out.boxes, out.scores, out.labels, out.counts]

    def route_c(self):
        self.graph.replay()
        return [self.roi_g.boxes, self.roi_g.scores, self.roi_g.labels, self.roi_g.counts]

    def check(self, a, b, c):
        for out, name in ((b, "eager"), (c, "graph")):
            counts = out[3].tolist()
            assert counts == [len(x["scores"]) for x in a], f"route {name} and predict disagree on the counts"
            for s, n in enumerate(counts):
                ok = torch.equal(out[0][s, :n], a[s]["box3d_lidar"]) and torch.equal(out[1][s, :n], a[s]["scores"]) and torch.equal(out[2][s, :n], a[s]["label_preds"])
                assert ok and bool((out[2][s, n:] == -1).all()) and not bool(out[0][s, n:].any()), f"route {name} and _forward_device disagree (sample {s})"
        return b[3].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--peaks", type=int, default=600, help="heat-map peaks per sample; about three quarters pass the threshold")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_two_stage_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("static_two_stage_bench: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    r = Routes(args.peaks, dev)
    paths = [("(a) predict + _forward_device", r.route_a), ("(b) predict plan + StaticRoIPlan.run", r.route_b), ("(c) one graph replay", r.route_c)]
    ev, wall = {n: [] for n, _ in paths}, {n: [] for n, _ in paths}
    counts = []
    for k in range(args.warmup + args.runs):   # the routes alternate
        outs = []
        for name, fn in paths:
            e, w, out = timed(fn)
            outs.append(out)
            if k >= args.warmup:
                ev[name].append(e)
                wall[name].append(w)
        counts = r.check(*outs)
    lines = [f"# head maps + neck map -> refined detections (Waymo 1 task, B = {B}, {SIZE} x {SIZE} maps, rotated NMS, {args.peaks} peaks per sample; "
             f"{SIZE} x {SIZE} x {C} channels_last bf16 neck map, cap {CAP}, num_point 5): three routes alternating on the same inputs, boxes, scores and "
             f"labels asserted bit-equal every round; median (min) of {args.runs} rounds after {args.warmup} warm-ups, HIP events around the call and the "
             f"host's wall time of it; device {torch.cuda.get_device_name(0)}",
             f"# stated plan of the static second stage: {S.STATIC_ROI_LAUNCHES} launches, no host read, no copy (7 + {S.STATIC_ROI_LAUNCHES} with the static "
             f"predict); counted below from a profiler trace of one extra round.  Route (a) is the yardstick",
             f"detections per sample in the last round: {counts}; MLP repacks {r.roi.repacks + r.roi_g.repacks}"]
    for name, fn in paths:   # one extra round under the profiler
        try:
            kernels, d2h, blocking = counts_of(fn)
            cnt = f"{kernels} launches, {d2h} device-to-host copies, blocking calls {dict(blocking) or 'none'}"
        except Exception as exc:   # the counts are a side figure: the timing stands without them
            cnt = f"launch count not taken ({type(exc).__name__})"
        lines.append(f"  {name:38s} events {med(ev[name])}   host wall {med(wall[name])}   {cnt}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
