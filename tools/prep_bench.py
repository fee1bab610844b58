#!/usr/bin/env python
"""Frame preparation of the S2D data step on the device (sparse2dense_amd/prep.py over csrc/prep.hip) beside this project's numpy
restatement of it, on one frame: 150 000 points, 100 boxes, about 20 000 stored object points.

    python tools/prep_bench.py [--runs 20] [--warmup 5] [--points 150000] [--boxes 100] [--stored 20000] [--out profiles/prep_bench.txt]

Rows: the composition (prep.compose_clouds: five launches and the frame's one host read, which is inside the timed span), the global noise
(one launch over the three clouds, host draws included), the shuffle (two permutation draws, two uploads, two gathers) and the whole
prep.S2DPreprocess call on a device-resident sweep with device-resident stored clouds.  HIP events around each span, median (min) of `runs`
calls after `warmup`; beside the event time the host's wall time of the same span (the host read and the draws are host work).  Launches
and host reads come from a torch.profiler trace of one extra call (tools/center_predict_bench.py: counts_of).
The numpy row is THIS PROJECT's restatement of the step (prep.py, the definition the tests use), timed on the same machine's host: the
reference's numba path is not available here, so no figure for it is given."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_predict_bench import counts_of  # noqa: E402
from sparse2dense_amd import prep, scene  # noqa: E402

CFG = dict(mode="train", shuffle_points=True, distillation=True, global_rot_noise=[-0.78539816, 0.78539816], global_scale_noise=[0.95, 1.05],
           global_translate_std=0.5, db_sampler=None, class_names=list(scene.WAYMO_CLASS_NAMES), no_augmentation=False)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out


def med(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f})"


def measure(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(runs):
        e, w, _ = timed(fn)
        ev.append(e)
        wall.append(w)
    try:
        kernels, d2h, blocking = counts_of(fn)
        cnt = f"{kernels} launches, {d2h} device-to-host copies, blocking calls {dict(blocking)}"
    except Exception as exc:   # the counts are a side figure: the timing stands without them
        cnt = f"launch count not taken ({type(exc).__name__})"
    return f"events {med(ev)}   host wall {med(wall)}   {cnt}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--stored", type=int, default=20000)
    ap.add_argument("--numpy-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prep_bench: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    s = scene.make_scene(args.points, seed=20240928)
    keep = slice(0, min(args.boxes, len(s["gt_boxes"])))
    s = dict(points=s["points"], gt_boxes=s["gt_boxes"][keep], gt_classes=s["gt_classes"][keep])
    objects = scene.make_object_clouds(s, seed=5, n_total=args.stored)
    boxes = s["gt_boxes"]
    names = np.array([scene.WAYMO_CLASS_NAMES[c - 1] for c in s["gt_classes"]])
    signs = [f"object_{j}" for j in range(len(names))]
    kinds = prep.kinds_of(names)
    packed = [g if g is not None else np.zeros((0, 5), np.float32) for g in objects]
    obj_np = np.concatenate(packed, 0)
    off = np.cumsum([0] + [len(g) for g in packed]).astype(np.int32)
    pts_dev, obj_dev = torch.from_numpy(s["points"]).to(dev), torch.from_numpy(obj_np).to(dev)
    store_dev = {n: torch.from_numpy(g).to(dev) for n, g in zip(signs, objects) if g is not None}
    store_np = {n: g for n, g in zip(signs, objects) if g is not None}

    dense, recon = prep.compose_clouds(pts_dev, boxes, kinds, obj_dev, off)
    inside = int(prep.points_in_rbbox(pts_dev, torch.from_numpy(boxes).to(dev)).any(1).sum())

    def whole(points, store):
        step = prep.S2DPreprocess(CFG, object_store=store.get)
        res = dict(type="WaymoDataset", lidar=dict(points=points, annotations=dict(boxes=boxes.copy(), names=names)))
        return step(res, dict(gt_boxes=boxes, gt_names=names, gt_signs=signs))

    np.random.seed(0)
    lines = [f"# frame preparation (prep.S2DPreprocess, training mode, distillation): {len(s['points'])} points, {len(boxes)} boxes, {len(obj_np)} stored "
             f"object points in {len(store_np)} objects; {inside} sweep points inside a box; dense cloud {dense.shape[0]} rows, reconstruction cloud "
             f"{recon.shape[0]} rows.  median (min) of {args.runs} calls after {args.warmup} warm-ups, HIP events around the span and the host's wall "
             f"time of it; device {torch.cuda.get_device_name(0)}",
             f"# stated launch plan: composition {prep.COMPOSE_LAUNCHES} launches + {prep.COMPOSE_HOST_READS} host read (3 x int32), noise "
             f"{prep.NOISE_LAUNCHES}, shuffle {prep.SHUFFLE_LAUNCHES_PER_CLOUD} per cloud; counted below from a profiler trace (uploads of boxes, kinds, "
             f"offsets and permutations are copies, not launches)"]
    lines.append("composition  " + measure(lambda: prep.compose_clouds(pts_dev, boxes, kinds, obj_dev, off), args.runs, args.warmup))
    clouds = [pts_dev.clone(), dense.clone(), recon.clone()]
    lines.append("global noise " + measure(lambda: prep.global_noise(boxes.copy(), *clouds, CFG), args.runs, args.warmup))
    lines.append("shuffle      " + measure(lambda: prep.shuffle_points(clouds[0], clouds[1]), args.runs, args.warmup))
    lines.append("whole call   " + measure(lambda: whole(pts_dev.clone(), store_dev), args.runs, args.warmup))
    t = []
    for _ in range(args.numpy_runs):
        p = s["points"].copy()
        t0 = time.perf_counter()
        whole(p, store_np)
        t.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"numpy restatement of this project (prep.py on the host, NOT the reference's numba path), whole call: {med(t)} over {args.numpy_runs} calls")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
