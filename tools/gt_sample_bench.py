#!/usr/bin/env python
"""The GT-database sampler step of the S2D data step on the device (prep.GTSampler over csrc/prep.hip) beside this project's numpy
restatement of it, on one frame: 150 000 points, 100 boxes, sample groups 15 / 10 / 10 over a synthetic database of about 2 000 objects,
resident on the device.

    python tools/gt_sample_bench.py [--runs 20] [--warmup 5] [--points 150000] [--boxes 100] [--objects 2000] [--out profiles/gt_sample_bench.txt]

Rows: the sampler step alone (`sample_all` on the device: the host draws, two uploads, select + count + segments, the one host read, the
paste) and the whole prep.S2DPreprocess call with and without the sampler (with: the pasted blocks in front of the three clouds, the old
clouds copied behind them).  HIP events around each span, median (min) of `runs` calls after `warmup`; beside the event time the host's wall
time of the same span.  Launches and host reads come from a torch.profiler trace of one extra call (tools/center_predict_bench.py:
counts_of).  Every call draws new candidates (the sampler's position moves on), as in training.
The numpy rows are THIS PROJECT's restatement (prep.py, the definition the tests use) on the same machine's host: the reference's numba
path is not available here, so no figure for it is given."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from prep_bench import CFG, med, measure  # noqa: E402
from sparse2dense_amd import prep, scene  # noqa: E402

SIZES = {"VEHICLE": (4.5, 2.0, 1.6), "PEDESTRIAN": (0.8, 0.8, 1.8), "CYCLIST": (1.8, 0.8, 1.7)}


def make_database(n_objects, seed):
    """name -> infos with 9-column boxes on a 150 m field, 20 .. 200 sweep rows each; a third of the objects has a completed cloud"""
    rs = np.random.RandomState(seed)
    db, rows, completed = {}, {}, {}
    for name, share in (("VEHICLE", 0.6), ("PEDESTRIAN", 0.3), ("CYCLIST", 0.1)):
        db[name] = []
        for k in range(int(n_objects * share)):
            size = np.array(SIZES[name]) * rs.uniform(0.85, 1.15, 3)
            box = np.concatenate([rs.uniform(-72, 72, 2), rs.uniform(-0.5, 1.0, 1), size, rs.normal(0, 3, 2), rs.uniform(-3.1, 3.1, 1)]).astype(np.float32)
            n = int(rs.randint(20, 200))
            sign = f"{name}_{k}"
            rows[sign] = np.concatenate([rs.uniform(-1, 1, (n, 3)) * box[3:6] / 2, rs.uniform(0, 1, (n, 2))], 1).astype(np.float32)
            if rs.uniform() < 0.33:
                m = int(rs.randint(200, 800))
                completed[sign] = np.concatenate([rs.uniform(-1, 1, (m, 3)) * box[[4, 3, 5]] / 2 * 1.1, rs.uniform(0, 1, (m, 2))], 1).astype(np.float32)
            db[name].append(dict(name=name, path=sign, box3d_lidar=box, num_points_in_gt=n, difficulty=0, gt_signs=sign))
    return db, rows, completed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--objects", type=int, default=2000)
    ap.add_argument("--numpy-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_sample_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gt_sample_bench: no GPU - nothing is measured without one")
    dev = torch.device("cuda:0")
    s = scene.make_scene(args.points, seed=20240928)
    keep = slice(0, min(args.boxes, len(s["gt_boxes"])))
    s = dict(points=s["points"], gt_boxes=s["gt_boxes"][keep], gt_classes=s["gt_classes"][keep])
    objects = scene.make_object_clouds(s, seed=5, n_total=20000)
    boxes = s["gt_boxes"]
    names = np.array([scene.WAYMO_CLASS_NAMES[c - 1] for c in s["gt_classes"]])
    signs = [f"object_{j}" for j in range(len(names))]
    db, rows, completed = make_database(args.objects, seed=7)
    count = {n: int((names == n).sum()) for n in scene.WAYMO_CLASS_NAMES}
    groups = [{n: count[n] + k} for n, k in zip(scene.WAYMO_CLASS_NAMES, (15, 10, 10))]   # 15 / 10 / 10 candidates per frame
    frame_np = {n: g for n, g in zip(signs, objects) if g is not None}
    store_np = {**completed, **frame_np}
    store_dev = {n: torch.from_numpy(g).to(dev) for n, g in frame_np.items()}
    pts_dev = torch.from_numpy(s["points"]).to(dev)
    np.random.seed(0)
    make = lambda: prep.GTSampler(db, groups, points_of=lambda info: rows[info["path"]])
    sampler = make().resident(dev, object_store=store_np.get)
    host_sampler = make()

    def whole(points, store, smp):
        step = prep.S2DPreprocess(CFG, object_store=store.get, db_sampler=smp)
        res = dict(type="WaymoDataset", lidar=dict(points=points, annotations=dict(boxes=boxes.copy(), names=names)))
        return step(res, dict(gt_boxes=boxes, gt_names=names, gt_signs=signs))

    got = sampler.sample_all(boxes, names, None, device=dev)
    lines = [f"# GT-database sampler (prep.GTSampler.sample_all and prep.S2DPreprocess with it, training mode, distillation): {len(s['points'])} points, "
             f"{len(boxes)} boxes {count}, groups +15 / +10 / +10 over {sum(len(v) for v in db.values())} objects ({sum(len(r) for r in rows.values())} "
             f"sweep rows, {len(completed)} completed clouds of {sum(len(c) for c in completed.values())} rows, resident); first call: "
             f"{len(got['gt_boxes'])} of 35 accepted, {got['points'].shape[0]} sampled rows, {got['recon_points'].shape[0]} reconstruction rows.  median "
             f"(min) of {args.runs} calls after {args.warmup} warm-ups, HIP events around the span and the host's wall time of it; device "
             f"{torch.cuda.get_device_name(0)}",
             f"# stated plan: sampler step {prep.SAMPLER_LAUNCHES} launches + {prep.SAMPLER_HOST_READS} host read (accept[S] and two row counts); counted "
             f"below from a profiler trace (uploads of boxes and row ranges and the copies of the old clouds are copies, not launches)"]
    lines.append("sampler step          " + measure(lambda: sampler.sample_all(boxes, names, None, device=dev), args.runs, args.warmup))
    lines.append("whole call, sampler   " + measure(lambda: whole(pts_dev.clone(), store_dev, sampler), args.runs, args.warmup))
    lines.append("whole call, none      " + measure(lambda: whole(pts_dev.clone(), store_dev, None), args.runs, args.warmup))
    for what, fn in (("sampler step", lambda: host_sampler.sample_all(boxes, names, store_np.get)),
                     ("whole call, sampler", lambda: whole(s["points"].copy(), store_np, host_sampler))):
        t = []
        for _ in range(args.numpy_runs):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"numpy restatement of this project (prep.py on the host, NOT the reference's numba path), {what}: {med(t)} over {args.numpy_runs} calls")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
