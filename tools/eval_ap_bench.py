#!/usr/bin/env python
"""Detection AP evaluation (sparse2dense_amd.evaluation) on a synthetic validation split: the device route (csrc/eval_ap.hip) beside this
project's host definition, in one process on the same annotations.

    python tools/eval_ap_bench.py [--frames 4000] [--compare-frames 100] [--runs 3] [--out profiles/eval_ap_bench.txt]

Split: `frames` frames on a 150 m field, 50 - 70 ground truths and 180 - 220 detections per frame, classes Car / Pedestrian / Cyclist, lidar
boxes through `Evaluator`'s conventions (dummy image box, occlusion 0, truncation 0, alpha -10, one difficulty).  Four of five ground truths
have a jittered detection, the other detections are scattered.  Before anything is measured the detections behind a decision that is not
margin-clear are dropped, with the device's own overlaps: an overlap within 1e-4 of one of the overlap levels 0.25, 0.30 .. 0.95, or a
ground truth with two candidates (overlap above 0.2) - detections after NMS rarely share an object.  So both routes take the same decisions
and their outputs are asserted equal.

Rows: `get_official_eval_result` and `get_coco_eval_result`.  Device: HIP events around the call and the host's wall time of it, median (min)
of `runs` calls after one warm-up, launches and host reads from evaluation.device_stats.  The host definition is numpy with a Python loop
over the ground truths (the reference's is numba, which is not available here, so no figure for the reference is given); it runs once, on
the first `compare-frames` frames (a twentieth of that for the coco result, which walks 10 overlaps x 3 difficulties: it takes about two
seconds per frame), where the device route is run again on the same frames and the outputs are asserted equal."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sparse2dense_amd import evaluation as E  # noqa: E402

NAMES = ["Car", "Pedestrian", "Cyclist"]
SIZES = np.array([(4.2, 1.8, 1.6), (0.8, 0.7, 1.75), (1.8, 0.7, 1.7)])


def make_split(frames, seed, dev):
    """(gt boxes [G, 7], gt labels, gt counts, det boxes [D, 7], det labels, det scores, det counts) on the device"""
    rs = np.random.RandomState(seed)
    ng, nd = rs.randint(50, 71, frames), rs.randint(180, 221, frames)
    g_total, d_total = int(ng.sum()), int(nd.sum())
    g_lab = rs.choice(3, g_total, p=[0.6, 0.25, 0.15])
    g_box = np.concatenate([rs.uniform(-75, 75, (g_total, 2)), rs.uniform(-1, 1, (g_total, 1)), SIZES[g_lab] * rs.uniform(0.9, 1.1, (g_total, 3)),
                            rs.uniform(-3.1, 3.1, (g_total, 1))], 1)
    d_lab = rs.choice(3, d_total, p=[0.6, 0.25, 0.15])
    d_box = np.concatenate([rs.uniform(-75, 75, (d_total, 2)), rs.uniform(-1, 1, (d_total, 1)), SIZES[d_lab] * rs.uniform(0.9, 1.1, (d_total, 3)),
                            rs.uniform(-3.1, 3.1, (d_total, 1))], 1)
    g_off, d_off = np.concatenate([[0], np.cumsum(ng)]), np.concatenate([[0], np.cumsum(nd)])
    for f in range(frames):   # the first 0.8 ng detections of a frame sit on its first ground truths
        k = int(0.8 * ng[f])
        src = g_box[g_off[f]:g_off[f] + k]
        jit = src.copy()
        jit[:, :3] += rs.uniform(-0.15, 0.15, (k, 3)) * src[:, 3:6]
        jit[:, 3:6] *= rs.uniform(0.95, 1.05, (k, 3))
        jit[:, 6] += rs.uniform(-0.1, 0.1, k)
        d_box[d_off[f]:d_off[f] + k] = jit
        d_lab[d_off[f]:d_off[f] + k] = g_lab[g_off[f]:g_off[f] + k]
    t = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)
    return (t(g_box, torch.float32), t(g_lab, torch.int64), ng, t(d_box, torch.float32), t(d_lab, torch.int64),
            t(rs.uniform(0.05, 0.99, d_total), torch.float32), nd)


def evaluator_of(split, keep=None, frames=None):
    g_box, g_lab, ng, d_box, d_lab, d_score, nd = split
    ev = E.Evaluator(NAMES, z_axis=2, z_center=0.5)
    g_off, d_off = np.concatenate([[0], np.cumsum(ng)]), np.concatenate([[0], np.cumsum(nd)])
    for f in range(len(ng) if frames is None else frames):
        rows = torch.arange(d_off[f], d_off[f + 1], device=d_box.device)
        if keep is not None:
            rows = rows[keep[d_off[f]:d_off[f + 1]]]
        ev.add([dict(box3d_lidar=d_box[rows], scores=d_score[rows], label_preds=d_lab[rows])], [g_box[g_off[f]:g_off[f + 1]]],
               [g_lab[g_off[f]:g_off[f + 1]]])
    return ev


def clear_detections(ev):
    """bool [D] on the device: detections to keep so that every decision is margin-clear (see the module text)"""
    packed = E._Packed(ev.gt_annos, ev.dt_annos)
    dev = packed.device
    nd, ng = torch.from_numpy(packed.nd).to(dev), torch.from_numpy(packed.ng).to(dev)
    frame = torch.repeat_interleave(torch.arange(packed.frames, device=dev), nd * ng)
    local = torch.arange(frame.numel(), device=dev) - packed.ov_off[frame]
    det_row = packed.det_off[frame].long() + local % nd[frame]
    gt_row = packed.gt_off[frame].long() + local // nd[frame]
    levels = torch.arange(0.25, 0.96, 0.05, device=dev)
    bad = torch.zeros(int(packed.det_off_h[-1]), dtype=torch.bool, device=dev)
    cand = torch.zeros(frame.numel(), dtype=torch.bool, device=dev)
    for metric in (1, 2):
        ov = E.device_overlaps(packed, metric, 2, 0.5)
        near = ((ov[:, None] - levels[None, :]).abs() < 1e-4).any(1)
        bad[det_row[near]] = True
        cand |= ov > 0.2
    shared = torch.bincount(gt_row[cand], minlength=int(packed.gt_off_h[-1])) >= 2
    bad[det_row[cand & shared[gt_row]]] = True
    return ~bad


def timed(fn, runs):
    fn()
    ev_ms, wall_ms = [], []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms.append(a.elapsed_time(b))
    return out, ev_ms, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--compare-frames", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_ap_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    split = make_split(args.frames, 0, dev)
    keep = clear_detections(evaluator_of(split))
    ev = evaluator_of(split, keep)
    nd, ng = sum(int(a["bbox"].shape[0]) for a in ev.dt_annos), sum(int(a["bbox"].shape[0]) for a in ev.gt_annos)
    lines = [f"# Detection AP evaluation (evaluation.Evaluator over csrc/eval_ap.hip): synthetic split of {args.frames} frames, {nd} detections "
             f"({nd / args.frames:.0f} per frame after {int((~keep).sum())} unclear ones were dropped), {ng} ground truths, 3 classes, 1 "
             f"difficulty; median (min) of {args.runs} calls after 1 warm-up; device {torch.cuda.get_device_name(0)}",
             f"# stated plan: {E.EVAL_CLASS_LAUNCHES} launches + {E.EVAL_CLASS_HOST_READS} host reads per metric, 3 metrics per result call"]
    med = lambda v: f"{np.median(v):9.3f} ms ({min(v):.3f})"
    for kind in ("official", "coco"):
        E.device_stats.update(launches=0, host_reads=0)
        before = dict(E.eval_paths)
        out, ev_ms, wall_ms = timed(getattr(ev, kind), args.runs)
        calls = args.runs + 1
        assert E.eval_paths["host"] == before["host"] and E.eval_paths["device"] == before["device"] + 3 * calls
        lines.append(f"{kind:9s} device, {args.frames} frames   events {med(ev_ms)}   host wall {med(wall_ms)}   "
                     f"{E.device_stats['launches'] // calls} launches, {E.device_stats['host_reads'] // calls} host reads per call")
        sub = evaluator_of(split, keep, max(1, min(args.compare_frames, args.frames) // (20 if kind == "coco" else 1)))
        got, _, wall_dev = timed(getattr(sub, kind), 1)
        host_gt, host_dt = [E._host_anno(a) for a in sub.gt_annos], [E._host_anno(a) for a in sub.dt_annos]
        t0 = time.perf_counter()
        if kind == "official":
            want = E.get_official_eval_result(host_gt, host_dt, [n.lower() for n in NAMES], [0], z_axis=2, z_center=0.5)
        else:
            want = E.get_coco_eval_result(host_gt, host_dt, [n.lower() for n in NAMES], z_axis=2, z_center=0.5)
        wall_host = (time.perf_counter() - t0) * 1e3
        assert got["result"] == want["result"] and got["detail"] == want["detail"], (got["result"], want["result"])
        lines.append(f"{kind:9s} first {len(sub.gt_annos)} frames: device host wall {wall_dev[0]:9.3f} ms, numpy host definition of this project "
                     f"{wall_host:9.3f} ms (1 call), outputs equal")
        lines.append("          " + out["result"].replace("\n", " | "))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
