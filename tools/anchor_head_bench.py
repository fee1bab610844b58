#!/usr/bin/env python
"""SECOND anchor head: the three HIP paths of csrc/anchor_head.hip beside torch restatements of the reference formulas run on the same
device in the same process (that chain of elementwise launches, not the new code, is the baseline).

    python tools/anchor_head_bench.py [--batch 4] [--boxes 100] [--runs 20] [--warmup 5] > profiles/anchor_head_bench.txt

B frames, A = 212 064 anchors, ~`boxes` boxes per frame; HIP events, median of `runs` timed runs after `warmup`.
  (i)   assignment chain (zero-fill + 2 kernels)      vs  per-frame, per-class float64 overlap matrices + argmax / tie test in torch
  (ii)  loss forward + backward (2 + 1 kernels)       vs  tests/anchor_util.loss_restatement (fp32) + autograd
  (iii) decode (1 kernel)                             vs  sigmoid / max / second_box_decode / argmax / threshold in torch"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import anchor_util as AU  # noqa: E402
from sparse2dense_amd import anchors as A, waymo_configs as WC  # noqa: E402


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def torch_decode(box, cls, dirs, anchors, thr):
    b = box.shape[0]
    dec = A.GroundBox3dCoder().decode_torch(box.view(b, -1, 7), anchors[None])
    scores, labels = torch.sigmoid(cls.view(b, -1, 3)).max(-1)
    return dec, scores, labels, dirs.view(b, -1, 2).max(-1)[1], scores >= thr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    asg = A.get_assigner(WC.SECOND_ASSIGNER)
    table = asg.anchors_numpy([1, AU.H, AU.W])
    anchors = torch.from_numpy(table).to(dev)
    frames = [AU.random_boxes(np.random.default_rng(50 + f), args.boxes) for f in range(args.batch)]
    boxes_np, classes_np = AU.pad_frames(frames)
    boxes, classes = torch.from_numpy(boxes_np).to(dev), torch.from_numpy(classes_np).to(dev)
    matched, unmatched = [float(v) for v in asg.matched], [float(v) for v in asg.unmatched]
    print(f"# anchor head micro-benchmark: B = {args.batch}, A = {len(table)}, {args.boxes} boxes per frame, median (min) of {args.runs} runs "
          f"after {args.warmup} warm-ups, HIP events; device {torch.cuda.get_device_name(0)}")

    out = A.assign_anchor_targets(boxes, classes, WC.SECOND_ASSIGNER)
    ref = AU.assign_restatement(boxes, classes, anchors, matched, unmatched)
    same = bool(torch.equal(out["labels"][0], ref[0]))
    hip = timed(lambda: A.assign_anchor_targets(boxes, classes, WC.SECOND_ASSIGNER), args.runs, args.warmup)
    base = timed(lambda: AU.assign_restatement(boxes, classes, anchors, matched, unmatched), args.runs, args.warmup)
    print(f"(i)   assignment        HIP {hip[0]:8.3f} ms ({hip[1]:.3f})   torch {base[0]:8.3f} ms ({base[1]:.3f})   x{base[0] / hip[0]:.1f}   "
          f"labels equal: {same}, positives {int((ref[0] > 0).sum())}")

    labels, targets = out["labels"][0], out["reg_targets"][0]
    preds = [t.to(dev).requires_grad_(True) for t in AU.loss_inputs(args.batch)]

    def hip_loss():
        for t in preds:
            t.grad = None
        A.anchor_loss(*preds, labels, targets, anchors, AU.LOSS_PARAMS)["loss"].backward()

    def torch_loss():
        for t in preds:
            t.grad = None
        AU.loss_restatement(*preds, labels, targets, anchors, dtype=torch.float32)["loss"].backward()
    hip_loss()
    g_hip = [t.grad.clone() for t in preds]
    torch_loss()
    err = max(float((a - t.grad).abs().max() / t.grad.abs().max()) for a, t in zip(g_hip, preds))
    hip, base = timed(hip_loss, args.runs, args.warmup), timed(torch_loss, args.runs, args.warmup)
    mb = args.batch * len(table) * (7 + 3 + 2 + 7 + 1 + 1) * 4 / 1e6
    print(f"(ii)  loss fwd + bwd    HIP {hip[0]:8.3f} ms ({hip[1]:.3f})   torch {base[0]:8.3f} ms ({base[1]:.3f})   x{base[0] / hip[0]:.1f}   "
          f"max gradient difference / max gradient {err:.1e}; algorithmic bytes {mb:.0f} MB forward, ~{2 * mb:.0f} MB with the gradients")

    box, cls, dirs = [t.to(dev) for t in AU.predict_inputs(args.batch)]
    thr = WC.SECOND_TEST_CFG["score_threshold"]
    d_hip, d_ref = A.decode_anchors(box, cls, dirs, anchors, thr), torch_decode(box, cls, dirs, anchors, thr)
    same = bool(torch.equal(d_hip[4], d_ref[4]) and torch.equal(d_hip[2].long(), d_ref[2]))
    hip = timed(lambda: A.decode_anchors(box, cls, dirs, anchors, thr), args.runs, args.warmup)
    base = timed(lambda: torch_decode(box, cls, dirs, anchors, thr), args.runs, args.warmup)
    print(f"(iii) decode            HIP {hip[0]:8.3f} ms ({hip[1]:.3f})   torch {base[0]:8.3f} ms ({base[1]:.3f})   x{base[0] / hip[0]:.1f}   "
          f"candidates and labels equal: {same}, candidates {int(d_ref[4].sum())}")


if __name__ == "__main__":
    main()
