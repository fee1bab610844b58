#!/usr/bin/env python
"""Six-task (nuScenes) CenterHead: device target assignment and the loss on its two paths, in one process on the same inputs.

    python tools/centerhead_tasks_bench.py [--batch 4] [--boxes 100] [--runs 20] [--warmup 5] > profiles/centerhead_tasks_bench.txt

B frames, 180 x 180 maps, the six tasks / ten classes of waymo_configs.NUSC_TASKS with a velocity branch, `boxes` boxes per frame;
HIP events, median of `runs` timed runs after `warmup`.  Every step runs under its own watchdog (--limit seconds: the process exits
if a step takes longer).
  (i)   targets.assign_label_tasks (torch.zeros for the heat maps + 1 kernel for all tasks)
  (ii)  CenterHead.loss forward + backward of sum(loss), multi-task node (csrc/center_loss.hip: 2 launches + zero-fill + 2)
  (iii) the same with S2D_CENTER_FUSED_LOSS=0: the per-task loop (sigmoid, clamp, focal 2 + 2, cat, RegLoss 1 + 2, weights ...)
Launch counts are device kernels seen by torch.profiler during one forward + backward."""
import argparse
import faulthandler
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sparse2dense_amd import heads, scene, targets  # noqa: E402
from sparse2dense_amd.waymo_configs import NUSC_TASKS, nusc_centerpoint_dcn  # noqa: E402

BRANCHES = {"reg": 2, "height": 1, "dim": 3, "vel": 2, "rot": 2}


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


def launches(fn):
    """device kernels of one call, or None where the profiler is not available"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as err:   # the figure is informative only
        print(f"# (launch count not available: {type(err).__name__}: {err})")
        return None


def random_frames(batch, boxes, seed=50):
    lo, hi = np.array(scene.NUSC_RANGE[:2]) + 1.0, np.array(scene.NUSC_RANGE[3:5]) - 1.0
    out = []
    for f in range(batch):
        rs = np.random.RandomState(seed + f)
        cls = rs.randint(1, 11, boxes).astype(np.int32)
        b = np.concatenate([rs.uniform(lo, hi, (boxes, 2)), rs.uniform(-2, 0.5, (boxes, 1)), rs.uniform(0.4, 8.0, (boxes, 3)),
                            rs.normal(0, 2, (boxes, 2)), rs.uniform(-np.pi, np.pi, (boxes, 1))], 1).astype(np.float32)
        out.append((b, cls))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step before the watchdog ends the process")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = random_frames(args.batch, args.boxes)
    boxes, classes = targets.pad_boxes([f[0] for f in frames], [f[1] for f in frames], dev)
    print(f"# six-task CenterHead micro-benchmark: B = {args.batch}, 180 x 180 maps, {len(NUSC_TASKS)} tasks / 10 classes, {args.boxes} boxes per "
          f"frame, median (min) of {args.runs} runs after {args.warmup} warm-ups, HIP events; device {torch.cuda.get_device_name(0)}")

    faulthandler.dump_traceback_later(args.limit, exit=True)
    assign = lambda: targets.assign_label_tasks(boxes, classes, NUSC_TASKS, with_boxes_and_cls=True)
    example = assign()
    host = scene.assign_targets_tasks(frames[0][0], frames[0][1], NUSC_TASKS)
    same = all(np.array_equal(example[k][t][0].cpu().numpy(), host[k][t]) for k in ("ind", "mask", "cat") for t in range(len(NUSC_TASKS)))
    t_assign = timed(assign, args.runs, args.warmup)
    n_assign = launches(assign)
    faulthandler.cancel_dump_traceback_later()
    print(f"(i)   target assignment          {t_assign[0]:8.3f} ms ({t_assign[1]:.3f})   launches {n_assign}   ind / mask / cat of frame 0 equal to the host "
          f"restatement: {same}, positives per task {[int(m.sum()) for m in example['mask']]}")

    cfg = dict(nusc_centerpoint_dcn()["bbox_head"], in_channels=64, dcn_head=False)
    cfg.pop("type")
    head = heads.CenterHead(**cfg).to(dev)
    g = torch.Generator().manual_seed(3)
    raw = [dict({"hm": torch.randn(args.batch, t["num_class"], 180, 180, generator=g) * 2 - 2.19},
                **{k: torch.randn(args.batch, c, 180, 180, generator=g) for k, c in BRANCHES.items()}) for t in NUSC_TASKS]
    leaves = [{k: v.to(dev).requires_grad_(True) for k, v in p.items()} for p in raw]

    def step():
        for p in leaves:
            for v in p.values():
                v.grad = None
        # (the per-task loop applies the sigmoid in place: hand it copies of the logits; the copies are part of BOTH timings)
        preds = [dict(p, hm=p["hm"] * 1.0) for p in leaves]
        losses = head.loss(example, preds)
        sum(losses["loss"]).backward()
        return losses

    results = {}
    for name, switch in (("fused", "1"), ("loop", "0")):
        faulthandler.dump_traceback_later(args.limit, exit=True)
        os.environ["S2D_CENTER_FUSED_LOSS"] = switch
        losses = step()
        results[name] = dict(loss=[float(v) for v in losses["loss"]], grads=[{k: v.grad.clone() for k, v in p.items()} for p in leaves],
                             time=timed(step, args.runs, args.warmup), launches=launches(step))
        faulthandler.cancel_dump_traceback_later()
    os.environ.pop("S2D_CENTER_FUSED_LOSS")
    f, l = results["fused"], results["loop"]
    err = max(float((a[k] - b[k]).abs().max() / b[k].abs().max()) for a, b in zip(f["grads"], l["grads"]) for k in a)
    rel = max(abs(a - b) / abs(b) for a, b in zip(f["loss"], l["loss"]))
    print(f"(ii)  loss fwd + bwd, one node     {f['time'][0]:8.3f} ms ({f['time'][1]:.3f})   launches {f['launches']} (6 of them the copies of the logits, "
          f"the rest the node and autograd's sum / stack around it)")
    print(f"(iii) loss fwd + bwd, per-task loop {l['time'][0]:8.3f} ms ({l['time'][1]:.3f})   launches {l['launches']}   x{l['time'][0] / f['time'][0]:.2f}   "
          f"max loss difference {rel:.1e}, max gradient difference / max gradient {err:.1e}")


if __name__ == "__main__":
    main()
