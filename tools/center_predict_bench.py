#!/usr/bin/env python
"""CenterHead.predict: the device path (csrc/center_predict.hip + the batched NMS) beside the per-segment torch chain it replaces
(CenterHead.predict_torch), in one process on the same seeded maps.

    python tools/center_predict_bench.py [--runs 20] [--warmup 5] [--out profiles/center_predict_bench.txt]

Per row: HIP events around one predict() call (the call contains its host reads, so this is the time the stream is held), median (min)
of `runs` calls after `warmup`, the two paths alternating; the host wall clock of the same calls; kernel launches, device-to-host copy
records and blocking runtime calls (synchronous copies and synchronisations: the host side of a host read, and of a small host-to-device
copy) per call, counted from a torch.profiler trace of one extra call taken after the timing, not inside it; and whether both paths
return the same boxes.  The heat maps have a few hundred passing cells per (task, sample) segment (tests/golden/predict_tasks_util.py)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import predict_tasks_util as U  # noqa: E402
from sparse2dense_amd.heads import CenterHead  # noqa: E402

NUSC = dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], nms=dict(nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=0.2),
            score_threshold=0.1, pc_range=[-54.0, -54.0], out_size_factor=8, voxel_size=[0.075, 0.075])
NUSC_CIRCLE = dict(NUSC, pc_range=[-51.2, -51.2], out_size_factor=4, voxel_size=[0.2, 0.2], circular_nms=True, min_radius=[4, 12, 10, 1, 0.85, 0.175])
WAYMO = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], nms=dict(nms_pre_max_size=4096, nms_post_max_size=500, nms_iou_threshold=0.7),
             score_threshold=0.1, pc_range=[-75.2, -75.2], out_size_factor=8, voxel_size=[0.1, 0.1])
SIX = [t["num_class"] for t in U.TASKS]
ROWS = [("nuScenes 6 tasks, B=4, 180x180, rotated NMS", SIX, True, 180, dict(NUSC)),
        ("nuScenes 6 tasks, B=4, 180x180, double_flip (16 maps), rotated NMS", SIX, True, 180, dict(NUSC, double_flip=True)),
        ("nuScenes 6 tasks, B=4, 180x180, circular NMS", SIX, True, 180, dict(NUSC_CIRCLE)),
        ("Waymo 1 task, B=4, 188x188, rotated NMS", [3], False, 188, dict(WAYMO))]


def head_of(classes, vel):
    heads = {k: v for k, v in U.COMMON_HEADS.items() if vel or k != "vel"}
    tasks = [dict(num_class=c, class_names=[f"c{i}_{j}" for j in range(c)]) for i, c in enumerate(classes)]
    return CenterHead(in_channels=64, tasks=tasks, dataset="nuscenes", weight=0.25, code_weights=[1.0] * (10 if vel else 8), common_heads=heads).eval()


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3, out


def counts_of(fn):
    """(kernel launches, device-to-host copy records, blocking runtime calls by name) of one call, from a profiler trace.  The blocking calls
    are the host side of a host read: stream / event synchronisations and synchronous copies (the closing device synchronise of this
    function is left out)."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = d2h = 0
    blocking = Counter()
    for e in prof.events():
        name = e.name.lower()
        if str(e.device_type).endswith("CUDA"):
            if "memcpy" in name:
                d2h += "dtoh" in name or "device -> host" in name or "devicetohost" in name
            elif "memset" not in name:
                kernels += 1
        elif name.startswith("hip") and name != "hipdevicesynchronize" and ("synchronize" in name or name in ("hipmemcpy", "hipmemcpywithstream")):
            blocking[e.name] += 1
    return kernels, d2h, blocking


def same(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x["scores"].shape != y["scores"].shape or not torch.equal(x["label_preds"], y["label_preds"]):
            return False
        if not torch.allclose(x["scores"], y["scores"], rtol=1e-5) or not torch.allclose(x["box3d_lidar"], y["box3d_lidar"], rtol=1e-4, atol=2e-4):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--peaks", type=int, default=400, help="heat-map peaks per (task, sample); about three quarters pass the threshold")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "center_predict_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("center_predict_bench: no GPU - nothing is measured without one")
    lines = [f"# CenterHead.predict, device path vs per-segment torch chain: median (min) of {args.runs} calls after {args.warmup} warm-ups, paths "
             f"alternating, HIP events around the call; device {torch.cuda.get_device_name(0)}; {args.peaks} heat-map peaks per segment"]
    for title, classes, vel, size, cfg in ROWS:
        flip = bool(cfg.get("double_flip", False))
        maps = [{k: v.cuda() for k, v in U.seeded_task_maps(c, 7000 + i, size, size, 4, flip, vel=vel, peaks=args.peaks).items()}
                for i, c in enumerate(classes)]
        head = head_of(classes, vel)
        paths = {"device": lambda: head.predict({}, maps, cfg), "torch": lambda: head.predict_torch({}, maps, cfg)}
        for fn in paths.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ev, wall, out = {k: [] for k in paths}, {k: [] for k in paths}, {}
        for _ in range(args.runs):
            for k, fn in paths.items():
                e, w, out[k] = one_call(fn)
                ev[k].append(e)
                wall[k].append(w)
        assert head.predict_paths["device"] == args.warmup + args.runs and head.predict_paths["torch"] == 0   # (predict_torch is called directly)
        try:
            cnt = {k: counts_of(fn) for k, fn in paths.items()}
            cnt_text = {k: f"{v[0]} launches, {v[1]} device-to-host copy records, {sum(v[2].values())} blocking runtime calls "
                           f"({', '.join(f'{n} x {c}' for n, c in sorted(v[2].items())) or 'none'})" for k, v in cnt.items()}
        except Exception as exc:   # the counts are a side figure: the timing above stands without them
            cnt_text = {k: f"launch count not taken ({type(exc).__name__})" for k in paths}
        kept = sum(len(o["scores"]) for o in out["device"])
        lines.append(f"{title}: {len(classes) * 4} segments, {kept} boxes kept, outputs agree: {same(out['device'], out['torch'])}")
        for k in paths:
            lines.append(f"    {k:6s} {statistics.median(ev[k]):8.3f} ms ({min(ev[k]):.3f})   host wall {statistics.median(wall[k]):8.3f} ms   {cnt_text[k]}")
        ratio = statistics.median(ev["torch"]) / statistics.median(ev["device"])
        lines.append(f"    torch / device = x{ratio:.2f}" + ("" if ratio >= 1 else "   (device path SLOWER on this run)"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
