#!/usr/bin/env python
"""MultiGroupHead.predict: the device path (csrc/anchor_predict.hip + the batched rotated NMS) beside the per-segment chain it replaces
(MultiGroupHead.predict_torch), in one process on the same seeded predictions.

    python tools/anchor_predict_bench.py [--runs 20] [--warmup 5] [--out profiles/anchor_predict_bench.txt]

Waymo SECOND: one task, 188 x 188 cells x 6 anchors, SECOND_TEST_CFG.  Per row: HIP events around one predict() call (the call contains
its host reads, so this is the time the stream is held), median (min) of `runs` calls after `warmup`, the two paths alternating; the host
wall clock of the same calls; kernel launches, device-to-host copy records and blocking runtime calls per call, counted from a
torch.profiler trace of one extra call taken after the timing, not inside it (tools/center_predict_bench.py: counts_of); and the assertion
that both paths return the same boxes, bit for bit.  The predictions are made like tests/anchor_util.predict_inputs: every class logit at
-6 except around fake objects on a lattice, whose rotation slots get logits U(-1.5, 3) - all of those pass score_threshold 0.1."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_predict_bench import counts_of, one_call  # noqa: E402
from sparse2dense_amd import anchors as A, waymo_configs as WC  # noqa: E402
from sparse2dense_amd.registry import build_head  # noqa: E402

H = W = 188
SLOTS = 6
# title, batch, objects per frame, lattice step in cells (14: objects never touch; 5: a crowded frame whose boxes overlap)
ROWS = [("B=4, ~250 anchors pass per frame", 4, 94, 14),
        ("B=4, more than nms_pre_max_size (1000) pass per frame: the cut is taken", 4, 450, 5),
        ("B=1, ~250 anchors pass", 1, 94, 14)]


def inputs(batch, objects, step, seed=4300):
    g = torch.Generator().manual_seed(seed)
    box = torch.randn((batch, H, W, SLOTS, 7), generator=g) * 0.05
    dirs = torch.randn((batch, H, W, SLOTS, 2), generator=g)
    cls = torch.full((batch, H, W, SLOTS, 3), -6.0)
    lattice = [(y, x) for y in range(10, H - 10, step) for x in range(10, W - 10, step)]
    assert objects <= len(lattice)
    for b in range(batch):
        for i in torch.randperm(len(lattice), generator=g)[:objects].tolist():
            y, x = lattice[i]
            c = int(torch.randint(0, 3, (1,), generator=g))
            for dx in ((0, 1) if c == 0 else (0,)):   # a VEHICLE also lights the cell to its right
                for r in range(2):
                    cls[b, y, x + dx, 2 * c + r, c] = float(torch.rand(1, generator=g) * 4.5 - 1.5)
    return [t.reshape(batch, H, W, -1) for t in (box, cls, dirs)]


def identical(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("box3d_lidar", "scores", "label_preds"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_predict_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("anchor_predict_bench: no GPU - nothing is measured without one")
    os.environ.pop("S2D_ANCHOR_DEVICE_PREDICT", None)
    cfg = WC.SECOND_TEST_CFG
    table = torch.from_numpy(A.get_assigner(WC.SECOND_ASSIGNER).anchors_numpy([1, H, W])).cuda()
    lines = [f"# MultiGroupHead.predict (Waymo SECOND, 1 task, {H} x {W} x {SLOTS} anchors, SECOND_TEST_CFG), device path vs per-segment chain "
             f"(predict_torch): median (min) of {args.runs} calls after {args.warmup} warm-ups, paths alternating, HIP events around the call; "
             f"device {torch.cuda.get_device_name(0)}"]
    for title, batch, objects, step in ROWS:
        box, cls, dirs = [t.cuda() for t in inputs(batch, objects, step)]
        preds = [dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)]
        example = dict(anchors=[table.unsqueeze(0).expand(batch, -1, -1)])
        head = build_head(WC.second_voxelnet_train()["bbox_head"]).cuda().eval()
        paths = {"device": lambda: head.predict(example, preds, cfg), "torch": lambda: head.predict_torch(example, preds, cfg)}
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
        assert head.predict_paths == {"device": args.warmup + args.runs, "torch": 0}, head.predict_paths   # (predict_torch is called directly)
        assert identical(out["device"], out["torch"]), f"{title}: the two paths disagree"
        passed = (torch.sigmoid(cls.reshape(batch, -1, 3)).amax(-1) >= cfg["score_threshold"]).sum(1).tolist()
        try:
            cnt = {k: counts_of(fn) for k, fn in paths.items()}
            cnt_text = {k: f"{v[0]} launches, {v[1]} device-to-host copy records, {sum(v[2].values())} blocking runtime calls "
                           f"({', '.join(f'{n} x {c}' for n, c in sorted(v[2].items())) or 'none'})" for k, v in cnt.items()}
        except Exception as exc:   # the counts are a side figure: the timing above stands without them
            cnt_text = {k: f"launch count not taken ({type(exc).__name__})" for k in paths}
        kept = sum(len(o["scores"]) for o in out["device"])
        lines.append(f"{title}: anchors passing per frame {passed}, {kept} boxes kept, outputs identical: True")
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
