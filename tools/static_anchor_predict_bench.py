#!/usr/bin/env python
"""MultiGroupHead.predict_static (anchor_predict.StaticAnchorPlan: launches only, fixed-capacity outputs) beside MultiGroupHead.predict, in
one process on the same seeded predictions - the three rows of tools/anchor_predict_bench.py.

    python tools/static_anchor_predict_bench.py [--runs 20] [--warmup 5] [--out profiles/static_anchor_predict_bench.txt]

Waymo SECOND: one task, 188 x 188 cells x 6 anchors, SECOND_TEST_CFG.  Per row three routes, alternating: `head.predict` (untouched by the
static path: a full sort and two host reads inside the call), `plan.run` eager, and `plan.run` replayed from one torch.cuda.graph.  HIP
events around the call, median (min) of `runs` calls after `warmup`; the host wall clock of the same calls; kernel launches, device-to-host
copy records and blocking runtime calls per call from a torch.profiler trace of one extra call taken after the timing; and the static
outputs asserted equal to predict's, bit for bit, at every round.  No threshold is set: the path is opt-in and no default depends on
these numbers."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from anchor_predict_bench import H, ROWS, SLOTS, W, inputs  # noqa: E402
from center_predict_bench import counts_of, one_call  # noqa: E402
from static_predict_bench import equal, fmt  # noqa: E402
from sparse2dense_amd import anchor_predict, anchors as A, waymo_configs as WC  # noqa: E402
from sparse2dense_amd.registry import build_head  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_anchor_predict_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("static_anchor_predict_bench: no GPU - nothing is measured without one")
    os.environ.pop("S2D_ANCHOR_DEVICE_PREDICT", None)
    cfg = WC.SECOND_TEST_CFG
    table = torch.from_numpy(A.get_assigner(WC.SECOND_ASSIGNER).anchors_numpy([1, H, W])).cuda()
    lines = [f"# MultiGroupHead.predict vs StaticAnchorPlan.run (eager, and replayed from one HIP graph), Waymo SECOND, 1 task, {H} x {W} x {SLOTS} "
             f"anchors, SECOND_TEST_CFG: median (min) of {args.runs} calls after {args.warmup} warm-ups, routes alternating, HIP events around the "
             f"call; device {torch.cuda.get_device_name(0)}"]
    for title, batch, objects, step in ROWS:
        box, cls, dirs = [t.cuda() for t in inputs(batch, objects, step)]
        preds = [dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)]
        example = dict(anchors=[table.unsqueeze(0).expand(batch, -1, -1)])
        head = build_head(WC.second_voxelnet_train()["bbox_head"]).cuda().eval()
        plan = anchor_predict.StaticAnchorPlan(cfg, head.num_classes, [table], batch, head.use_direction_classifier, head.direction_offset, box.device)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                plan.run(preds)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            det = plan.run(preds)
        routes = {"predict": lambda: head.predict(example, preds, cfg), "static eager": lambda: plan.run(preds), "static graph": graph.replay}
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ev, wall, same = {k: [] for k in routes}, {k: [] for k in routes}, True
        for _ in range(args.runs):
            for k, fn in routes.items():
                e, w, out = one_call(fn)
                ev[k].append(e)
                wall[k].append(w)
                if k == "predict":
                    want = out
                else:
                    same = same and equal(det, want)   # (after the events: the comparison reads the counts)
        assert same, f"{title}: the static outputs differ from predict's"
        assert head.predict_paths == {"device": args.warmup + args.runs, "torch": 0}, head.predict_paths
        try:
            cnt = {}
            for k, fn in routes.items():
                v = counts_of(fn)
                cnt[k] = (f"{v[0]} launches, {v[1]} device-to-host copy records, {sum(v[2].values())} blocking runtime calls "
                          f"({', '.join(f'{n} x {c}' for n, c in sorted(v[2].items())) or 'none'})")
        except Exception as exc:   # a side figure: the timing stands without it
            cnt = {k: f"launch count not taken ({type(exc).__name__})" for k in routes}
        passed = (torch.sigmoid(cls.reshape(batch, -1, 3)).amax(-1) >= cfg["score_threshold"]).sum(1).tolist()
        lines.append(f"{title}: anchors passing per frame {passed}, k = {plan.k}, {int(det.counts.sum())} boxes kept, pre_max cuts taken: "
                     f"{int(det.overflow.sum())}, static outputs equal predict's bit for bit: {same}")
        for k in routes:
            lines.append(f"    {k:13s} {fmt(ev[k])}   host wall {statistics.median(wall[k]):8.3f} ms   {cnt[k]}")
        m = {k: statistics.median(v) for k, v in ev.items()}
        lines.append(f"    predict / static eager = x{m['predict'] / m['static eager']:.2f}, predict / static graph = x{m['predict'] / m['static graph']:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
