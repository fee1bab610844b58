#!/usr/bin/env python
"""CenterHead.predict_static (center_predict.StaticPredictPlan: launches only, fixed-capacity outputs) beside CenterHead.predict, in one
process on the same seeded maps - the four rows of tools/center_predict_bench.py.

    python tools/static_predict_bench.py [--runs 20] [--warmup 5] [--out profiles/static_predict_bench.txt]

Per row three routes, alternating: `head.predict` (untouched by the static path: two host reads inside the call), `plan.run` eager, and
`plan.run` replayed from one torch.cuda.graph.  HIP events around the call, median (min) of `runs` calls after `warmup`; the host wall
clock of the same calls; kernel launches per call from a torch.profiler trace of one extra call taken after the timing; and the static
outputs asserted equal to predict's, bit for bit.  Then s2d_segment_topk alone against torch.sort(stable, descending) on score rows
shaped like CenterHead's ([24, 32 400]) and like the anchor head's ([4, 212 064]), about 1 % of the cells passing."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import predict_tasks_util as U  # noqa: E402
from center_predict_bench import ROWS, counts_of, head_of, one_call  # noqa: E402
from sparse2dense_amd import _lib, center_predict  # noqa: E402


def equal(det, want):
    counts = det.counts.tolist()
    return counts == [len(w["scores"]) for w in want] and all(
        torch.equal(det.boxes[b, :n], w["box3d_lidar"]) and torch.equal(det.scores[b, :n], w["scores"]) and torch.equal(det.labels[b, :n], w["label_preds"])
        for b, (n, w) in enumerate(zip(counts, want)))


def fmt(ms):
    return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f})"


def predict_rows(args, lines):
    for title, classes, vel, size, cfg in ROWS:
        flip = bool(cfg.get("double_flip", False))
        maps = [{k: v.cuda() for k, v in U.seeded_task_maps(c, 7000 + i, size, size, 4, flip, vel=vel, peaks=args.peaks).items()}
                for i, c in enumerate(classes)]
        head = head_of(classes, vel)
        plan = center_predict.StaticPredictPlan(cfg, head.num_classes, 4, size, size, vel, maps[0]["hm"].device)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                plan.run(maps)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            det = plan.run(maps)
        routes = {"predict": lambda: head.predict({}, maps, cfg), "static eager": lambda: plan.run(maps), "static graph": graph.replay}
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
        assert head.predict_paths["torch"] == 0
        try:
            cnt = {k: f"{counts_of(fn)[0]} launches" for k, fn in routes.items()}
        except Exception as exc:   # a side figure: the timing stands without it
            cnt = {k: f"launch count not taken ({type(exc).__name__})" for k in routes}
        lines.append(f"{title}: {len(classes) * 4} segments, k = {plan.k}, {int(det.counts.sum())} boxes kept, overflow flags set: "
                     f"{int(det.overflow.sum())}, static outputs equal predict's bit for bit: {same}")
        for k in routes:
            lines.append(f"    {k:13s} {fmt(ev[k])}   host wall {statistics.median(wall[k]):8.3f} ms   {cnt[k]}")
        m = {k: statistics.median(v) for k, v in ev.items()}
        lines.append(f"    predict / static eager = x{m['predict'] / m['static eager']:.2f}, predict / static graph = x{m['predict'] / m['static graph']:.2f}")


def topk_rows(args, lines):
    lib = _lib.load()
    gen = torch.Generator().manual_seed(5)
    for segs, n, k in ((24, 32400, 1000), (4, 212064, 1000)):
        score = torch.sigmoid(torch.randn(segs, n, generator=gen))
        score[torch.rand(segs, n, generator=gen) < 0.99] = float("-inf")
        score = score.cuda()
        order = torch.empty((segs, k), dtype=torch.int64, device="cuda")
        sorted_ = torch.empty((segs, k), dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        routes = {"s2d_segment_topk": lambda: _lib.check(lib.s2d_segment_topk(score.data_ptr(), segs, n, n, k, None, order.data_ptr(), sorted_.data_ptr(), k,
                                                                                None, None, None, st), "s2d_segment_topk"),
                  "torch.sort": lambda: torch.sort(score, dim=1, descending=True, stable=True)}
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ev = {k_: [] for k_ in routes}
        for _ in range(args.runs):
            for k_, fn in routes.items():
                e, _, out = one_call(fn)
                ev[k_].append(e)
        same = torch.equal(order, out[1][:, :k]) and torch.equal(sorted_, out[0][:, :k])
        assert same, f"top-K of [{segs}, {n}] differs from torch.sort"
        m = {k_: statistics.median(v) for k_, v in ev.items()}
        lines.append(f"score rows [{segs}, {n}], k = {k}, about 1 % of the cells above -inf, first k columns equal: {same}")
        for k_ in routes:
            lines.append(f"    {k_:17s} {fmt(ev[k_])}")
        ratio = m["torch.sort"] / m["s2d_segment_topk"]
        lines.append(f"    torch.sort / s2d_segment_topk = x{ratio:.2f}" + ("" if ratio >= 1 else "   (the select kernel is SLOWER on this row)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--peaks", type=int, default=400, help="heat-map peaks per (task, sample); about three quarters pass the threshold")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_predict_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("static_predict_bench: no GPU - nothing is measured without one")
    lines = [f"# CenterHead.predict vs StaticPredictPlan.run (eager, and replayed from one HIP graph): median (min) of {args.runs} calls after {args.warmup} "
             f"warm-ups, routes alternating, HIP events around the call; device {torch.cuda.get_device_name(0)}; {args.peaks} heat-map peaks per segment"]
    predict_rows(args, lines)
    lines.append("# s2d_segment_topk alone against torch.sort(stable, descending) of the whole rows")
    topk_rows(args, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
