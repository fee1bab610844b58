#!/usr/bin/env python
"""One training step of the RoI head - MLP forward, the two RoI losses, backward - on the kernels of csrc/roi_mlp_train.hip
(`RoIHead.fused_training`) beside the torch chain of this same commit (`fused_training = False`: three nn.Sequential's, the head's loss
functions, autograd), in one process on the same inputs.

    python tools/roi_train_bench.py [--runs 20] [--warmup 5] [--out profiles/roi_train_bench.txt]

Shape: the two-stage configs' head (2560 -> 256 -> 256, two branches 256 -> 256 -> 256 -> 1 | 7, DP_RATIO 0.3) with the weights of
tests/test_roi_mlp_cpu.make_head(..., signed=True), R = B x 128 sampled RoIs for B = 1 and B = 4, soft (roi_iou) labels.  A step is
`forward_ret_dict` from the MLP, `get_loss()` - which ends in the reference's `total.item()` on both paths - and `backward()`; target
assignment and BEV sampling are not part of it (tools/two_stage_bench.py times them).  Per row: median (min) of `runs` steps after
`warmup`, the two paths alternating, HIP events around the step; the host wall clock of the same steps; kernel launches, device-to-host
copy records and blocking runtime calls from a torch.profiler trace of one extra step.  Each path draws its own dropout masks while it is
timed.  Then, with masks fixed for both paths, e_chain and e_fused of every compared tensor against the float64 definitions
(second_stage.roi_mlp_train_reference, roi_loss_reference) - the errors of tests/test_roi_train_gpu.py, relative to max|ref|."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from center_predict_bench import counts_of, one_call  # noqa: E402
from roi_train_util import draw_masks, errors, make_case, make_train_head, run_step  # noqa: E402
from sparse2dense_amd import _lib, second_stage as S  # noqa: E402

CIN, WIDTHS, PER_SAMPLE = 2560, ((256, 256), (256, 256), (256, 256)), 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_train_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("roi_train_bench: no GPU - nothing is measured without one")
    head = make_train_head(CIN, *WIDTHS).cuda()
    params = list(head.parameters())
    lines = [f"# RoI head training step (MLP forward + RoI losses + backward), kernels of csrc/roi_mlp_train.hip vs the torch chain of the same commit: "
             f"median (min) of {args.runs} steps after {args.warmup} warm-ups, paths alternating, HIP events around the step; device "
             f"{torch.cuda.get_device_name(0)}; {CIN} -> 256 -> 256 -> 2 x (256 -> 256 -> 1 | 7), DP_RATIO 0.3, R = B x {PER_SAMPLE}"]
    plan = _lib.RoiMlpPlan()
    _lib.check(_lib.load().s2d_roi_mlp_plan_make(CIN, 2, 256, 256, 2, 256, 256, 2, 256, 256, 1, 7, ctypes.byref(plan)))
    fwd, bwd = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().s2d_roi_mlp_train_launches(ctypes.byref(plan), ctypes.byref(fwd), ctypes.byref(bwd)))
    lines.append(f"launch plan of the fused path: weight pack 1 (the weights moved since the last step) + mask draw 1 + MLP forward {fwd.value} + "
                 f"num_batches_tracked 1 + loss 1 | loss backward 1 + MLP backward {bwd.value} = {fwd.value + bwd.value + 5} of this project's launches; "
                 f"the profiler's count below adds torch's own (label / mask casts, the sum of the two losses and its backward, .item())")
    for batch in (1, 4):
        rows = batch * PER_SAMPLE
        case = {k: v.cuda() for k, v in make_case(CIN, rows, batch).items()}
        case["labels"] = case["labels"].clamp(min=0)   # roi_iou labels: no ignored rows (torch's BCE asserts on a label of -1)

        def step(fused):
            for p in params:
                p.grad = None
            x = case["x"].view(batch, PER_SAMPLE, CIN)
            if fused:
                cls, reg = S.roi_mlp_train_fused(head, x)
            else:   # RoIHead.forward's torch chain
                shared = head.shared_fc_layer(x.reshape(-1, 1, CIN).permute(0, 2, 1).contiguous())
                cls = head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
                reg = head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
            head.forward_ret_dict = dict(rcnn_cls=cls, rcnn_reg=reg, rcnn_cls_labels=case["labels"].view(batch, -1),
                                         reg_valid_mask=case["fg"].view(batch, -1), gt_of_rois=case["target"].view(batch, PER_SAMPLE, -1), fused_training=fused)
            total, tb = head.get_loss()
            total.backward()
            return tb["rcnn_loss"]
        paths = {"fused": lambda: step(True), "torch": lambda: step(False)}
        for fn in paths.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ev, wall = {k: [] for k in paths}, {k: [] for k in paths}
        for _ in range(args.runs):
            for k, fn in paths.items():
                e, w, _ = one_call(fn)
                ev[k].append(e)
                wall[k].append(w)
        try:
            cnt = {k: counts_of(fn) for k, fn in paths.items()}
            cnt_text = {k: f"{v[0]} launches, {v[1]} device-to-host copy records, {sum(v[2].values())} blocking runtime calls "
                           f"({', '.join(f'{n} x {c}' for n, c in sorted(v[2].items())) or 'none'})" for k, v in cnt.items()}
        except Exception as exc:   # the counts are a side figure: the timing above stands without them
            cnt_text = {k: f"launch count not taken ({type(exc).__name__})" for k in paths}
        lines.append(f"B = {batch}, R = {rows}:")
        for k in paths:
            lines.append(f"    {k:6s} {statistics.median(ev[k]):8.3f} ms ({min(ev[k]):.3f})   host wall {statistics.median(wall[k]):8.3f} ms   {cnt_text[k]}")
        ratio = statistics.median(ev["torch"]) / statistics.median(ev["fused"])
        lines.append(f"    torch / fused = x{ratio:.2f} device, x{statistics.median(wall['torch']) / statistics.median(wall['fused']):.2f} host wall"
                     + ("" if ratio >= 1 else "   (fused path SLOWER on this run)"))
        # the same masks for the definition, the chain and the kernels
        for p in params:
            p.grad = None
        head.forward_ret_dict = None
        host = {k: v.cpu() for k, v in case.items()}
        masks = draw_masks(head, rows, 31 + batch)
        ref, chain, got = (run_step(head, host, masks, how) for how in ("ref", "chain", "fused"))
        rel = lambda key, l=None: tuple(errors((ref if l is None else ref["layers"][l])[key], (r if l is None else r["layers"][l])[key])[0] /
                                        errors((ref if l is None else ref["layers"][l])[key], (r if l is None else r["layers"][l])[key])[1] for r in (chain, got))
        rowsf = [("rcnn_cls | rcnn_reg", rel("out")), ("loss_cls", rel("loss_cls")), ("loss_reg", rel("loss_reg"))]
        for l, layer in enumerate(ref["layers"]):
            rowsf += [(f"layer {l} d{key}" if key not in ("mean", "var") else f"layer {l} running {key}", rel(key, l)) for key in layer if key != "tracked"]
        worst = max(rowsf, key=lambda r: r[1][1] / (4 * r[1][0] + 1e-7))
        lines.append(f"    errors against the float64 definitions with the same masks, relative to max|ref| (e_chain, e_fused), {len(rowsf)} tensors; "
                     f"closest to the tests' bound 4 e_chain + 1e-7: {worst[0]} ({worst[1][0]:.3e}, {worst[1][1]:.3e})")
        lines += [f"        {name:24s} e_chain {c:.3e}   e_fused {f:.3e}" for name, (c, f) in rowsf]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
