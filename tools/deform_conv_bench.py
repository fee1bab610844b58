#!/usr/bin/env python
"""Deformable convolution v1: the three kernels of csrc/deform_conv.hip beside the pure-torch composite (sparse2dense_amd.dcn.
deform_conv_composite, fp32) on the same device in the same process, and beside their HBM bound.

    python tools/deform_conv_bench.py [--batch 4] [--size 180] [--runs 20] [--warmup 5] > profiles/deform_conv_bench.txt

B x 64 x size x size (the nuScenes 0.075 m head: 64 -> 64, 3x3, padding 1, 4 deformable groups), offsets uniform in +-`--range` pixels,
bf16 offsets (what conv_offset produces under autocast); HIP events, median of `runs` timed runs after `warmup`.
  (i)   forward (1 kernel, fused ReLU)                      vs  composite forward + relu
  (ii)  data backward (zero-fill + kernel + bf16 store)     vs  autograd of the composite w.r.t. input and offsets
  (iii) weight backward (kernel + reduce)                   vs  autograd of the composite w.r.t. the weight
  (iv)  DCNSepHead forward + backward (2 classes, nuScenes common_heads) under bf16 autocast: kernels vs composite (dcn.ENABLED = False)
HBM bound: the bytes every implementation must move - x + offsets + y (forward), x + offsets + y + dY + dX + d_offset (data backward),
x + offsets + y + dY (weight backward) - at --tbps (8 TB/s peak)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sparse2dense_amd import dcn, heads  # noqa: E402


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


def line(tag, hip, base, bound_bytes, tbps, note=""):
    bound = bound_bytes / (tbps * 1e12) * 1e3
    print(f"{tag:24s} HIP {hip[0]:8.3f} ms ({hip[1]:.3f})   composite {base[0]:8.3f} ms ({base[1]:.3f})   x{base[0] / hip[0]:.1f}   "
          f"HBM bound {bound:.3f} ms ({bound_bytes / 1e6:.0f} MB): {100 * bound / hip[0]:.0f} % of it{note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=180)
    ap.add_argument("--range", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tbps", type=float, default=8.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, c, s = args.batch, 64, args.size
    geo = (c, 3, 3, 1, 1, 1, 4)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, c, s, s, generator=g).to(dev)
    off = ((torch.rand(n, 72, s, s, generator=g) * 2 - 1) * args.range).to(dev)
    wt = (torch.randn(c, c, 3, 3, generator=g) / 24).to(dev)
    dy = torch.randn(n, c, s, s, generator=g).to(dev)
    xb = x.bfloat16().contiguous(memory_format=torch.channels_last)
    ob = off.bfloat16().contiguous(memory_format=torch.channels_last)
    dyb = dy.bfloat16().contiguous(memory_format=torch.channels_last)
    print(f"# deformable conv micro-benchmark: {n} x {c} x {s} x {s}, 64 -> 64, 3x3, dg 4, offsets in +-{args.range} px (bf16), median (min) of "
          f"{args.runs} runs after {args.warmup} warm-ups, HIP events; device {torch.cuda.get_device_name(0)}")
    px = n * s * s
    b_x, b_o, b_y = px * c * 2, px * 72 * 2, px * c * 2

    pf, pb = dcn.pack_weights(wt)
    y = dcn.deform_conv_fwd_hip(xb, ob, pf, *geo, True)
    xr, orr, wr = (t.clone().requires_grad_(True) for t in (x.bfloat16().float(), ob.float().contiguous(), wt.bfloat16().float()))
    comp = lambda: torch.relu(dcn.deform_conv_composite(xr, orr, wr, 1, 1, 1, 1, 4))
    yr = comp()
    err = float((y.float() - yr.detach()).abs().max() / yr.detach().abs().max())
    hip = timed(lambda: dcn.deform_conv_fwd_hip(xb, ob, pf, *geo, True, y=y), args.runs, args.warmup)
    with torch.no_grad():
        base = timed(comp, args.runs, args.warmup)
    line("(i)   forward", hip, base, b_x + b_o + b_y, args.tbps, f"; max difference / max {err:.1e}")

    dx, doff = dcn.deform_conv_bwd_data_hip(xb, ob, dyb, y, pb, *geo)
    hip = timed(lambda: dcn.deform_conv_bwd_data_hip(xb, ob, dyb, y, pb, *geo, dx=dx, d_offset=doff), args.runs, args.warmup)
    dyf = dyb.float()
    base = timed(lambda: torch.autograd.grad((yr * dyf).sum(), (xr, orr), retain_graph=True), args.runs, args.warmup)
    line("(ii)  data backward", hip, base, 2 * b_x + 2 * b_o + 2 * b_y, args.tbps, " (composite: backward only, graph kept)")

    hip = timed(lambda: dcn.deform_conv_wgrad_hip(xb, ob, dyb, y, *geo), args.runs, args.warmup)
    base = timed(lambda: torch.autograd.grad((yr * dyf).sum(), (wr,), retain_graph=True), args.runs, args.warmup)
    line("(iii) weight backward", hip, base, b_x + b_o + 2 * b_y, args.tbps, " (composite: backward only, graph kept)")
    del yr, xr, orr, wr

    common = {"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)}
    torch.manual_seed(0)
    head = heads.DCNSepHead(64, 2, common, bn=True, final_kernel=3).to(dev).train()
    for fa in (head.feature_adapt_cls, head.feature_adapt_reg):
        torch.nn.init.normal_(fa.conv_offset.weight, std=0.1)
    for m in head.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(memory_format=torch.channels_last)
    xh = xb.clone().requires_grad_(True)

    def step():
        for p in head.parameters():
            p.grad = None
        xh.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = head(xh)
        sum(v.float().sum() for v in out.values()).backward()
    hip = timed(step, args.runs, args.warmup)
    dcn.ENABLED = False
    try:
        base = timed(step, max(3, args.runs // 4), 2)
    finally:
        dcn.ENABLED = True
    print(f"(iv)  DCNSepHead fwd+bwd   HIP {hip[0]:8.3f} ms ({hip[1]:.3f})   composite {base[0]:8.3f} ms ({base[1]:.3f})   x{base[0] / hip[0]:.1f}   "
          f"(two deformable convs + 7 branches of conv3x3 / batch norm / small conv; six such heads per nuScenes frame)")


if __name__ == "__main__":
    main()
