#!/usr/bin/env python
"""Feature loss of the PointPillars distillation branch (heads.pooled_distill_loss): the fused path (csrc/pillar_distill.hip) beside the torch
restatement it replaces (S2D_PILLAR_DISTILL_FUSED=0), in one process on the same inputs.

    python tools/pillar_distill_bench.py [--runs 20] [--warmup 5] [--batch 4] [--out profiles/pillar_distill_bench.txt]

Row 1: the loss alone at B x 64 x 468 x 468 in the benchmarked dtypes and layouts - student maps bf16 channels_last, teacher canvases fp32
planar with ~15 % (dense cloud) and ~2 % (object-only cloud) occupied cells, the densities of a pillar scatter.  HIP events around the
forward, around the backward and around both, median (min) of `runs` calls after `warmup`, the two paths alternating; kernel launches per
forward + backward from a torch.profiler trace of one extra call (tools/center_predict_bench.py: counts_of); loss and gradients compared.
For the fused path the achieved share of the HBM peak BASELINE.md names (8 TB/s), from the compulsory bytes: four maps read forward, four
read and two student gradients written backward.
Row 2: one whole pillar distillation step (train_step.distill_loss + backward_and_clip on a resident example: teacher forward, student
forward, every loss, backward, clip) at the same batch, bf16 channels_last models as bench.py builds them, both paths alternating."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from center_predict_bench import counts_of  # noqa: E402
from sparse2dense_amd import heads  # noqa: E402

C, H, W = 64, 468, 468
HBM_PEAK = 8.0e12   # BASELINE.md "Peaks to divide by"
ENV = "S2D_PILLAR_DISTILL_FUSED"


def set_path(fused):
    if fused:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = "0"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def med(v):
    return f"{statistics.median(v):8.3f} ms ({min(v):.3f})"


def loss_rows(args, lines):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(5100)
    shape = (args.batch, C, H, W)
    student = lambda: torch.randn(shape, generator=g, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    canvas = lambda occ: torch.relu(torch.randn(shape, generator=g, device=dev)) * (torch.rand((args.batch, 1, H, W), generator=g, device=dev) < occ)
    sa, sb, da, db = student(), student(), canvas(0.15), canvas(0.02)
    occupied = [float((t != 0).any(1).float().mean()) for t in (da, db)]

    def call(fused):
        set_path(fused)
        t_f, loss = timed(lambda: heads.pooled_distill_loss(sa, da, sb, db))
        t_b, grads = timed(lambda: torch.autograd.grad(loss, [sa, sb]))
        return t_f, t_b, loss.detach(), grads

    def both(fused):
        set_path(fused)
        return torch.autograd.grad(heads.pooled_distill_loss(sa, da, sb, db), [sa, sb])

    paths = {"fused": True, "torch": False}
    for fused in paths.values():
        for _ in range(args.warmup):
            both(fused)
    torch.cuda.synchronize()
    tf, tb, tt, out = ({k: [] for k in paths} for _ in range(4))
    for _ in range(args.runs):
        for k, fused in paths.items():
            f, b, loss, grads = call(fused)
            tf[k].append(f)
            tb[k].append(b)
            out[k] = (loss, grads)
            tt[k].append(timed(lambda: both(fused))[0])
    rel = abs(float(out["fused"][0]) - float(out["torch"][0])) / abs(float(out["torch"][0]))
    gerr = max(float((a.float() - b.float()).abs().max() / b.float().abs().max()) for a, b in zip(out["fused"][1], out["torch"][1]))
    assert rel <= 1e-5 and gerr <= 6e-3, (rel, gerr)   # the bounds of tests/test_pillar_distill_gpu.py
    try:
        cnt = {k: f"{counts_of(lambda: both(fused))[0]} launches" for k, fused in paths.items()}
    except Exception as exc:   # the counts are a side figure: the timing above stands without them
        cnt = {k: f"launch count not taken ({type(exc).__name__})" for k in paths}
    n = args.batch * C * H * W
    bytes_f, bytes_b = n * (2 * 2 + 2 * 4), n * (2 * 2 + 2 * 4 + 2 * 2)
    lines.append(f"loss alone, B={args.batch} x {C} x {H} x {W}, student bf16 channels_last, teacher fp32 planar (occupied cells {occupied[0]:.3f} / "
                 f"{occupied[1]:.3f}): loss rel diff {rel:.2e}, gradient max diff / max {gerr:.2e}")
    for k in paths:
        lines.append(f"    {k:6s} forward {med(tf[k])}   backward {med(tb[k])}   forward + backward {med(tt[k])}   {cnt[k]}")
    f, b = statistics.median(tf["fused"]) * 1e-3, statistics.median(tb["fused"]) * 1e-3
    lines.append(f"    fused, compulsory bytes over the 8 TB/s HBM peak: forward {bytes_f / 1e6:.0f} MB -> {bytes_f / f / HBM_PEAK:.1%}, "
                 f"backward {bytes_b / 1e6:.0f} MB -> {bytes_b / b / HBM_PEAK:.1%}")
    ratio = statistics.median(tt["torch"]) / statistics.median(tt["fused"])
    lines.append(f"    torch / fused (forward + backward) = x{ratio:.2f}" + ("" if ratio >= 1 else "   (fused path SLOWER on this run)"))


def step_rows(args, lines):
    from sparse2dense_amd import waymo_configs
    from sparse2dense_amd.data import SyntheticPillarFrames
    from sparse2dense_amd.registry import build_detector
    from sparse2dense_amd.train_step import backward_and_clip, distill_loss
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    student = build_detector(waymo_configs.pillar_s2d_student())
    teacher = build_detector(waymo_configs.centerpoint_pillar())
    for p in teacher.parameters():
        p.requires_grad = False
    for m in (student, teacher):
        m.dense_dtype = torch.bfloat16
        m.use_channels_last()
    student, teacher = student.to(dev).train(), teacher.to(dev).eval()
    params = [p for p in student.parameters() if p.requires_grad]
    ex = SyntheticPillarFrames(args.batch, n_points=args.points, distill=True, device=dev).example()

    def step(fused):
        set_path(fused)
        loss, losses = distill_loss(teacher, student, ex)
        norm = backward_and_clip(loss, params, 35.0)
        return loss.detach(), norm, losses["sparse2dense_loss"][0]

    paths = {"fused": True, "torch": False}
    for fused in paths.values():
        for _ in range(args.warmup):
            step(fused)
    torch.cuda.synchronize()
    ts, out = {k: [] for k in paths}, {}
    for _ in range(args.runs):
        for k, fused in paths.items():
            t, out[k] = timed(lambda: step(fused))
            ts[k].append(t)
    vals = {k: [float(x) for x in v] for k, v in out.items()}
    lines.append(f"whole pillar distillation step, B={args.batch}, {args.points} points per frame, bf16 channels_last models, resident example "
                 f"(teacher forward + student forward + losses + backward + clip): loss / gradient norm / feature loss fused {vals['fused']}, "
                 f"torch {vals['torch']}")
    for k in paths:
        lines.append(f"    {k:6s} {med(ts[k])}")
    ratio = statistics.median(ts["torch"]) / statistics.median(ts["fused"])
    lines.append(f"    torch / fused = x{ratio:.2f}" + ("" if ratio >= 1 else "   (fused path SLOWER on this run)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--no-step", action="store_true", help="the loss rows only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pillar_distill_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pillar_distill_bench: no GPU - nothing is measured without one")
    lines = [f"# heads.pooled_distill_loss, fused kernels vs torch restatement ({ENV}=0): median (min) of {args.runs} calls after {args.warmup} "
             f"warm-ups, paths alternating, HIP events around the call; device {torch.cuda.get_device_name(0)}"]
    loss_rows(args, lines)
    if not args.no_step:
        step_rows(args, lines)
    os.environ.pop(ENV, None)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
