#!/usr/bin/env python
"""The second stage of TwoStageDetector: the device path (csrc/roi_head.hip) beside the torch chain it replaces, in one process on the
same inputs.

    python tools/two_stage_bench.py [--runs 20] [--warmup 5] [--out profiles/two_stage_bench.txt]

Shape: B = 4, a 188 x 188 x 512 channels_last bf16 neck map, 300-500 proposals per sample, 100 ground-truth boxes per sample (the
two-stage Waymo configuration, waymo_configs.two_stage_voxelnet).  The first stage is replaced by a stand-in that hands the same
proposals, map and loss dictionary to every call and launches nothing, so the HIP events around the detector call time the second
stage only: pack / BEV features / (match, sampling, targets) / RoI MLP / (refine or the two RoI losses).  Per row: median (min) of
`runs` calls after `warmup`, the two paths alternating; the host wall clock of the same calls; kernel launches, device-to-host copy
records and blocking runtime calls per call from a torch.profiler trace of one extra call; whether both paths return the same numbers.
Training runs under a fixed seed (numpy, torch), set before every call, so both paths sample the same RoIs.  The inference row has
three columns: the device path with the fused RoI MLP (csrc/roi_mlp.hip), the device path with the torch MLP (S2D_ROI_MLP=0: the row
of the commit before the fused kernel) and the torch chain.  Then the feature kernel alone against the bytes it has to move (four 1 KiB
taps per sample point in, one fp32 row out), and the RoI MLP alone on the inference row's [B * 500, 2560] features: the fused launch
against the head's three nn.Sequential's, with their launch counts and their largest absolute errors against the float64 definition
(second_stage.roi_mlp_reference) - e_chain and e_fused of tests/test_roi_mlp_gpu.py - and the fused launch at other row counts."""
import argparse
import copy
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from center_predict_bench import counts_of, one_call  # noqa: E402
from sparse2dense_amd import registry, second_stage as S, waymo_configs  # noqa: E402

B, C, HW, GT = 4, 512, 188, 100


def inputs(seed=0):
    """(proposals per sample, neck map, gt_boxes_and_cls): the ground truth is spread over the range, the proposals are jittered copies
    of it (IoUs from ~0 to ~0.9, so the sampler finds foreground, hard and easy background) plus clutter"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    n = lambda *s: torch.randn(*s, generator=g)
    gt = torch.zeros(B, 500, 10)
    preds = []
    counts = [300, 500, 420, 360]
    for b in range(B):
        box = torch.cat([(r(GT, 2) - 0.5) * 140, n(GT, 1) * 0.5, r(GT, 1) * 1.5 + 1.5, r(GT, 1) * 3 + 3, r(GT, 1) * 0.5 + 1.4, (r(GT, 1) - 0.5) * 6.28], 1)
        gt[b, :GT, :7] = box
        gt[b, :GT, 9] = torch.randint(1, 4, (GT,), generator=g).float()
        k = counts[b]
        src = torch.randint(0, GT, (k,), generator=g)
        jitter = n(k, 7) * torch.tensor([0.4, 0.4, 0.1, 0.15, 0.3, 0.1, 0.1]) * (r(k, 1) * 2)
        prop = box[src] + jitter
        prop[k * 3 // 4:, :2] = (r(k - k * 3 // 4, 2) - 0.5) * 140   # clutter
        preds.append((prop, r(k), gt[b, src, 9].long() - 1))
    boxes, scores, labels = (torch.cat([p[i] for p in preds]).cuda() for i in range(3))
    sizes = [len(p[0]) for p in preds]
    preds = [dict(box3d_lidar=x, scores=s, label_preds=l, metadata=None) for x, s, l in zip(boxes.split(sizes), scores.split(sizes), labels.split(sizes))]
    bev = n(B, HW, HW, C).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)   # channels_last, as the bf16 neck leaves it
    return preds, bev, gt.cuda()


def agree(a, b, training):
    if training:
        return (torch.equal(a["rois"], b["rois"]) and torch.allclose(a["gt_of_rois"], b["gt_of_rois"], rtol=1e-4, atol=1e-4)
                and torch.allclose(a["roi_features"], b["roi_features"], rtol=1e-4, atol=1e-4)
                and torch.allclose(a["rcnn_cls_labels"], b["rcnn_cls_labels"], atol=1e-4) and abs(a["loss"] - b["loss"]) <= 1e-4 * abs(b["loss"]))
    return all(x["box3d_lidar"].shape == y["box3d_lidar"].shape and torch.equal(x["label_preds"], y["label_preds"])
               and torch.allclose(x["box3d_lidar"], y["box3d_lidar"], rtol=1e-4, atol=1e-4) and torch.allclose(x["scores"], y["scores"], rtol=1e-4, atol=1e-6)
               for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_stage_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("two_stage_bench: no GPU - nothing is measured without one")
    preds, bev, gt = inputs()
    cfg = waymo_configs.two_stage_voxelnet()
    det = registry.build_detector(cfg).cuda()   # (the first stage is built but never run: its forward is replaced below)
    zero = torch.zeros((), device="cuda")
    det.single_det.forward_two_stage = lambda example, return_loss=True, **kw: (
        (preds, bev, None, {"loss": [zero.clone()]}) if return_loss else (preds, bev, None, None, None, None))
    total = sum(len(p["scores"]) for p in preds)
    lines = [f"# TwoStageDetector second stage, device path vs torch chain: median (min) of {args.runs} calls after {args.warmup} warm-ups, paths "
             f"alternating, HIP events around the call (first stage replaced by a stand-in that launches nothing); device "
             f"{torch.cuda.get_device_name(0)}; B = {B}, {HW} x {HW} x {C} channels_last bf16 map, {total} proposals "
             f"({', '.join(str(len(p['scores'])) for p in preds)}), {GT} ground-truth boxes per sample"]

    def call(path, training):
        os.environ["S2D_ROI_DEVICE"] = "0" if path == "torch" else "1"
        os.environ["S2D_ROI_MLP"] = "1" if path == "fused" else "0"
        if training:
            np.random.seed(7); torch.manual_seed(7)
            out = det({"gt_boxes_and_cls": gt}, return_loss=True)
            ret = dict(det.roi_head.forward_ret_dict)
            ret["loss"] = float(out["loss"][0])
            return ret
        with torch.no_grad():
            return det({}, return_loss=False)

    for title, training in (("inference (eval, no_grad): features of all proposals, RoI MLP, refine", False),
                            ("training forward + RoI losses (fixed seed): match, sampling, targets, features of the 128 sampled RoIs per sample, RoI MLP", True)):
        det.train(training)
        names = ("device", "torch") if training else ("fused", "device", "torch")   # (the training branch keeps the torch MLP)
        paths = {k: (lambda k=k: call(k, training)) for k in names}
        before, mlp_before = dict(det.roi_paths), dict(det.roi_head.mlp_paths)
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
        n = args.warmup + args.runs
        assert det.roi_paths["device"] - before["device"] == n * (len(names) - 1) and det.roi_paths["torch"] - before["torch"] == n, det.roi_paths
        assert det.roi_head.mlp_paths["fused"] - mlp_before["fused"] == (0 if training else n), det.roi_head.mlp_paths
        try:
            cnt = {k: counts_of(fn) for k, fn in paths.items()}
            cnt_text = {k: f"{v[0]} launches, {v[1]} device-to-host copy records, {sum(v[2].values())} blocking runtime calls "
                           f"({', '.join(f'{n} x {c}' for n, c in sorted(v[2].items())) or 'none'})" for k, v in cnt.items()}
        except Exception as exc:   # the counts are a side figure: the timing above stands without them
            cnt_text = {k: f"launch count not taken ({type(exc).__name__})" for k in paths}
        lines.append(f"{title}: outputs agree: {all(agree(out[k], out['torch'], training) for k in names[:-1])}")
        for k in paths:
            lines.append(f"    {k:6s} {statistics.median(ev[k]):8.3f} ms ({min(ev[k]):.3f})   host wall {statistics.median(wall[k]):8.3f} ms   {cnt_text[k]}")
        ratio = statistics.median(ev["torch"]) / statistics.median(ev["device"])
        lines.append(f"    torch / device = x{ratio:.2f}" + ("" if ratio >= 1 else "   (device path SLOWER on this run)"))
        if not training:
            ratio = statistics.median(ev["device"]) / statistics.median(ev["fused"])
            lines.append(f"    device / fused = x{ratio:.2f}, torch / fused = x{statistics.median(ev['torch']) / statistics.median(ev['fused']):.2f}"
                         + ("" if ratio >= 1 else "   (fused MLP SLOWER on this run)"))

    # the feature kernel alone: 4 taps of C bf16 per sample point in, C fp32 per sample point out
    boxes = torch.cat([p["box3d_lidar"] for p in preds])
    ext = det.second_stage[0]
    for what, slots in (("all proposals (inference)", 500), ("128 sampled per sample (training)", 128)):
        row = np.full((B, slots), -1, np.int32)
        off = 0
        for b, p in enumerate(preds):
            k = min(len(p["scores"]), slots)
            row[b, :k] = off + np.arange(k)
            off += len(p["scores"])
        row_d = torch.from_numpy(row).cuda()
        fn = lambda: S.roi_bev_features(bev, boxes, row_d, ext.pc_start, ext.voxel_size, ext.out_stride, 5)
        for _ in range(args.warmup):
            fn()
        t = [one_call(fn)[0] for _ in range(args.runs)]
        pts = int((row >= 0).sum()) * 5
        moved = pts * 4 * C * 2 + B * slots * 5 * C * 4
        lines.append(f"roi_bev_features alone, {what}: {pts} sample points, {moved / 1e6:.2f} MB to move (taps in, fp32 rows out; the chain's fp32 NHWC "
                     f"copy alone writes {B * HW * HW * C * 4 / 1e6:.0f} MB), median {statistics.median(t) * 1e3:.1f} us (min {min(t) * 1e3:.1f}) "
                     f"= {moved / statistics.median(t) / 1e6:.1f} GB/s including the launch")
    # the RoI MLP alone on the inference row's features: one fused launch against the three nn.Sequential's
    det.eval()
    os.environ["S2D_ROI_MLP"] = "1"
    head = det.roi_head
    row = np.full((B, 500), -1, np.int32)
    off = 0
    for b, p in enumerate(preds):
        row[b, :len(p["scores"])] = off + np.arange(len(p["scores"]))
        off += len(p["scores"])
    feats = S.roi_bev_features(bev, boxes, torch.from_numpy(row).cuda(), ext.pc_start, ext.voxel_size, ext.out_stride, 5).view(B * 500, 5 * C)

    def torch_mlp():
        shared = head.shared_fc_layer(feats.reshape(-1, 1, feats.shape[-1]).permute(0, 2, 1).contiguous())
        return (head.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1), head.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1))
    with torch.no_grad():
        mlp = {"fused": lambda: S.roi_mlp_fused(head, feats), "torch": torch_mlp}
        for fn in mlp.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        t, res = {k: [] for k in mlp}, {}
        for _ in range(args.runs):
            for k, fn in mlp.items():
                e, _, res[k] = one_call(fn)
                t[k].append(e)
        try:
            launches = {k: str(counts_of(fn)[0]) for k, fn in mlp.items()}
        except Exception as exc:
            launches = {k: f"not counted ({type(exc).__name__})" for k in mlp}
        head.forward_ret_dict = None   # (the training row's graph tensors do not copy)
        ref = torch.cat(S.roi_mlp_reference(copy.deepcopy(head).double(), feats.double()), dim=1)
    err = {k: float((torch.cat(res[k], dim=1).double() - ref).abs().max()) for k in mlp}
    flop = 2 * feats.shape[0] * sum(l.cin * l.cout for l in head._mlp_cache["plan"].layer[:head._mlp_cache["plan"].num_layers])
    ratio = statistics.median(t["torch"]) / statistics.median(t["fused"])
    lines.append(f"RoI MLP alone, eval, {feats.shape[0]} x {feats.shape[1]} fp32 features -> 256 -> 256 -> 2 x (256 -> 256 -> 1 | 7), {flop / 1e9:.2f} GFLOP: "
                 f"fused {statistics.median(t['fused']) * 1e3:.1f} us (min {min(t['fused']) * 1e3:.1f}), {launches['fused']} launches, "
                 f"{flop / statistics.median(t['fused']) / 1e9:.1f} TFLOP/s including the launch; torch {statistics.median(t['torch']) * 1e3:.1f} us "
                 f"(min {min(t['torch']) * 1e3:.1f}), {launches['torch']} launches; torch / fused = x{ratio:.2f}"
                 + ("" if ratio >= 1 else "   (fused MLP SLOWER on this run)"))
    lines.append(f"    largest absolute error against the float64 definition (max|out| {float(ref.abs().max()):.3f}): e_chain (torch fp32 MLP) {err['torch']:.3e}, "
                 f"e_fused {err['fused']:.3e}; bound of the tests 4 * e_chain + 1e-7 * max|out| = {4 * err['torch'] + 1e-7 * float(ref.abs().max()):.3e}")
    # the fused launch at other row counts (16 rows = one workgroup; 4 096 = one per CU): where it stops being latency-bound
    scale = []
    with torch.no_grad():
        for rows in (16, 4096, 8000, 32000):
            x = torch.randn(rows, 5 * C, device="cuda")
            fn = lambda: S.roi_mlp_fused(head, x)
            for _ in range(args.warmup):
                fn()
            scale.append(f"{rows} rows {statistics.median([one_call(fn)[0] for _ in range(args.runs)]) * 1e3:.1f} us")
    lines.append(f"    fused launch alone by row count (random features, median of {args.runs}): {', '.join(scale)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
