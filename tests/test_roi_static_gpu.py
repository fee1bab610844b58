"""The static second stage on the device (s2d_roi_pack_static, s2d_roi_refine_static through second_stage.StaticRoIPlan and
TwoStageDetector.forward_static): padded rows with device counts, 4 launches, no host read, capturable behind the static predict.

Bit for bit against the existing device path (`pack_rois`, `refine_rois`, `TwoStageDetector._forward_device` behind `CenterHead.predict`):
both sides copy the same rows, sample the same boxes on the same map, run the same MLP kernel, whose result for a row depends on that row
alone, and the same refinement device function, so no margin is needed and none is asserted.  The refinement is also compared with the
reference's recorded outputs (tests/golden/second_stage.npz) under the tolerance of test_roi_device_gpu.py, and a repacked MLP with its
float64 definition under the rule of test_roi_mlp_gpu.py: e_fused <= 4 e_chain + 1e-7 max|out|.

The padding of every input is a trap: rows behind counts[b] hold NaN boxes, score 1.0 and a valid label; the padding rows of rcnn_cls and
rcnn_reg hold NaN.  The kernels' outputs lie inside sentinel-filled buffers, and the sentinels are checked."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from golden_util import fill_params, seeded
from roi_static_util import TRAP_LABEL, FixedMapsFirstStage, clamp_counts, pack_static_host, plant_traps, trapped_rows
from sparse2dense_amd import _lib, center_predict, registry, second_stage as S
from test_roi_mlp_cpu import make_head, module_mlp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64   # sentinel elements on either side of every output (a multiple of 16 bytes: the outputs keep their alignment)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """an output of `shape` inside a sentinel-filled buffer"""

    def __init__(self, shape, dtype):
        self.sentinel = -77 if dtype in (torch.int32, torch.int64) else -7.75
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), self.sentinel, dtype=dtype, device=DEV)
        self.out = self.buf[GUARD:GUARD + self.n].view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.n:] == self.sentinel).all())


# ---- pack_static ------------------------------------------------------------------------------------------------------------------------
def _pack_static(boxes, scores, labels, counts, cap):
    b, det_cap = boxes.shape[:2]
    outs = [Guarded((b, cap, 7), torch.float32), Guarded((b, cap), torch.float32), Guarded((b, cap), torch.int64), Guarded((b, cap), torch.int32),
            Guarded((b,), torch.int32)]
    _lib.check(_lib.load().s2d_roi_pack_static(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), counts.data_ptr(), b, det_cap, cap,
                                               *[o.out.data_ptr() for o in outs], _stream()), "s2d_roi_pack_static")
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs)
    return [o.out for o in outs]


def _many_counts(b, det_cap, cap):
    """0, 1, cap, above cap, above det_cap and negative first, then seeded values around the two limits"""
    special = [0, 1, cap, cap + 3, det_cap + 5, -2, min(det_cap, cap), min(det_cap, cap) - 1]
    rng = np.random.RandomState(b * 1000 + det_cap)
    return (special + rng.randint(-3, max(det_cap, cap) + 6, size=max(b - len(special), 0)).tolist())[:b]


@pytest.mark.parametrize("det_cap,cap,counts", [
    (8, 16, [0]), (8, 16, [1]), (8, 16, [8]), (8, 16, [9]), (8, 16, [-3]),                    # det_cap < cap, B = 1
    (16, 16, [0, 16, 20]), (24, 16, [1, 16, 24]), (24, 16, [-1, 30, 17]), (8, 16, [16, 7, 40]),   # B = 3: det_cap ==, > and < cap
    (8, 16, None), (16, 16, None), (24, 16, None),                                              # B = 64
    (300, 260, [260, 300, 257, 3]),                                                             # a second block of slots
])
def test_pack_static_equals_pack_rois_on_the_rows_below_the_counts(det_cap, cap, counts):
    counts = _many_counts(64, det_cap, cap) if counts is None else counts
    b = len(counts)
    boxes, scores, labels = trapped_rows(b, det_cap, counts, 100 + det_cap)
    have = np.clip(counts, 0, det_cap)   # the rows each sample holds; pack_rois drops those behind cap
    offsets = [0] + np.cumsum(have).tolist()
    keep = torch.arange(det_cap)[None, :] < torch.from_numpy(have)[:, None]
    assert not torch.isnan(boxes[keep]).any() and (b * det_cap == int(keep.sum()) or torch.isnan(boxes[~keep]).all())
    want = S.pack_rois(boxes[keep].cuda(), scores[keep].cuda(), labels[keep].cuda(), offsets, cap)
    rois, roi_scores, roi_labels, row, out_counts = _pack_static(boxes.cuda(), scores.cuda(), labels.cuda(),
                                                                 torch.tensor(counts, dtype=torch.int32, device=DEV), cap)
    assert torch.equal(rois, want[0]) and torch.equal(roi_scores, want[1]) and torch.equal(roi_labels, want[2])
    host = pack_static_host(boxes.numpy(), scores.numpy(), labels.numpy(), counts, cap)
    n = clamp_counts(counts, det_cap, cap)
    assert out_counts.cpu().numpy().tolist() == n.tolist() == host[4].tolist()
    assert np.array_equal(row.cpu().numpy(), host[3])
    for s, k in enumerate(n):   # the zero padding
        assert not rois[s, k:].any() and not roi_scores[s, k:].any() and not roi_labels[s, k:].any() and bool((row[s, k:] == -1).all())
        assert bool((roi_labels[s, :k] >= 1).all())


# ---- refine_static ----------------------------------------------------------------------------------------------------------------------
def _refine_static(rois, roi_scores, roi_labels, cls, reg, counts):
    b, cap = roi_labels.shape
    outs = [Guarded((b, cap, 7), torch.float32), Guarded((b, cap), torch.float32), Guarded((b, cap), torch.int64)]
    _lib.check(_lib.load().s2d_roi_refine_static(rois.data_ptr(), roi_scores.data_ptr(), roi_labels.data_ptr(), cls.data_ptr(), reg.data_ptr(),
                                                 counts.data_ptr(), b, cap, *[o.out.data_ptr() for o in outs], _stream()), "s2d_roi_refine_static")
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs)
    return [o.out for o in outs]


@pytest.mark.parametrize("cap,counts", [(16, [0]), (16, [16]), (16, [0, 1, 16]), (32, [31, 5, 32]), (16, None), (260, [260, 3, 257])])
def test_refine_static_equals_refine_rois_below_the_counts_and_writes_the_padding(cap, counts):
    counts = _many_counts(64, cap, cap) if counts is None else counts
    n = clamp_counts(counts, cap, cap)
    b = len(counts)
    rois = torch.cat([seeded((b, cap, 2), 61, 5.0), seeded((b, cap, 1), 62), seeded((b, cap, 3), 63).abs() + 0.5, seeded((b, cap, 1), 64, 2.0)], 2).cuda()
    roi_scores, roi_labels = seeded((b, cap), 65).abs().clamp(max=1.0).cuda(), (1 + torch.arange(b * cap).view(b, cap) % 3).cuda()
    cls, reg = seeded((b * cap, 1), 66, 2.0).cuda(), seeded((b * cap, 7), 67, 0.3).cuda()
    want = S.refine_rois(rois, roi_scores, roi_labels, cls, reg)
    pad = (torch.arange(cap)[None, :] >= torch.from_numpy(n.astype(np.int64))[:, None]).cuda()
    cls[pad.view(-1)], reg[pad.view(-1)] = float("nan"), float("nan")   # the MLP's values for the padding never arrive
    boxes, scores, labels = _refine_static(rois, roi_scores, roi_labels, cls, reg, torch.tensor(counts, dtype=torch.int32, device=DEV))
    for s, k in enumerate(n):
        assert torch.equal(boxes[s, :k], want[0][s, :k]) and torch.equal(scores[s, :k], want[1][s, :k]) and torch.equal(labels[s, :k], want[2][s, :k])
        assert not boxes[s, k:].any() and not scores[s, k:].any() and bool((labels[s, k:] == -1).all())
    assert not torch.isnan(boxes).any() and not torch.isnan(scores).any()


def test_refine_static_matches_the_reference_boxes_and_post_process(golden_dir):
    """the set-up and the tolerances of test_roi_device_gpu.test_refine_matches_the_reference_boxes_and_post_process: 40 RoIs in 50 slots"""
    g = np.load(os.path.join(golden_dir, "second_stage.npz"))
    roi = registry.build(dict(type="RoIHead", input_channels=24 * 5, code_size=7,
                              model_cfg=dict(CLASS_AGNOSTIC=True, SHARED_FC=[64, 64], CLS_FC=[64, 64], REG_FC=[64, 64], DP_RATIO=0.3)),
                         registry.ROI_HEAD)
    fill_params(roi).eval()
    rois = torch.zeros(1, 50, 7); rois[0, :40] = torch.from_numpy(g["boxes"])
    feats = torch.zeros(1, 50, 120); feats[0, :40] = torch.from_numpy(g["bev_features"])
    scores = torch.zeros(1, 50); scores[0, :40] = seeded((40,), 31).abs().clamp(max=1.0)
    labels = torch.zeros(1, 50, dtype=torch.long); labels[0, :40] = 1 + torch.arange(40) % 3
    with torch.no_grad():
        chain = roi(dict(rois=rois.clone(), roi_features=feats.clone(), roi_scores=scores, roi_labels=labels), training=False)
        ref = S.TwoStageDetector.post_process(None, chain)[0]
        cls, reg = S.roi_mlp_fused(copy.deepcopy(roi).cuda(), feats.cuda())
    cls[40:], reg[40:] = float("nan"), float("nan")
    box, score, label = _refine_static(rois.cuda(), scores.cuda(), labels.cuda(), cls, reg, torch.tensor([40], dtype=torch.int32, device=DEV))
    np.testing.assert_allclose(box[:, :40].cpu().numpy(), g["batch_box_preds"][:, :40], rtol=1e-4, atol=1e-5)    # the reference
    np.testing.assert_allclose(cls[:40].view(1, 40, 1).cpu().numpy(), g["batch_cls_preds"][:, :40], rtol=1e-4, atol=1e-5)
    assert box.shape == (1, 50, 7) and score.shape == (1, 50) and label.dtype == torch.int64
    np.testing.assert_allclose(box[0, :40].cpu().numpy(), ref["box3d_lidar"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(score[0, :40].cpu().numpy(), ref["scores"].numpy(), rtol=1e-4, atol=1e-5)
    assert torch.equal(label[0, :40].cpu(), ref["label_preds"]) and bool((label[0, 40:] == -1).all())
    assert not box[0, 40:].any() and not score[0, 40:].any() and float(ref["scores"].max()) > 0.1


# ---- the whole plan ---------------------------------------------------------------------------------------------------------------------
H = W = C = 16
CAP = 16
EXT = dict(pc_start=[-6.4, -6.4], voxel_size=[0.1, 0.1], out_stride=8)
TASKS = [dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])]
HEAD_CFG = dict(type="CenterHead", in_channels=C, tasks=TASKS, dataset="waymo", weight=2, code_weights=[1.0] * 8,
                common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)})
# a 16 x 16 map of 0.8 m cells; at most 32 candidates per sample, CAP kept
TEST_CFG = dict(post_center_limit_range=[-8.0, -8.0, -10.0, 8.0, 8.0, 10.0], score_threshold=0.1, pc_range=[-6.4, -6.4], out_size_factor=8,
                voxel_size=[0.1, 0.1], nms=dict(nms_pre_max_size=32, nms_post_max_size=CAP, nms_iou_threshold=0.7))
PEAKS = (0, 60, 7)   # per sample: no detection, more than CAP survive the NMS (exactly CAP are kept), a few


def _head_maps(frame, peaks=PEAKS):
    """seeded head maps of len(peaks) samples; the boxes are about 0.4 m wide on 0.8 m cells, so the NMS removes few"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import predict_tasks_util as P
    shift = frame % len(peaks)
    per = [P.seeded_task_maps(3, 7000 + 10 * frame + s, H, W, 1, False, vel=False, peaks=p, peak_logit=(-1.0, 2.0))
           for s, p in enumerate(peaks[shift:] + peaks[:shift])]
    maps = {k: torch.cat([m[k] for m in per]) for k in per[0]}
    maps["dim"] = maps["dim"] - 1.8
    return [{k: v.to(DEV) for k, v in maps.items()}]


def _bev(frame, layout, samples=len(PEAKS)):
    nhwc = seeded((samples, H, W, C), 300 + frame)
    if layout == "nchw_fp32":
        return nhwc.permute(0, 3, 1, 2).contiguous().to(DEV)
    return nhwc.to(torch.bfloat16).to(DEV).permute(0, 3, 1, 2)   # channels_last bf16


def _detector(num_point):
    det = registry.build_detector(dict(type="TwoStageDetector", first_stage_cfg=dict(type=FixedMapsFirstStage, bbox_head=HEAD_CFG), NMS_POST_MAXSIZE=CAP,
                                       num_point=num_point, second_stage_modules=[dict(type="BEVFeatureExtractor", **EXT)],
                                       roi_head=dict(type="RoIHead", input_channels=num_point * C, code_size=7,
                                                     model_cfg=dict(CLASS_AGNOSTIC=True, SHARED_FC=[32, 16], CLS_FC=[16], REG_FC=[32, 16], DP_RATIO=0.3))),
                                  test_cfg=TEST_CFG)
    det.roi_head = make_head(num_point * C, (32, 16), (16,), (32, 16), signed=True)
    return det.to(DEV).eval()


def _eager(det, maps, bev):
    """`forward(return_loss=False)`: CenterHead.predict + TwoStageDetector._forward_device"""
    det.single_det.maps, det.single_det.bev = maps, bev
    before = det.roi_paths["device"]
    with torch.no_grad():
        out = det({}, return_loss=False)
    assert det.roi_paths["device"] == before + 1 and det.roi_head.mlp_paths["torch"] == 0
    return out


def _static_plans(det, maps, bev):
    sp = center_predict.StaticPredictPlan(TEST_CFG, det.bbox_head.num_classes, maps[0]["hm"].shape[0], H, W, False, maps[0]["hm"].device)
    assert sp.cap == CAP and sp.box_dim == 7
    with torch.no_grad():   # (the head's parameters require a gradient: outside no_grad the plan refuses, as roi_mlp_fused does)
        rp = S.StaticRoIPlan(det.roi_head, det.second_stage, det.num_point, sp.samples, sp.cap, det.NMS_POST_MAXSIZE, bev.shape[1], bev.dtype, bev.device)
    return sp, rp


def _assert_equals_eager(out, want, what):
    counts = out.counts.tolist()
    assert counts == [len(w["scores"]) for w in want], what
    for b, n in enumerate(counts):
        assert torch.equal(out.boxes[b, :n], want[b]["box3d_lidar"]) and torch.equal(out.scores[b, :n], want[b]["scores"]), (what, b)
        assert torch.equal(out.labels[b, :n], want[b]["label_preds"]), (what, b)
        assert not out.boxes[b, n:].any() and not out.scores[b, n:].any() and bool((out.labels[b, n:] == -1).all()), (what, b)
    return counts


@pytest.mark.parametrize("num_point", [1, 5])
@pytest.mark.parametrize("layout", ["nchw_fp32", "channels_last_bf16"])
def test_the_plan_equals_the_detector_on_the_device_path(num_point, layout):
    det = _detector(num_point)
    maps, bev = _head_maps(0), _bev(0, layout)
    assert bev.is_contiguous() == (layout == "nchw_fp32")
    want = _eager(det, maps, bev)
    sp, rp = _static_plans(det, maps, bev)
    with torch.no_grad():
        first = sp.run(maps)
        out = rp.run(first, bev)
    assert isinstance(out, center_predict.StaticDetections) and out.overflow is first.overflow and out.boxes.shape == (3, CAP, 7)
    counts = _assert_equals_eager(out, want, "plan")
    assert counts[0] == 0 and counts[1] == CAP and 0 < counts[2] < CAP   # no detection, exactly cap, a few
    rows = out.as_list(["m0", "m1", "m2"])
    assert [sorted(r) for r in rows] == [sorted(want[0])] * 3 and [r["metadata"] for r in rows] == ["m0", "m1", "m2"]
    # trap-filled padding: the same detections in buffers whose rows behind the counts hold NaN boxes, score 1.0 and a valid label
    kept = [t.clone() for t in (out.boxes, out.scores, out.labels, out.counts)]
    trap = center_predict.StaticDetections(first.boxes.clone(), first.scores.clone(), first.labels.clone(), first.counts.clone(), first.overflow)
    plant_traps(trap.boxes, trap.scores, trap.labels, counts)
    assert torch.isnan(trap.boxes[0]).all() and not torch.isnan(trap.boxes[1]).any() and int(trap.labels[2, -1]) == TRAP_LABEL
    with torch.no_grad():
        again = rp.run(trap, bev)
    assert again is out and all(torch.equal(a, b) for a, b in zip(kept, (again.boxes, again.scores, again.labels, again.counts)))   # two runs, bit-equal
    assert bool((rp.row[0] == -1).all()) and rp.row[1].tolist() == list(range(CAP, 2 * CAP)) and not torch.isnan(rp.feats).any()
    assert rp.repacks == 0


def test_run_neither_synchronises_nor_allocates_nor_repacks():
    det = _detector(5)
    maps, bev = _head_maps(1), _bev(1, "channels_last_bf16")
    sp, rp = _static_plans(det, maps, bev)
    with torch.no_grad():
        first = sp.run(maps)
        out = rp.run(first, bev)   # warm-up: the code objects are loaded
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in rp.buffers().items()}
        assert set(ptrs) == {"rois", "roi_scores", "roi_labels", "row", "counts", "feats", "rcnn_cls", "rcnn_reg", "boxes", "scores", "labels"}
        kept = [t.clone() for t in (out.boxes, out.scores, out.labels, out.counts)]
        before, repacks = torch.cuda.memory_stats()["allocation.all.allocated"], rp.repacks
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = rp.run(first, bev)
            again = rp.run(first, bev)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before and rp.repacks == repacks == 0
    assert again is out and {k: v.data_ptr() for k, v in rp.buffers().items()} == ptrs
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(kept, (out.boxes, out.scores, out.labels, out.counts))) and int(out.counts.sum()) > 0


def test_an_edited_weight_and_running_variance_are_repacked_before_the_launches():
    """the MLP outputs of the run behind the edit against the float64 definition on the NEW parameters under the rule of test_roi_mlp_gpu.py
    (e_fused <= 4 e_chain + 1e-7 max|out|, e_chain the torch fp32 modules' error on the same features); the refinement of those outputs is
    `refine_rois`' bit for bit"""
    det = _detector(5)
    head = det.roi_head
    maps, bev = _head_maps(2), _bev(2, "nchw_fp32")
    sp, rp = _static_plans(det, maps, bev)
    with torch.no_grad():
        first = sp.run(maps)
        old = [t.clone() for t in rp.run(first, bev)][:3]
        assert rp.repacks == 0
        head.shared_fc_layer[0].weight.add_(0.05)
        head.reg_layers[1].running_var.mul_(1.5)
        out = rp.run(first, bev)
        assert rp.repacks == 1
        rp.run(first, bev)
        assert rp.repacks == 1
        counts = out.counts.tolist()
        assert max(counts) == CAP
        ref = torch.cat(S.roi_mlp_reference(copy.deepcopy(head).double(), rp.feats.double()), dim=1)
        chain = torch.cat(module_mlp(head, rp.feats), dim=1)
        fused = torch.cat([rp.rcnn_cls, rp.rcnn_reg], dim=1)
        e_chain, e_fused, top = float((chain.double() - ref).abs().max()), float((fused.double() - ref).abs().max()), float(ref.abs().max())
        print(f"e_chain {e_chain:.3e}, e_fused {e_fused:.3e}, max|out| {top:.3e}")
        assert top > 1e-2 and e_fused <= 4 * e_chain + 1e-7 * top, (e_fused, e_chain, top)
        want = S.refine_rois(rp.rois, rp.roi_scores, rp.roi_labels, rp.rcnn_cls, rp.rcnn_reg)
    for b, n in enumerate(counts):
        assert torch.equal(out.boxes[b, :n], want[0][b, :n]) and torch.equal(out.scores[b, :n], want[1][b, :n]) and torch.equal(out.labels[b, :n], want[2][b, :n])
    assert float((out.boxes - old[0]).abs().max()) > 1e-3   # the new parameters arrived
    _assert_equals_eager(out, _eager(det, maps, bev), "repacked")


def _capture(run):
    """warm up on a side stream, then record one call of `run` into a graph"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    return graph


def test_one_captured_graph_of_predict_and_second_stage():
    det = _detector(5)
    static_maps = [{k: v.clone() for k, v in p.items()} for p in _head_maps(0)]
    static_bev = _bev(0, "channels_last_bf16").clone(memory_format=torch.preserve_format)
    assert static_bev.stride(1) == 1
    sp, rp = _static_plans(det, static_maps, static_bev)
    with torch.no_grad():
        graph = _capture(lambda: rp.run(sp.run(static_maps), static_bev))
    seen = set()
    for k in range(6):
        maps, bev = _head_maps(k), _bev(k, "channels_last_bf16")
        for name in static_maps[0]:
            static_maps[0][name].copy_(maps[0][name])
        static_bev.copy_(bev)
        graph.replay()
        torch.cuda.synchronize()
        seen |= set(_assert_equals_eager(rp.out, _eager(det, maps, bev), k))
    assert {0, CAP} <= seen and len(seen) > 2 and rp.repacks == 0


def test_the_plan_refuses_what_it_was_not_built_for():
    det = _detector(5)
    maps, bev = _head_maps(0), _bev(0, "nchw_fp32")
    sp, rp = _static_plans(det, maps, bev)
    with pytest.raises(_lib.S2DError, match="a gradient is required"):   # outside no_grad the head's parameters require one
        rp.run(sp.out, bev)
    with pytest.raises(_lib.S2DError, match="a gradient is required"):
        S.StaticRoIPlan(det.roi_head, det.second_stage, 5, 3, CAP, CAP, C, torch.float32, DEV)
    z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)
    det_of = lambda b, cap, dim: center_predict.StaticDetections(z(b, cap, dim), z(b, cap), z(b, cap, dtype=torch.int64), z(b, dtype=torch.int32), None)
    with torch.no_grad():
        for bad, word in [((3, CAP, 9), "7-column"), ((2, CAP, 7), "built for"), ((3, CAP + 1, 7), "built for")]:
            with pytest.raises(_lib.S2DError, match=word):
                rp.run(det_of(*bad), bev)
        for bad, word in [(bev.to(torch.bfloat16), "torch.bfloat16"), (bev[:, :8], "H, W"), (bev[:2], "H, W"), (bev.cpu(), "not a")]:
            with pytest.raises(_lib.S2DError, match=word):
                rp.run(det_of(3, CAP, 7), bad)
        with pytest.raises(_lib.S2DError, match="65 samples"):
            S.StaticRoIPlan(det.roi_head, det.second_stage, 5, 65, CAP, CAP, C, torch.float32, DEV)
        out = rp.run(det_of(3, CAP, 7), bev)   # zero counts: three samples without a detection
    assert out.counts.tolist() == [0, 0, 0] and not out.boxes.any() and bool((out.labels == -1).all())


# ---- forward_static ---------------------------------------------------------------------------------------------------------------------
def _same_lists(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w) and g["metadata"] == w["metadata"]
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert g[k].shape == w[k].shape and torch.equal(g[k], w[k]), k


def test_forward_static_equals_forward_on_fixed_maps():
    det = _detector(5)
    det.single_det.maps, det.single_det.bev = _head_maps(3), _bev(3, "channels_last_bf16")
    ex = dict(metadata=[dict(token="a"), dict(token="b"), dict(token="c")])
    with torch.enable_grad():   # forward_static is no_grad on its own
        out = det.forward_static(dict(ex))
    assert det.static_calls == 1 and det.roi_paths == {"device": 0, "torch": 0} and det.bbox_head.static_predict_calls == 1
    with torch.no_grad():
        want = det(dict(ex), return_loss=False)
    assert det.roi_paths == {"device": 1, "torch": 0} and sum(len(w["scores"]) for w in want) > CAP
    _same_lists(out.as_list(), want)
    plan = next(iter(det._static_roi_plans.values()))
    assert det.forward_static(dict(ex)) is out and det.static_calls == 2 and len(det._static_roi_plans) == 1 and plan.repacks == 0


@pytest.mark.parametrize("kind", ["VoxelNet", "KD_VoxelNet"])
def test_forward_static_on_a_small_two_stage_detector_equals_forward(kind):
    """a real first stage (VoxelNet with one block per neck stage, or the S2D student KD_VoxelNet of the two-stage configs; one frame of
    6000 points) through `first_stage_maps`, `predict_static` and the cached StaticRoIPlan; `forward` is then fed the maps that call
    produced, so both routes see the same first stage bit for bit"""
    from sparse2dense_amd import waymo_configs
    from sparse2dense_amd.data import SyntheticFrames
    torch.manual_seed(0)
    if kind == "VoxelNet":
        first = waymo_configs.centerpoint_voxelnet()
        first["neck"] = dict(first["neck"], layer_nums=[1, 1])
    else:
        first = waymo_configs.s2d_student()
    assert first["type"] == kind
    cfg = dict(type="TwoStageDetector", first_stage_cfg=first, NMS_POST_MAXSIZE=32, num_point=5, freeze=True,
               second_stage_modules=[dict(type="BEVFeatureExtractor", pc_start=[-75.2, -75.2], voxel_size=[0.1, 0.1], out_stride=8)],
               roi_head=dict(type="RoIHead", input_channels=512 * 5, code_size=7,
                             model_cfg=dict(CLASS_AGNOSTIC=True, SHARED_FC=[32, 16], CLS_FC=[16], REG_FC=[32, 16], DP_RATIO=0.3)))
    det = registry.build_detector(cfg).to(DEV).eval()
    det.single_det.test_cfg = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], score_threshold=0.05, pc_range=[-75.2, -75.2],
                                   out_size_factor=8, voxel_size=[0.1, 0.1], nms=dict(nms_pre_max_size=64, nms_post_max_size=32, nms_iou_threshold=0.7))
    ex = SyntheticFrames(1, n_points=6000, seed=5, device=DEV).example()
    seen = {}
    real = det.single_det.first_stage_maps

    def recording(example):
        seen["bev"], seen["maps"] = real(example)
        return seen["bev"], seen["maps"]
    det.single_det.first_stage_maps = recording
    out = det.forward_static(dict(ex))
    assert det.static_calls == 1 and seen["bev"].shape[:2] == (1, 512) and 0 < int(out.counts[0]) <= 32
    det.single_det.forward_two_stage = lambda example, return_loss=True, **kw: (
        det.bbox_head.predict(example, seen["maps"], det.single_det.test_cfg), seen["bev"], None, None, None, None)
    with torch.no_grad():
        want = det(dict(ex), return_loss=False)
    assert det.roi_paths == {"device": 1, "torch": 0}
    _same_lists(out.as_list(), want)
