"""The device two-stage RoI path (csrc/roi_head.hip through second_stage.py) against the reference's recorded outputs
(tests/golden/second_stage.npz, roi_training.npz) and against the torch chain on the CPU."""
import copy
import os

import numpy as np
import pytest
import torch

from golden_util import fill_params, seeded
from sparse2dense_amd import _lib, registry, second_stage as S
from test_second_stage import ROI_TRAIN_CFG, _check_roi_training

pytestmark = pytest.mark.gpu

EXT = dict(pc_start=[-75.2, -75.2], voxel_size=[0.1, 0.1], out_stride=8)


def _chain_features(bev_nhwc, centers, num_point, ext=EXT):
    """the torch chain on the CPU: bev [H, W, C] fp32, centers [num_point * n, 3] -> [n, num_point * C]"""
    e = S.BEVFeatureExtractor(**ext)
    return e({"bev_feature": bev_nhwc[None]}, [centers], num_point)[0]


# ---- features ---------------------------------------------------------------------------------------------------------------------------
def _fixture_features(g, bev_nchw):
    """The fixture's 200 sample points are an affine image of the boxes' side points (make_golden_r02.py:131-134), so no box list has
    exactly them as its side points: each point is presented as the CENTRE of a box of its own (num_point = 1, 200 slots) and the five
    sets of 40 are laid side by side as the reference's torch.cat does.  The blend sees the reference's coordinates bit for bit."""
    pts = torch.from_numpy(g["centers"])
    boxes = torch.cat([pts, torch.zeros(200, 4)], dim=1).cuda()
    row = torch.arange(200, dtype=torch.int32).view(1, 200).cuda()
    f = S.roi_bev_features(bev_nchw, boxes, row, EXT["pc_start"], EXT["voxel_size"], EXT["out_stride"], num_point=1)
    assert f.shape == (1, 200, 24) and f.dtype == torch.float32
    return torch.cat([f[0, i * 40:(i + 1) * 40] for i in range(5)], dim=1).cpu()


def test_bev_features_match_the_reference_on_both_layouts_and_bf16(golden_dir):
    g = np.load(os.path.join(golden_dir, "second_stage.npz"))
    nhwc = torch.from_numpy(g["bev"]).cuda()                         # [1, 47, 53, 24]
    x = (g["centers"][:, 0] + 75.2) / 0.8
    y = (g["centers"][:, 1] + 75.2) / 0.8
    assert int(((x < 0) | (x > 52) | (y < 0) | (y > 46)).sum()) == 70   # the clamps are exercised
    views = {"nchw": nhwc.permute(0, 3, 1, 2).contiguous(), "channels_last": nhwc.permute(0, 3, 1, 2)}
    assert views["nchw"].is_contiguous() and views["channels_last"].stride(1) == 1
    for name, v in views.items():
        np.testing.assert_allclose(_fixture_features(g, v).numpy(), g["bev_features"], rtol=1e-5, atol=1e-5, err_msg=name)
    # bf16 channels_last: the taps are widened before the multiply = the chain on the rounded map
    bf = nhwc.to(torch.bfloat16)
    ref = _chain_features(bf.float().cpu()[0], torch.from_numpy(g["centers"]), 5)
    np.testing.assert_allclose(_fixture_features(g, bf.permute(0, 3, 1, 2)).numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(_fixture_features(g, bf.permute(0, 3, 1, 2).contiguous()).numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("layout,dtype,channels,num_point", [
    ("channels_last", torch.bfloat16, 512, 5),    # the fast case: one 16-byte load per lane and tap, all 64 lanes
    ("channels_last", torch.bfloat16, 512, 1),
    ("channels_last", torch.float32, 512, 5),
    ("nchw", torch.float32, 512, 5),
    ("nchw", torch.bfloat16, 40, 5),
    ("channels_last", torch.bfloat16, 21, 5),     # odd channel count: element loads, unaligned rows
    ("channels_last_sliced", torch.bfloat16, 24, 5),   # channels 1..24 of 32: contiguous channels, rows not 16-byte aligned
    ("channels_last_padded", torch.bfloat16, 24, 5),   # channels 0..23 of 32: aligned rows with a pitch above the channel count
    ("channels_last", torch.float32, 22, 1),
])
def test_bev_features_of_a_batch_with_holes_match_the_chain(layout, dtype, channels, num_point):
    """B = 3 with 0, 7 and 16 boxes in 16 slots, a shuffled row table with -1 holes, a 16 x 16 map that the side points leave"""
    ext = dict(pc_start=[-6.4, -6.4], voxel_size=[0.1, 0.1], out_stride=8)
    counts, cap = (0, 7, 16), 16
    total = sum(counts)
    boxes = torch.cat([seeded((total, 2), 21, 5.0), seeded((total, 1), 22), seeded((total, 3), 23).abs() + 0.5, seeded((total, 1), 24, 2.0)], 1)
    lo = 1 if layout == "channels_last_sliced" else 0
    stored = seeded((3, 16, 16, 32 if layout in ("channels_last_sliced", "channels_last_padded") else channels), 25).to(dtype)
    nhwc = stored[..., lo:lo + channels]
    bev = stored.cuda().permute(0, 3, 1, 2)[:, lo:lo + channels]
    bev = bev.contiguous() if layout == "nchw" else bev
    assert bev.shape == (3, channels, 16, 16) and (layout == "nchw") == bev.is_contiguous()
    rng = np.random.RandomState(5)
    row = np.full((3, cap), -1, np.int32)
    row[1, rng.permutation(cap)[:7]] = rng.permutation(7)                 # sample 1: its 7 boxes in shuffled slots, 9 holes
    row[2] = 7 + rng.permutation(16)
    row[2, [3, 11]] = -1
    filler = torch.full((3, cap, num_point * channels), float("nan"), device="cuda")   # the allocator hands this block to the output
    del filler
    got = S.roi_bev_features(bev, boxes.cuda(), torch.from_numpy(row).cuda(), ext["pc_start"], ext["voxel_size"], ext["out_stride"], num_point).cpu()
    assert got.shape == (3, cap, num_point * channels)
    centers = S.box_side_centers(boxes) if num_point == 5 else boxes[:, :3]
    outside = 0
    for b in range(3):
        ref = _chain_features(nhwc[b].float(), centers, num_point, ext)   # all boxes on sample b's map
        for s in range(cap):
            if row[b, s] < 0:
                assert torch.equal(got[b, s], torch.zeros_like(got[b, s])), (b, s)
            else:
                np.testing.assert_allclose(got[b, s].numpy(), ref[row[b, s]].numpy(), rtol=1e-5, atol=1e-5, err_msg=f"{b} {s}")
    xy = (centers[:, :2] + 6.4) / 0.8
    outside = int(((xy < 0) | (xy > 15)).any(dim=1).sum())
    assert 0 < outside < len(centers)


# ---- match ------------------------------------------------------------------------------------------------------------------------------
def _oracle_iou3d(a, b):
    from oracle import iou_nms as OI
    return S.boxes_iou3d(a, b, bev_iou=lambda x, y: torch.from_numpy(OI.bev_iou(x.numpy(), y.numpy())))


def test_match_gives_the_reference_iou_and_row_for_every_roi(golden_dir):
    g = np.load(os.path.join(golden_dir, "roi_training.npz"))
    rois, labels, gt = torch.from_numpy(g["rois"]), torch.from_numpy(g["roi_labels"]), torch.from_numpy(g["gt"])
    assert rois.shape == (2, 60, 7) and gt.shape == (2, 20, 8) and int((labels == 0).sum()) > 0
    # samples 0, 1: the fixture; 2: ground truth all zero; 3: sample 0 with a label that no ground-truth row carries on every third RoI
    rois4 = torch.cat([rois, rois[:1], rois[:1]])
    labels4 = torch.cat([labels, labels[:1], labels[:1]]).clone()
    labels4[3, ::3] = 7
    gt4 = torch.cat([gt, torch.zeros_like(gt[:1]), gt[:1]])
    layer = S.ProposalTargetLayer(ROI_TRAIN_CFG["TARGET_CONFIG"], iou_fn=_oracle_iou3d)
    for by_class in (True, False):
        iou, arg, count = [t.cpu() for t in S.match_rois_to_gt(rois4.cuda(), labels4.cuda(), gt4.cuda(), by_class=by_class)]
        assert iou.dtype == torch.float32 and arg.dtype == torch.int64 and count.dtype == torch.int32
        assert count.tolist() == [12, 12, 1, 12]
        for b in (0, 1, 3):
            valid = gt4[b, :12]
            if by_class:
                ref_iou, ref_arg = layer.get_max_iou_with_same_class(rois4[b], labels4[b], valid[:, :7], valid[:, -1].long())
            else:
                ref_iou, ref_arg = torch.max(_oracle_iou3d(rois4[b], valid[:, :7]), dim=1)
            np.testing.assert_allclose(iou[b].numpy(), ref_iou.numpy(), rtol=0, atol=2e-4, err_msg=f"{by_class} {b}")
            assert torch.equal(arg[b], ref_arg), (by_class, b, (arg[b] != ref_arg).nonzero().view(-1).tolist())   # EVERY RoI
            assert float(ref_iou.max()) > 0.55
        assert float(iou[2].abs().max()) == 0 and int(arg[2].abs().max()) == 0
        if by_class:
            assert float(iou[3, ::3].abs().max()) == 0 and int(arg[3, ::3].abs().max()) == 0 and float(iou[3].max()) > 0.55


def test_match_rejects_more_ground_truth_than_it_stages():
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    with pytest.raises(_lib.S2DError, match="1..512 supported"):
        S.match_rois_to_gt(z(1, 4, 7), z(1, 4, dtype=torch.long), z(1, S.ROI_MAX_GT + 1, 8))
    iou, arg, count = S.match_rois_to_gt(z(1, 4, 7), z(1, 4, dtype=torch.long), z(1, S.ROI_MAX_GT, 8))
    assert count.tolist() == [1] and float(iou.abs().max()) == 0


# ---- the training branch ----------------------------------------------------------------------------------------------------------------
def test_roi_head_training_branch_on_the_device_path_matches_the_reference(golden_dir):
    """roi_training.npz through RoIHead.forward(device=True): match kernel -> one read -> host draws -> one copy -> targets kernel.
    The fixture's IoUs keep at least 2e-3 from every sampling threshold, so the same RoIs are sampled as by the reference."""
    g = np.load(os.path.join(golden_dir, "roi_training.npz"))
    roi = registry.build(dict(type="RoIHead", input_channels=40, code_size=7, model_cfg=ROI_TRAIN_CFG), registry.ROI_HEAD)
    fill_params(roi).train().to("cuda")
    np.random.seed(int(g["np_seed"])); torch.manual_seed(int(g["torch_seed"]))
    t = lambda k: torch.from_numpy(g[k]).cuda()
    batch = dict(rois=t("rois"), roi_labels=t("roi_labels"), roi_scores=t("roi_scores"), roi_features=t("roi_features"), gt_boxes_and_cls=t("gt"))
    roi(batch, training=True, device=True)
    total, tb = roi.get_loss()
    total.backward()
    ret = roi.forward_ret_dict
    _check_roi_training(g, roi, ret, total, tb, rtol=2e-4, atol=2e-5)
    assert ret["rois"].shape == (2, 32, 7) and ret["gt_of_rois"].shape == (2, 32, 8) and ret["roi_features"].shape == (2, 32, 40)
    assert ret["reg_valid_mask"].dtype == torch.int64 and ret["roi_labels"].dtype == torch.int64 and ret["rcnn_cls_labels"].dtype == torch.float32


def test_targets_with_hard_labels_match_the_chain(golden_dir):
    """CLS_SCORE_TYPE = "cls" (int64 labels with -1 between the thresholds) and the encode on arbitrary sampled slots, against the chain
    on the CPU fed the kernel's own IoUs and rows"""
    g = np.load(os.path.join(golden_dir, "roi_training.npz"))
    cfg = dict(ROI_TRAIN_CFG["TARGET_CONFIG"], CLS_SCORE_TYPE="cls")
    t = lambda k: torch.from_numpy(g[k]).cuda()
    iou, arg, _ = S.match_rois_to_gt(t("rois"), t("roi_labels"), t("gt"))
    idx = torch.from_numpy(np.random.RandomState(2).randint(0, 60, size=(2, 45)).astype(np.int32))
    out = {k: v.cpu() for k, v in S.roi_targets(idx.cuda(), t("rois"), t("roi_labels"), t("roi_scores"), iou, arg, t("gt"), cfg).items()}
    take = lambda x: torch.stack([x[b][idx[b].long()] for b in range(2)])
    ious, rois = take(iou.cpu()), take(torch.from_numpy(g["rois"]))
    gt_src = torch.stack([torch.from_numpy(g["gt"])[b][arg.cpu()[b][idx[b].long()]] for b in range(2)])
    assert torch.equal(out["rois"], rois) and torch.equal(out["gt_of_rois_src"], gt_src) and torch.equal(out["gt_iou_of_rois"], ious)
    assert torch.equal(out["roi_labels"], take(torch.from_numpy(g["roi_labels"]))) and torch.equal(out["roi_scores"], take(torch.from_numpy(g["roi_scores"])))

    class Fixed(S.ProposalTargetLayer):   # the chain behind the sampling, fed the same sampled tensors
        def sample_rois_for_rcnn(self, batch_dict):
            return rois.clone(), gt_src.clone(), ious.clone(), out["roi_scores"], out["roi_labels"], torch.zeros(2, 45, 1)
    head = registry.build(dict(type="RoIHead", input_channels=40, code_size=7, model_cfg=ROI_TRAIN_CFG), registry.ROI_HEAD)
    head.proposal_target_layer = Fixed(cfg)
    ref = head.assign_targets(dict(batch_size=2))
    assert ref["rcnn_cls_labels"].dtype == out["rcnn_cls_labels"].dtype == torch.int64
    assert torch.equal(out["rcnn_cls_labels"], ref["rcnn_cls_labels"]) and torch.equal(out["reg_valid_mask"], ref["reg_valid_mask"])
    assert set(out["rcnn_cls_labels"].unique().tolist()) == {-1, 0, 1}
    np.testing.assert_allclose(out["gt_of_rois"].numpy(), ref["gt_of_rois"].numpy(), rtol=2e-4, atol=2e-5)


# ---- refine -----------------------------------------------------------------------------------------------------------------------------
def test_refine_matches_the_reference_boxes_and_post_process(golden_dir):
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
        dev_head = copy.deepcopy(roi).cuda()
        out = dev_head(dict(rois=rois.cuda(), roi_features=feats.cuda(), roi_scores=scores.cuda(), roi_labels=labels.cuda()), training=False, device=True)
    np.testing.assert_allclose(out["batch_box_preds"].cpu().numpy(), g["batch_box_preds"], rtol=1e-4, atol=1e-5)    # the reference
    np.testing.assert_allclose(out["batch_cls_preds"].cpu().numpy(), g["batch_cls_preds"], rtol=1e-4, atol=1e-5)
    assert out["batch_box_preds"].shape == (1, 50, 7) and out["refined_scores"].shape == (1, 50) and out["refined_labels"].dtype == torch.int64
    np.testing.assert_allclose(out["batch_box_preds"][0, :40].cpu().numpy(), ref["box3d_lidar"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out["refined_scores"][0, :40].cpu().numpy(), ref["scores"].numpy(), rtol=1e-4, atol=1e-5)
    assert torch.equal(out["refined_labels"][0, :40].cpu(), ref["label_preds"]) and int(out["refined_labels"][0, 40:].max()) == -1
    assert float(ref["scores"].max()) > 0.1


# ---- pack -------------------------------------------------------------------------------------------------------------------------------
def test_pack_pads_as_the_chain_does():
    boxes9 = seeded((12, 9), 41).cuda()
    scores, labels = seeded((12,), 42).abs().cuda(), (torch.arange(12) % 3).cuda()
    offsets = [0, 5, 5, 12]
    rois, roi_scores, roi_labels = S.pack_rois(boxes9, scores, labels, offsets, 6)
    assert rois.shape == (3, 6, 7) and roi_labels.dtype == torch.int64
    for b in range(3):
        n = min(offsets[b + 1] - offsets[b], 6)
        src = boxes9[offsets[b]:offsets[b] + n]
        assert torch.equal(rois[b, :n], src[:, [0, 1, 2, 3, 4, 5, 8]]) and float(rois[b, n:].abs().sum()) == 0
        assert torch.equal(roi_scores[b, :n], scores[offsets[b]:offsets[b] + n]) and float(roi_scores[b, n:].abs().sum()) == 0
        assert torch.equal(roi_labels[b, :n], labels[offsets[b]:offsets[b] + n] + 1) and int(roi_labels[b, n:].abs().sum()) == 0


# ---- detector ---------------------------------------------------------------------------------------------------------------------------
TEST_CFG = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], pc_range=[-75.2, -75.2], out_size_factor=8, voxel_size=[0.1, 0.1],
                nms=dict(nms_pre_max_size=4096, nms_post_max_size=500, nms_iou_threshold=0.7))


def _detector(first_stage, model_cfg):
    cfg = dict(type="TwoStageDetector", first_stage_cfg=first_stage, NMS_POST_MAXSIZE=500, num_point=5, freeze=True,
               second_stage_modules=[dict(type="BEVFeatureExtractor", **EXT)],
               roi_head=dict(type="RoIHead", input_channels=512 * 5, code_size=7, model_cfg=model_cfg))
    return registry.build_detector(cfg).to("cuda")


def _replay_first_stage(det, ex, return_loss):
    """runs the first stage ONCE and makes det.single_det hand the same result to every later forward: the two paths then see the same
    proposals and the same neck map bit for bit (combine_loss appends to the loss lists, so each call gets its own copies)"""
    with torch.no_grad():
        first = det.single_det.forward_two_stage(ex, return_loss)

    def again(example, return_loss=True, **kw):
        return tuple(({k: list(v) for k, v in o.items()} if i == 3 and isinstance(o, dict) else o) for i, o in enumerate(first))
    det.single_det.forward_two_stage = again
    return first


def test_detector_inference_takes_the_device_path_and_agrees_with_the_chain(monkeypatch):
    from sparse2dense_amd import waymo_configs
    from sparse2dense_amd.data import SyntheticFrames
    torch.manual_seed(0)
    det = _detector(waymo_configs.s2d_student(), dict(CLASS_AGNOSTIC=True, SHARED_FC=[256, 256], CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=0.3)).eval()
    det.single_det.test_cfg = dict(TEST_CFG, score_threshold=0.05)
    ex = SyntheticFrames(2, n_points=20000, seed=5, device="cuda").example()
    first = _replay_first_stage(det, ex, False)
    assert first[1].is_cuda and first[1].shape[1] == 512
    monkeypatch.delenv("S2D_ROI_DEVICE", raising=False)
    with torch.no_grad():
        dev = det(dict(ex), return_loss=False)
        assert det.roi_paths == {"device": 1, "torch": 0}
        monkeypatch.setenv("S2D_ROI_DEVICE", "0")
        ref = det(dict(ex), return_loss=False)
    assert det.roi_paths == {"device": 1, "torch": 1}
    assert len(dev) == len(ref) == 2
    for d, r in zip(dev, ref):
        assert 0 < len(r["scores"]) <= 500 and d["box3d_lidar"].shape == r["box3d_lidar"].shape and torch.equal(d["label_preds"], r["label_preds"])
        np.testing.assert_allclose(d["box3d_lidar"].cpu().numpy(), r["box3d_lidar"].cpu().numpy(), rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(d["scores"].cpu().numpy(), r["scores"].cpu().numpy(), rtol=1e-4, atol=1e-6)


def test_detector_training_step_takes_the_device_path_and_agrees_with_the_chain(monkeypatch):
    from sparse2dense_amd import scene, waymo_configs
    from sparse2dense_amd.data import SyntheticFrames
    torch.manual_seed(0)
    model_cfg = dict(ROI_TRAIN_CFG, SHARED_FC=[256, 256], CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=0.3,
                     TARGET_CONFIG=dict(ROI_TRAIN_CFG["TARGET_CONFIG"], ROI_PER_IMAGE=128))
    det = _detector(waymo_configs.centerpoint_voxelnet(), model_cfg).train()
    det.single_det.test_cfg = dict(TEST_CFG, score_threshold=0.0)
    ex = SyntheticFrames(2, n_points=20000, seed=5, device="cuda").example()
    gts = []
    for b in range(2):   # gt_boxes_and_cls as AssignLabel lays it out: (x, y, z, w, l, h, yaw, vx, vy, class), zero padded
        s = scene.make_scene(20000, seed=5 + b)
        rows = np.zeros((500, 10), np.float32)
        n = len(s["gt_boxes"])
        rows[:n, :9] = s["gt_boxes"][:, [0, 1, 2, 3, 4, 5, 8, 6, 7]]
        rows[:n, 9] = s["gt_classes"]
        gts.append(rows)
    ex["gt_boxes_and_cls"] = torch.from_numpy(np.stack(gts)).cuda()
    first = _replay_first_stage(det, ex, True)
    monkeypatch.delenv("S2D_ROI_DEVICE", raising=False)

    def step(example):
        np.random.seed(3); torch.manual_seed(3)
        det.zero_grad(set_to_none=True)
        losses = det(example, return_loss=True)
        sum(losses["loss"]).backward()
        ret = det.roi_head.forward_ret_dict
        grads = {n: p.grad.detach().clone() for n, p in det.roi_head.named_parameters()}
        return losses, {k: v.detach().clone() for k, v in ret.items()}, grads

    dev_loss, dev_ret, dev_grad = step(dict(ex))
    assert det.roi_paths == {"device": 1, "torch": 0}
    monkeypatch.setenv("S2D_ROI_DEVICE", "0")
    ref_loss, ref_ret, ref_grad = step(dict(ex))
    assert det.roi_paths == {"device": 1, "torch": 1}
    assert set(dev_ret) == set(ref_ret)
    for k in ref_ret:
        assert dev_ret[k].shape == ref_ret[k].shape and dev_ret[k].dtype == ref_ret[k].dtype, k
    assert dev_ret["rois"].shape == (2, 128, 7) and dev_ret["roi_features"].shape == (2, 128, 2560)
    assert torch.equal(dev_ret["rois"], ref_ret["rois"]) and torch.equal(dev_ret["roi_labels"], ref_ret["roi_labels"])   # the same RoIs were sampled
    assert torch.equal(dev_ret["reg_valid_mask"], ref_ret["reg_valid_mask"])
    for k in ("gt_of_rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "rcnn_cls_labels", "roi_features", "rcnn_cls", "rcnn_reg"):
        np.testing.assert_allclose(dev_ret[k].float().cpu().numpy(), ref_ret[k].float().cpu().numpy(), rtol=1e-4, atol=1e-4, err_msg=k)
    for k in ("loss", "roi_reg_loss", "roi_cls_loss"):
        np.testing.assert_allclose([float(v) for v in dev_loss[k]], [float(v) for v in ref_loss[k]], rtol=1e-4, err_msg=k)
    for n in ref_grad:
        a, b = dev_grad[n].double(), ref_grad[n].double()
        assert float((a - b).norm() / (b.norm() + 1e-30)) <= 2e-3, n
    assert all(p.grad is None for p in det.single_det.parameters())
    # a neck map that carries a gradient takes the chain (no backward through the BEV sampling)
    monkeypatch.delenv("S2D_ROI_DEVICE", raising=False)
    live = first[1].detach().clone().requires_grad_(True)
    assert "gradient" in det.device_path_reason(first[0], live, ex, True) and det.device_path_reason(first[0], first[1], dict(ex), True) is None
    det.single_det.forward_two_stage = lambda example, return_loss=True, **kw: (first[0], live, first[2], {k: list(v) for k, v in first[3].items()})
    step(dict(ex))
    assert det.roi_paths == {"device": 1, "torch": 2}
