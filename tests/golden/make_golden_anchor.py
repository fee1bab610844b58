#!/usr/bin/env python
"""Generates the anchor-head fixtures by IMPORTING the reference (read-only, /root/reference) in the build container:

    python tests/golden/make_golden_anchor.py

  anchor_targets.npz   TargetAssigner.assign_v2 (det3d/core/anchor/target_assigner.py:68-137) behind the ground-truth preparation of
                       AssignTarget.__call__ (preprocess.py:726-770) on the full 188 x 188 grid for the three frames of
                       tests/anchor_util.target_frames; anchors as every 97th row + float64 column sums
  anchor_loss.npz      MultiGroupHead.loss + backward (mg_head.py:535-695) at B = 2 on anchor_util.loss_inputs with the targets above:
                       every scalar, and of the three gradients the positives, 4 096 seeded negatives, float64 sum and sum of squares
  anchor_predict.npz   MultiGroupHead.predict (mg_head.py:697-1086) on anchor_util.predict_inputs.  THE NMS STEP OF THIS GOLDEN IS THE
                       PROJECT'S ORACLE (oracle/iou_nms.py), NOT THE REFERENCE: the reference's rotate_nms_cc is a compiled extension
                       that does not exist here; it is replaced by oracle.iou_nms.rotate_nms on the converted boxes
                       ((x, y, w, l, r) clockwise -> (dx, dy, heading) = (w, l, -r))

The numba loops run as plain Python (numba.jit is stubbed to the identity); iou_jit is wrapped so that it computes as numba would
(float64 intermediates, the result rounded once to float32).  Only inputs and outputs are stored."""
import importlib
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from make_golden import _ns, save  # noqa: E402

import anchor_util as AU  # noqa: E402  (tests/ is put on sys.path by make_golden)


class AttrDict(dict):
    __getattr__ = dict.__getitem__


def install():
    MG.install_reference_stubs()
    for pkg in ["det3d.core.bbox", "det3d.core.anchor", "det3d.ops.nms", "det3d.ops.iou3d_nms"]:
        _ns(pkg, os.path.join(MG.REF, *pkg.split(".")))
    _ns("det3d.ops.nms.nms_cpu", rotate_nms_cc=None)
    _ns("det3d.ops.nms.nms_gpu", nms_gpu=None, rotate_iou_gpu=None, rotate_nms_gpu=None)
    _ns("det3d.ops.iou3d_nms.iou3d_nms_cuda")
    _ns("det3d.ops.iou3d_nms.iou3d_nms_utils")
    meshgrid = np.meshgrid
    np.meshgrid = lambda *a, **k: list(meshgrid(*a, **k))   # the reference assigns into the result
    losses = importlib.import_module("det3d.models.losses.losses")
    reg = sys.modules["det3d.models.registry"]
    bfc = sys.modules["det3d.utils"].build_from_cfg
    sys.modules["det3d.models.builder"].build_loss = lambda cfg: bfc(cfg, reg.LOSSES)
    ops = importlib.import_module("det3d.core.bbox.box_np_ops")
    raw_iou = ops.iou_jit
    ops.iou_jit = lambda boxes, query, eps=1.0: raw_iou(boxes.astype(np.float64), query.astype(np.float64), float(eps)).astype(np.float32)
    bto = importlib.import_module("det3d.core.bbox.box_torch_ops")
    sys.modules["det3d.core"].box_torch_ops = bto
    sys.modules["det3d.core.box_torch_ops"] = bto
    return ops, bto, losses


def reference_assigner(ops):
    from sparse2dense_amd import waymo_configs as WC
    ag = importlib.import_module("det3d.core.anchor.anchor_generator")
    ta = importlib.import_module("det3d.core.anchor.target_assigner")
    sim = importlib.import_module("det3d.core.bbox.region_similarity")
    coders = importlib.import_module("det3d.core.bbox.box_coders")
    cfg = WC.SECOND_ASSIGNER["target_assigner"]
    gens = [ag.AnchorGeneratorRange(sizes=g["sizes"], anchor_ranges=g["anchor_ranges"], rotations=g["rotations"], velocities=None,
                                    match_threshold=g["matched_threshold"], unmatch_threshold=g["unmatched_threshold"],
                                    class_name=g["class_name"]) for g in cfg["anchor_generators"]]
    coder = coders.GroundBox3dCoderTorch(linear_dim=False, vec_encode=False, n_dim=7)
    return ta.TargetAssigner(box_coder=coder, anchor_generators=gens, region_similarity_calculator=sim.NearestIouSimilarity(),
                             positive_fraction=None, sample_size=512), coder


def assign_frame(assigner, ops, anchors_dict, boxes, classes):
    """the ground-truth preparation of AssignTarget.__call__ (class by class, yaw limited to [-pi, pi)) + assign_v2"""
    names = np.array(assigner.classes)
    order = np.concatenate([np.where(classes == c + 1)[0] for c in range(len(names))]).astype(np.int64)
    b, c = boxes[order].copy(), classes[order]
    b[:, -1] = ops.limit_period(b[:, -1], offset=0.5, period=np.pi * 2)
    return assigner.assign_v2(anchors_dict, b, None, gt_classes=c, gt_names=names[c - 1] if len(c) else np.zeros((0,), names.dtype))


def margins(ops, assigner, anchors_dict, boxes, classes):
    """smallest distance of an anchor's maximum overlap to a threshold of its class, and of |limit_period(r, .5, pi)| to pi / 4"""
    m_thr = np.inf
    for ci, (name, d) in enumerate(anchors_dict.items()):
        sel = boxes[classes == ci + 1]
        if not len(sel):
            continue
        sel = sel.copy()
        sel[:, -1] = ops.limit_period(sel[:, -1], offset=0.5, period=np.pi * 2)
        an = d["anchors"].reshape(-1, 7)
        ov = assigner._region_similarity_calculator.compare(an[:, [0, 1, 3, 4, 6]], sel[:, [0, 1, 3, 4, 6]]).max(1)
        for thr in (d["matched_thresholds"][0], d["unmatched_thresholds"][0]):
            m_thr = min(m_thr, float(np.abs(ov.astype(np.float64) - np.float64(thr)).min()))
    rot = ops.limit_period(boxes[:, -1], offset=0.5, period=np.pi * 2)
    m_rot = float(np.abs(np.abs(ops.limit_period(rot, 0.5, np.pi)) - np.pi / 4).min()) if len(boxes) else np.inf
    return m_thr, m_rot


def gen_targets(ops):
    assigner, coder = reference_assigner(ops)
    fmap = [1, AU.H, AU.W]
    anchors = assigner.generate_anchors(fmap)["anchors"].reshape(-1, 7)
    anchors_dict = assigner.generate_anchors_dict(fmap)
    frames = AU.target_frames(anchors)
    out = {"anchor_rows": anchors[::97].copy(), "anchor_colsum": anchors.astype(np.float64).sum(0), "anchor_count": np.int64(len(anchors))}
    labels, targets, weights = [], [], []
    for i, (b, c) in enumerate(frames):
        t0 = time.time()
        m_thr, m_rot = margins(ops, assigner, anchors_dict, b, c)
        assert m_thr > 1e-5 and m_rot > 1e-4, (i, m_thr, m_rot)
        td = assign_frame(assigner, ops, anchors_dict, b, c)
        labels.append(td["labels"].astype(np.int32)); targets.append(td["bbox_targets"].astype(np.float32))
        weights.append(td["bbox_outside_weights"].astype(np.float32))
        print(f"frame {i}: {len(b)} boxes, margins {m_thr:.2e} / {m_rot:.2e}, pos {(labels[-1] > 0).sum()}, ignored {(labels[-1] < 0).sum()}, "
              f"neg {(labels[-1] == 0).sum()}, {time.time() - t0:.1f} s")
    boxes, classes = AU.pad_frames(frames)
    labels, targets, weights = np.stack(labels), np.stack(targets), np.stack(weights)
    pos = np.argwhere(labels > 0)
    assert np.all(targets[labels <= 0] == 0) and np.all(weights == (labels > 0))
    # reg_targets are zero off the positives: stored sparse
    save("anchor_targets.npz", boxes=boxes, classes=classes, labels=labels.astype(np.int8), pos_index=pos.astype(np.int32),
         pos_targets=targets[labels > 0], **out)
    return anchors, labels, targets, coder


def reference_head(coder):
    mg = importlib.import_module("det3d.models.bbox_heads.mg_head")
    from sparse2dense_amd import waymo_configs as WC
    cfg = dict(WC.second_voxelnet_train()["bbox_head"])
    cfg.pop("type")
    cfg["box_coder"] = coder
    return mg.MultiGroupHead(**cfg)


def gen_loss(anchors, labels, targets, coder):
    head = reference_head(coder)
    b = 2
    box, cls, dirs = [t.requires_grad_(True) for t in AU.loss_inputs(b)]
    example = dict(voxels=None, num_points=None, coordinates=None, anchors=[torch.from_numpy(anchors)[None].repeat(b, 1, 1)],
                   labels=[torch.from_numpy(labels[:b].astype(np.int32))], reg_targets=[torch.from_numpy(targets[:b])])
    ret = head.loss(example, [dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)])
    ret["loss"][0].backward()
    out = {k: np.float64(ret[k][0].detach()) for k in ("loss", "cls_pos_loss", "cls_neg_loss", "dir_loss_reduced", "cls_loss_reduced",
                                                       "loc_loss_reduced")}
    out["loc_loss_elem"] = np.asarray([float(v) for v in ret["loc_loss_elem"][0]], np.float64)
    out["num_pos"], out["num_neg"] = np.int64(ret["num_pos"][0]), np.int64(ret["num_neg"][0])
    flat = labels[:b].reshape(-1)
    pos, neg = np.flatnonzero(flat > 0), AU.negative_sample(labels[:b])
    for name, t, width in (("box", box, 7), ("cls", cls, 3), ("dir", dirs, 2)):
        g = t.grad.reshape(-1, width).numpy()
        out[f"d{name}_pos"], out[f"d{name}_neg"] = g[pos], g[neg]
        out[f"d{name}_sum"], out[f"d{name}_sumsq"] = np.float64(g.astype(np.float64).sum()), np.float64((g.astype(np.float64) ** 2).sum())
        out[f"d{name}_absmax"] = np.float64(np.abs(g).max())
    print({k: v for k, v in out.items() if np.ndim(v) == 0})
    save("anchor_loss.npz", **out)


def gen_predict(anchors, coder, bto):
    from oracle import iou_nms
    from sparse2dense_amd import waymo_configs as WC
    head = reference_head(coder)
    thr = WC.SECOND_TEST_CFG["nms"]["nms_iou_threshold"]
    seen = []

    def rotate_nms_cc(dets, iou_threshold):   # dets: (x, y, w, l, r, score), sorted by the caller's topk
        b7 = np.zeros((len(dets), 7), np.float32)
        b7[:, [0, 1, 3, 4]] = dets[:, :4]
        b7[:, 6] = -dets[:, 4]
        iou = iou_nms.bev_iou(b7, b7)
        off = iou[~np.eye(len(b7), dtype=bool)]
        assert not np.any((off > thr / 2) & (off < thr * 2)), "a candidate pair sits near the NMS threshold: pick another seed"
        seen.append(len(dets))
        return iou_nms.rotate_nms(b7, dets[:, 5], iou_threshold)
    bto.rotate_nms_cc = rotate_nms_cc
    b = 2
    box, cls, dirs = AU.predict_inputs(b)
    example = dict(voxels=None, num_points=None, coordinates=None, anchors=[torch.from_numpy(anchors)[None].repeat(b, 1, 1)], metadata=[])
    test_cfg = AttrDict({k: (AttrDict(v) if isinstance(v, dict) else v) for k, v in WC.SECOND_TEST_CFG.items()})
    with torch.no_grad():
        rets = head.predict(example, [dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)], test_cfg)
        # the candidate set before the NMS, by the reference's own calls
        dec = coder.decode_torch(box.view(b, -1, 7), example["anchors"][0])
        scores, lab = torch.max(torch.sigmoid(cls.view(b, -1, 3)), dim=-1)
        dlab = torch.max(dirs.view(b, -1, 2), dim=-1)[1]
    out = {}
    for i in range(b):
        keep = scores[i] >= torch.tensor([WC.SECOND_TEST_CFG["score_threshold"]]).type_as(scores)
        idx = torch.nonzero(keep).reshape(-1)
        out[f"cand_index_{i}"] = idx.numpy().astype(np.int32)
        out[f"cand_boxes_{i}"] = dec[i][idx].numpy()
        out[f"cand_scores_{i}"] = scores[i][idx].numpy()
        out[f"cand_labels_{i}"] = lab[i][idx].numpy().astype(np.int32)
        out[f"cand_dir_{i}"] = dlab[i][idx].numpy().astype(np.int32)
        out[f"box3d_lidar_{i}"] = rets[i]["box3d_lidar"].numpy()
        out[f"scores_{i}"] = rets[i]["scores"].numpy()
        out[f"label_preds_{i}"] = rets[i]["label_preds"].numpy().astype(np.int64)
        print(f"sample {i}: {len(idx)} candidates -> {len(rets[i]['scores'])} boxes")
    assert len(seen) == b
    save("anchor_predict.npz", **out)


if __name__ == "__main__":
    ops, bto, _ = install()
    anchors, labels, targets, coder = gen_targets(ops)
    gen_loss(anchors, labels, targets, coder)
    gen_predict(anchors, coder, bto)
