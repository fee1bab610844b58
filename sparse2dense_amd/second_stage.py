"""Two-stage CenterPoint head: what sits on top of the hot path's first stage in the reference's
`two_stage` configs (first stage frozen, configs/waymo/voxelnet/two_stage/*: num_point=5, NMS_POST_MAXSIZE=500).

  DETECTORS["TwoStageDetector"]        /root/reference/det3d/models/detectors/two_stage.py:8-199
  SECOND_STAGE["BEVFeatureExtractor"]  /root/reference/det3d/models/second_stage/bird_eye_view.py:9-41
                                       (bilinear_interpolate_torch, det3d/core/utils/center_utils.py:93-122)
  ROI_HEAD["RoIHead"]                  /root/reference/det3d/models/roi_heads/roi_head.py:16-106,
                                       roi_head_template.py:27-41,153-183 (make_fc_layers, generate_predicted_boxes)
  VoxelNet/KD_VoxelNet.forward_two_stage   /root/reference/det3d/models/detectors/voxelnet.py:107-141,266-301

  ProposalTargetLayer                  /root/reference/det3d/models/roi_heads/target_assigner/proposal_target_layer.py:14-237
  RoIHead.assign_targets / losses      /root/reference/det3d/models/roi_heads/roi_head_template.py:43-151
  boxes_iou3d                          /root/reference/det3d/ops/iou3d_nms/iou3d_nms_utils.py:28-70

Module / parameter names follow the reference (`single_det.*`, `roi_head.shared_fc_layer.0.weight` ...), so two-stage
checkpoints load through checkpoint.load_state_dict.  Inference path (`return_loss=False`): first-stage decode + rotated NMS
(heads.CenterHead.predict on the HIP kernels) -> 5 BEV feature samples per box -> RoI MLP -> refined boxes and scores.
Training path (`return_loss=True`, two_stage.py:154-199): the same first stage with its loss, then the RoIs are matched to the
ground truth by 3-D IoU (rotated BEV overlap from csrc/nms.hip x height overlap), sampled into ROI_PER_IMAGE foreground /
hard- / easy-background boxes with the reference's numpy / torch random draws (same seeds -> same samples), residual targets are
encoded in each RoI's frame, and the RoI MLP is trained with the IoU-scaled BCE + masked L1 losses.

Device path (csrc/roi_head.hip; `pack_rois`, `roi_bev_features`, `match_rois_to_gt`, `roi_targets`, `refine_rois` below): everything
between the first stage's predict and the RoI MLP, and behind the MLP at inference, in one launch each.  The neck map is read where it
lies (NCHW or channels_last, fp32 or bf16): no fp32 NHWC copy.  Training reads `max_iou` back once (the sampling draws are the
reference's host draws, `ProposalTargetLayer.subsample_rois_host`) and sends the sampled indices with their slot-to-row table in one
copy; only the ROI_PER_IMAGE sampled RoIs get BEV features.  `TwoStageDetector.forward` takes this path whenever it applies
(`TwoStageDetector.device_path_reason`), `S2D_ROI_DEVICE=0` keeps the torch chain; `det.roi_paths` counts the calls of each.

RoI MLP at inference (csrc/roi_mlp.hip; `roi_mlp_reference`, `roi_mlp_fused`, `RoIHead.mlp_reason`): on the device path the eval-mode MLP - shared_fc_layer,
cls_layers, reg_layers - is ONE fused fp32 MFMA launch from a packed weight image and a scale / shift vector cached on the head.  Training mode, a required
gradient, a head outside the kernel's shape family or `S2D_ROI_MLP=0` keep the three nn.Sequential's; `head.mlp_paths` counts the calls of each.

RoI head training (csrc/roi_mlp_train.hip; `roi_mlp_train_reference`, `roi_loss_reference`, `roi_mlp_train_fused`, `roi_loss_fused`, `RoIHead.fused_training`,
`train_mlp_reason`, `train_paths`): opt-in, the training-mode MLP (batch statistics, dropout masks drawn in one call), the two RoI losses and the backward of all
of it on fp32 MFMA kernels, one launch per depth, with no host read between the first forward and the last backward launch.  Off by default: nothing above
changes unless `head.fused_training` is set.

Static path (`StaticRoIPlan`, `TwoStageDetector.forward_static`; s2d_roi_pack_static, s2d_roi_refine_static): the inference second stage on the
padded, device-counted detections of `CenterHead.predict_static`, every buffer allocated once, 4 launches with no host read - capturable into
one HIP graph behind the static predict.  Opt-in; nothing above takes it by itself."""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, center_predict, registry
from .registry import DETECTORS, ROI_HEAD, SECOND_STAGE

ROI_MAX_GT = 512      # S2D_ROI_MAX_GT: ground-truth rows per sample that s2d_roi_match_gt stages in LDS
ROI_MAX_BATCH = 64    # S2D_ROI_MAX_BATCH: the per-sample offsets of s2d_roi_pack travel in the kernel arguments


def bilinear_interpolate(im, x, y):
    """im [H, W, C]; x, y [N] in feature-map cells -> [N, C] (center_utils.py:93-122: neighbours clamped to the map)"""
    x0 = torch.floor(x).long()
    y0 = torch.floor(y).long()
    x1, y1 = x0 + 1, y0 + 1
    x0c, x1c = x0.clamp(0, im.shape[1] - 1), x1.clamp(0, im.shape[1] - 1)
    y0c, y1c = y0.clamp(0, im.shape[0] - 1), y1.clamp(0, im.shape[0] - 1)
    wa = (x1c.type_as(x) - x) * (y1c.type_as(y) - y)
    wb = (x1c.type_as(x) - x) * (y - y0c.type_as(y))
    wc = (x - x0c.type_as(x)) * (y1c.type_as(y) - y)
    wd = (x - x0c.type_as(x)) * (y - y0c.type_as(y))
    return (im[y0c, x0c] * wa[:, None] + im[y1c, x0c] * wb[:, None] + im[y0c, x1c] * wc[:, None] + im[y1c, x1c] * wd[:, None])


@SECOND_STAGE.register_module
class BEVFeatureExtractor(nn.Module):
    def __init__(self, pc_start, voxel_size, out_stride):
        super().__init__()
        self.pc_start, self.voxel_size, self.out_stride = pc_start, voxel_size, out_stride

    def absl_to_relative(self, absolute):
        a1 = (absolute[..., 0] - self.pc_start[0]) / self.voxel_size[0] / self.out_stride
        a2 = (absolute[..., 1] - self.pc_start[1]) / self.voxel_size[1] / self.out_stride
        return a1, a2

    def forward(self, example, batch_centers, num_point):
        ret = []
        for bev, centers in zip(example["bev_feature"], batch_centers):
            xs, ys = self.absl_to_relative(centers)
            feat = bilinear_interpolate(bev, xs, ys)
            if num_point > 1:   # the num_point sample sets are stacked along dim 0: concatenate them per box
                sec = len(feat) // num_point
                feat = torch.cat([feat[i * sec:(i + 1) * sec] for i in range(num_point)], dim=1)
            ret.append(feat)
        return ret


def _cfg_get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg.get(key, *default) if default else cfg[key]
    return getattr(cfg, key, *default)


def limit_period(val, offset=0.5, period=np.pi):
    return val - torch.floor(val / period + offset) * period


def rotate_points_along_z(points, angle):
    """points [B, N, 3+C] as ROW vectors times [[c, -s, 0], [s, c, 0], [0, 0, 1]] per batch entry (box_torch_ops.py:326-344)"""
    cosa, sina = torch.cos(angle), torch.sin(angle)
    x = points[:, :, 0] * cosa[:, None] + points[:, :, 1] * sina[:, None]
    y = -points[:, :, 0] * sina[:, None] + points[:, :, 1] * cosa[:, None]
    return torch.cat([x[..., None], y[..., None], points[:, :, 2:]], dim=-1)


def _to_pcdet(boxes):
    """(x, y, z, w, l, h, yaw) -> OpenPCDet's (x, y, z, dx, dy, dz, heading) (iou3d_nms_utils.py:22-26)"""
    b = boxes[:, [0, 1, 2, 4, 3, 5, -1]].clone()
    b[:, -1] = -b[:, -1] - np.pi / 2
    return b


def boxes_iou3d(boxes_a, boxes_b, bev_iou=None):
    """3-D IoU matrix [N, M] of (x, y, z, w, l, h, yaw) boxes (iou3d_nms_utils.boxes_iou3d_gpu): rotated BEV overlap x height overlap
    over the union of the volumes.  The BEV overlap comes from the device IoU kernel (IoU = o / (A + B - o) -> o = IoU (A + B) /
    (1 + IoU)); `bev_iou` (tests: the CPU oracle) replaces it, otherwise CUDA tensors are required - no CPU fallback."""
    a, b = _to_pcdet(boxes_a), _to_pcdet(boxes_b)
    if bev_iou is None:
        from . import nms
        bev_iou = nms.boxes_iou_bev
    iou = bev_iou(a.contiguous(), b.contiguous()).to(a.dtype)
    area_a, area_b = (a[:, 3] * a[:, 4]).view(-1, 1), (b[:, 3] * b[:, 4]).view(1, -1)
    overlaps_bev = iou * (area_a + area_b) / (1.0 + iou)
    a_max, a_min = (a[:, 2] + a[:, 5] / 2).view(-1, 1), (a[:, 2] - a[:, 5] / 2).view(-1, 1)
    b_max, b_min = (b[:, 2] + b[:, 5] / 2).view(1, -1), (b[:, 2] - b[:, 5] / 2).view(1, -1)
    overlaps_h = torch.clamp(torch.min(a_max, b_max) - torch.max(a_min, b_min), min=0)
    overlaps_3d = overlaps_bev * overlaps_h
    vol_a, vol_b = (a[:, 3] * a[:, 4] * a[:, 5]).view(-1, 1), (b[:, 3] * b[:, 4] * b[:, 5]).view(1, -1)
    return overlaps_3d / torch.clamp(vol_a + vol_b - overlaps_3d, min=1e-6)


def _device_args(what, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise _lib.S2DError(f"{what}: CUDA tensors expected (no CPU fallback)")
    dev = tensors[0].device
    return _lib.load(), dev, torch._C._cuda_getCurrentRawStream(dev.index)


def _f32c(t):
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def pack_rois(boxes, scores, labels, offsets, cap):
    """the packed first-stage lists (boxes [total, 7 | 9] heading last, scores [total], labels [total] int64; sample b = rows
    offsets[b] .. offsets[b + 1], host ints) as the zero-padded rois [B, cap, 7], roi_scores [B, cap], roi_labels [B, cap] = label + 1
    of `reorder_first_stage_pred_and_feature`, in one launch and without a device read"""
    lib, dev, st = _device_args("pack_rois", boxes, scores, labels)
    bs = len(offsets) - 1
    boxes, scores, labels = _f32c(boxes), _f32c(scores), labels.long().contiguous()
    if int(offsets[-1]) != boxes.shape[0] or scores.shape[0] != boxes.shape[0] or labels.shape[0] != boxes.shape[0]:
        raise _lib.S2DError(f"pack_rois: offsets end at {offsets[-1]}, lists hold {boxes.shape[0]} / {scores.shape[0]} / {labels.shape[0]} rows")
    rois = torch.empty((bs, cap, 7), dtype=torch.float32, device=dev)
    roi_scores = torch.empty((bs, cap), dtype=torch.float32, device=dev)
    roi_labels = torch.empty((bs, cap), dtype=torch.int64, device=dev)
    off = (ctypes.c_int32 * (bs + 1))(*[int(o) for o in offsets])
    _lib.check(lib.s2d_roi_pack(boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), boxes.shape[1] if boxes.dim() == 2 else 7, off, bs, cap,
                                rois.data_ptr(), roi_scores.data_ptr(), roi_labels.data_ptr(), st), "s2d_roi_pack")
    return rois, roi_scores, roi_labels


def roi_bev_features(bev, boxes, row, pc_start, voxel_size, out_stride, num_point=5):
    """BEV features of the boxes named by `row` [B, cap] int32 (rows of the packed list `boxes` [total, 7 | 9], -1 = empty slot ->
    zeros): [B, cap, num_point * C] fp32, the numbers of `box_side_centers` + `BEVFeatureExtractor`.  bev [B, C, H, W] fp32 or bf16 is
    read in place with its own strides (NCHW and channels_last alike; channels_last takes 16-byte loads)."""
    lib, dev, st = _device_args("roi_bev_features", bev, boxes, row)
    if bev.dtype not in (torch.float32, torch.bfloat16):
        bev = bev.float()
    boxes = _f32c(boxes)
    row = row.int().contiguous()
    bs, c, h, w = bev.shape
    if row.dim() != 2 or row.shape[0] != bs:
        raise _lib.S2DError(f"roi_bev_features: row table {tuple(row.shape)} for a map of {bs} samples")
    feats = torch.empty((bs, row.shape[1], num_point * c), dtype=torch.float32, device=dev)
    _lib.check(lib.s2d_roi_bev_features(bev.data_ptr(), int(bev.dtype == torch.bfloat16), bs, c, h, w, *bev.stride(), boxes.data_ptr(), boxes.shape[0],
                                        boxes.shape[1] if boxes.dim() == 2 else 7, row.data_ptr(), row.shape[1], int(num_point), float(pc_start[0]),
                                        float(pc_start[1]), float(voxel_size[0]), float(voxel_size[1]), float(out_stride), feats.data_ptr(), st),
               "s2d_roi_bev_features")
    return feats


def match_rois_to_gt(rois, roi_labels, gt, by_class=True):
    """every RoI's best 3-D IoU with its sample's valid ground truth and that row: (max_iou [B, cap] fp32, assignment [B, cap] int64,
    gt_count [B] int32).  rois [B, cap, 7], roi_labels [B, cap], gt [B, G, >= 8] (box in the first 7 columns, class last; G <=
    ROI_MAX_GT).  What `ProposalTargetLayer.sample_rois_for_rcnn` computes per sample before the sampling, for all samples in one launch."""
    lib, dev, st = _device_args("match_rois_to_gt", rois, roi_labels, gt)
    rois, gt, roi_labels = _f32c(rois), _f32c(gt), roi_labels.long().contiguous()
    bs, cap = roi_labels.shape
    max_iou = torch.empty((bs, cap), dtype=torch.float32, device=dev)
    assignment = torch.empty((bs, cap), dtype=torch.int64, device=dev)
    gt_count = torch.empty((bs,), dtype=torch.int32, device=dev)
    _lib.check(lib.s2d_roi_match_gt(rois.data_ptr(), roi_labels.data_ptr(), bs, cap, gt.data_ptr(), gt.shape[1], gt.shape[2], int(bool(by_class)),
                                    max_iou.data_ptr(), assignment.data_ptr(), gt_count.data_ptr(), st), "s2d_roi_match_gt")
    return max_iou, assignment, gt_count


def roi_targets(idx, rois, roi_labels, roi_scores, max_iou, assignment, gt, sampler_cfg):
    """`ProposalTargetLayer.forward` behind the sampling + `RoIHead.assign_targets` for the sampled slots idx [B, per] (int32): the dict
    of rois, roi_labels, roi_scores, gt_iou_of_rois, gt_of_rois_src, gt_of_rois (encoded), reg_valid_mask, rcnn_cls_labels"""
    lib, dev, st = _device_args("roi_targets", idx, rois, roi_labels, roi_scores, max_iou, assignment, gt)
    kind = _cfg_get(sampler_cfg, "CLS_SCORE_TYPE")
    if kind not in ("cls", "roi_iou"):
        raise NotImplementedError(kind)
    idx = idx.int().contiguous()
    rois, roi_scores, max_iou, gt = _f32c(rois), _f32c(roi_scores), _f32c(max_iou), _f32c(gt)
    roi_labels, assignment = roi_labels.long().contiguous(), assignment.long().contiguous()
    bs, per = idx.shape
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    l = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)
    out = dict(rois=f(bs, per, rois.shape[-1]), roi_labels=l(bs, per), roi_scores=f(bs, per), gt_iou_of_rois=f(bs, per), gt_of_rois_src=f(bs, per, 8),
               gt_of_rois=f(bs, per, 8), reg_valid_mask=l(bs, per), rcnn_cls_labels=f(bs, per) if kind == "roi_iou" else l(bs, per))
    _lib.check(lib.s2d_roi_targets(idx.data_ptr(), bs, per, rois.shape[1], rois.shape[-1], rois.data_ptr(), roi_labels.data_ptr(), roi_scores.data_ptr(),
                                   max_iou.data_ptr(), assignment.data_ptr(), gt.data_ptr(), gt.shape[1], gt.shape[2],
                                   float(_cfg_get(sampler_cfg, "REG_FG_THRESH")), float(_cfg_get(sampler_cfg, "CLS_FG_THRESH")),
                                   float(_cfg_get(sampler_cfg, "CLS_BG_THRESH")), int(kind == "roi_iou"), out["rois"].data_ptr(),
                                   out["roi_labels"].data_ptr(), out["roi_scores"].data_ptr(), out["gt_iou_of_rois"].data_ptr(),
                                   out["gt_of_rois_src"].data_ptr(), out["gt_of_rois"].data_ptr(), out["reg_valid_mask"].data_ptr(),
                                   out["rcnn_cls_labels"].data_ptr(), st), "s2d_roi_targets")
    return out


def refine_rois(rois, roi_scores, roi_labels, rcnn_cls, rcnn_reg):
    """`RoIHead.generate_predicted_boxes` + the arithmetic of `TwoStageDetector.post_process`: (boxes [B, cap, 7], scores [B, cap] =
    sqrt(sigmoid(cls) * roi_score), labels [B, cap] = roi_label - 1).  The caller slices every sample to its first count_b slots."""
    lib, dev, st = _device_args("refine_rois", rois, roi_scores, roi_labels, rcnn_cls, rcnn_reg)
    bs, cap = roi_labels.shape
    rois, roi_scores, roi_labels = _f32c(rois), _f32c(roi_scores), roi_labels.long().contiguous()
    rcnn_cls, rcnn_reg = _f32c(rcnn_cls.detach()), _f32c(rcnn_reg.detach())
    if rois.shape[-1] != 7 or rcnn_reg.numel() != bs * cap * 7 or rcnn_cls.numel() != bs * cap:
        raise _lib.S2DError(f"refine_rois: rois {tuple(rois.shape)}, rcnn_cls {tuple(rcnn_cls.shape)}, rcnn_reg {tuple(rcnn_reg.shape)} (code size 7, one class)")
    boxes = torch.empty((bs, cap, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((bs, cap), dtype=torch.float32, device=dev)
    labels = torch.empty((bs, cap), dtype=torch.int64, device=dev)
    _lib.check(lib.s2d_roi_refine(rois.data_ptr(), roi_scores.data_ptr(), roi_labels.data_ptr(), rcnn_cls.data_ptr(), rcnn_reg.data_ptr(), bs * cap,
                                  boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), st), "s2d_roi_refine")
    return boxes, scores, labels


def _mlp_chain(seq):
    """the (conv, batch norm | None) pairs of one of RoIHead's nn.Sequential's, or None when it holds anything but
    Conv1d(kernel_size=1) [+ BatchNorm1d + ReLU] [+ Dropout] groups"""
    out, mods, i = [], list(seq), 0
    while i < len(mods):
        conv = mods[i]
        if not isinstance(conv, nn.Conv1d) or conv.kernel_size != (1,) or conv.stride != (1,) or conv.groups != 1 or conv.padding not in ((0,), "valid"):
            return None
        i += 1
        bn = None
        if i < len(mods) and isinstance(mods[i], nn.BatchNorm1d):
            bn = mods[i]
            if i + 1 >= len(mods) or not isinstance(mods[i + 1], nn.ReLU) or bn.running_mean is None or bn.weight is None:
                return None
            i += 2
        if i < len(mods) and isinstance(mods[i], nn.Dropout):
            i += 1
        out.append((conv, bn))
    return out


def _mlp_affine(conv, bn):
    """(scale, shift) of y = act(scale * (x . W^T) + shift): eval batch norm behind the convolution, or the convolution's own bias"""
    if bn is None:
        scale = torch.ones_like(conv.weight[:, 0, 0])
        return scale, (conv.bias if conv.bias is not None else torch.zeros_like(scale))
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    mean = bn.running_mean if conv.bias is None else bn.running_mean - conv.bias
    return scale, bn.bias - mean * scale


def roi_mlp_reference(head, feats):
    """The eval-mode MLP of `head` (a RoIHead) restated from its parameters: feats [..., cin] -> (rcnn_cls [R, num_class], rcnn_reg [R,
    code_size]), R = the product of the leading dimensions.  Every layer is act(scale * F.linear(x, W) + shift) with scale = gamma /
    sqrt(running_var + eps), shift = beta - running_mean * scale behind a batch norm and scale = 1, shift = bias on the two final
    convolutions; dropout is the identity.  Any dtype (the parameters' and the features' must agree), any device: this is the definition
    csrc/roi_mlp.hip implements, and in float64 the oracle it is tested against."""
    def run(seq, x):
        chain = _mlp_chain(seq)
        if chain is None:
            raise NotImplementedError("roi_mlp_reference: a chain of Conv1d(kernel_size=1) [+ BatchNorm1d + ReLU] groups expected")
        for conv, bn in chain:
            scale, shift = _mlp_affine(conv, bn)
            x = F.linear(x, conv.weight.squeeze(-1)) * scale + shift
            if bn is not None:
                x = F.relu(x)
        return x
    with torch.no_grad():
        shared = run(head.shared_fc_layer, feats.reshape(-1, feats.shape[-1]))
        return run(head.cls_layers, shared), run(head.reg_layers, shared)


ROI_MLP_MAX_CIN, ROI_MLP_MAX_WIDTH = 4096, 256   # s2d_roi_mlp_supported


def roi_mlp_fused(head, feats):
    """(rcnn_cls [R, 1], rcnn_reg [R, 7]) of feats [..., cin] through the fused kernel of csrc/roi_mlp.hip - what
    RoIHead.forward(training=False, device=True) runs.  Raises with `head.mlp_reason(feats)` when the kernel does not apply: no fallback."""
    reason, spec = head._mlp_check(feats)
    if reason is not None:
        raise _lib.S2DError(f"roi_mlp_fused: {reason}")
    return head._mlp_fused(feats, spec)


# ---- the training branch of the RoI MLP: float64 definitions, then the kernels of csrc/roi_mlp_train.hip ---------------------------------
ROI_MLP_TRAIN_ROWS = (2, 8192)   # s2d_roi_mlp_train_supported


def _mlp_dropouts(seq):
    """the nn.Dropout behind each (conv, batch norm) group of `_mlp_chain(seq)`, or None where the module has none: the dropout sites are
    the module's own (RoIHead.__init__ / make_fc_layers, with the reference's `dp_ratio >= 0` / `> 0` asymmetry)"""
    out, mods = [], list(seq)
    for i, m in enumerate(mods):
        if isinstance(m, nn.Conv1d):
            j = i + 1
            while j < len(mods) and isinstance(mods[j], (nn.BatchNorm1d, nn.ReLU)):
                j += 1
            out.append(mods[j] if j < len(mods) and isinstance(mods[j], nn.Dropout) else None)
    return out


def roi_mlp_train_sites(head):
    """[(width, p)] of the dropout sites of `head` in the order shared, cls, reg - the order of the `masks` of the functions below"""
    sites = []
    for seq in (head.shared_fc_layer, head.cls_layers, head.reg_layers):
        for (conv, _), dp in zip(_mlp_chain(seq), _mlp_dropouts(seq)):
            if dp is not None:
                sites.append((conv.out_channels, dp.p))
    return sites


def roi_mlp_train_reference(head, feats, masks=None):
    """The TRAINING-mode MLP of `head` restated from its parameters: feats [..., cin] -> (rcnn_cls [R, 1], rcnn_reg [R, code], stats).
    A hidden layer is z = a . W^T, mean and biased variance of z over the R rows, y = gamma * (z - mean) / sqrt(var + eps) + beta,
    a' = relu(y), and behind a dropout site a' = a' * mask / (1 - p) with the caller's 0/1 mask [R, width] of that site (`masks`: one per
    site in the order of `roi_mlp_train_sites`; None = no dropout).  The final layers carry their bias.  Differentiable by autograd;
    `stats` = per hidden layer (shared, cls, reg) the batch mean and the UNBIASED variance the running statistics move toward (detached).
    Does not touch the running statistics.  Any dtype: in float64 the oracle csrc/roi_mlp_train.hip is tested against."""
    stats, site = [], [0]

    def run(seq, x):
        chain = _mlp_chain(seq)
        if chain is None:
            raise NotImplementedError("roi_mlp_train_reference: a chain of Conv1d(kernel_size=1) [+ BatchNorm1d + ReLU] groups expected")
        for (conv, bn), dp in zip(chain, _mlp_dropouts(seq)):
            z = F.linear(x, conv.weight.squeeze(-1), conv.bias)
            if bn is None:
                x = z
                continue
            mean, var = z.mean(dim=0), z.var(dim=0, unbiased=False)
            stats.append((mean.detach(), z.var(dim=0, unbiased=True).detach()))
            x = F.relu(bn.weight * (z - mean) / torch.sqrt(var + bn.eps) + bn.bias)
            if dp is not None:
                if masks is not None:
                    x = x * masks[site[0]].to(x) / (1 - dp.p)
                site[0] += 1
        return x
    shared = run(head.shared_fc_layer, feats.reshape(-1, feats.shape[-1]))
    return run(head.cls_layers, shared), run(head.reg_layers, shared), stats


class _BceOfSigmoid(torch.autograd.Function):
    """F.binary_cross_entropy(sigmoid(x), y, reduction="none") as torch computes it and differentiates it: logarithms clamped at -100
    forward; (p - y) / max(p (1 - p), 1e-12) * p (1 - p) backward - zero where the sigmoid has saturated, not 0 * inf"""
    @staticmethod
    def forward(ctx, x, y):
        p = torch.sigmoid(x)
        ctx.save_for_backward(p, y)
        return -(y * torch.clamp(torch.log(p), min=-100.0) + (1 - y) * torch.clamp(torch.log(1 - p), min=-100.0))

    @staticmethod
    def backward(ctx, g):
        p, y = ctx.saved_tensors
        v = p * (1 - p)
        return g * (p - y) / torch.clamp(v, min=1e-12) * v, None


def _loss_cfg(loss_cfg):
    w = _cfg_get(loss_cfg, "LOSS_WEIGHTS")
    if _cfg_get(loss_cfg, "CLS_LOSS") != "BinaryCrossEntropy" or _cfg_get(loss_cfg, "REG_LOSS") != "L1":
        raise NotImplementedError(f"RoI losses {_cfg_get(loss_cfg, 'CLS_LOSS')} / {_cfg_get(loss_cfg, 'REG_LOSS')} (BinaryCrossEntropy and L1 only)")
    return [float(c) for c in w["code_weights"]], float(w["rcnn_cls_weight"]), float(w["rcnn_reg_weight"])


def roi_loss_reference(rcnn_cls, rcnn_reg, cls_labels, reg_valid_mask, gt_of_rois, loss_cfg):
    """(loss_cls, loss_reg) of RoIHead.get_box_cls_layer_loss (BinaryCrossEntropy) and get_box_reg_layer_loss (L1) as torch computes them,
    in the dtype of the predictions: p = sigmoid(x), per row -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) masked by label >= 0
    and divided by clamp(valid, min=1); |reg - target| times code_weights masked by reg_valid_mask > 0 and divided by max(fg, 1); each
    times its weight.  Labels may be soft (roi_iou) or hard with -1."""
    code_weights, w_cls, w_reg = _loss_cfg(loss_cfg)
    x = rcnn_cls.reshape(-1)
    y = cls_labels.reshape(-1).to(x.dtype)
    valid = (y >= 0).to(x.dtype)
    loss_cls = (_BceOfSigmoid.apply(x, y) * valid).sum() / torch.clamp(valid.sum(), min=1.0) * w_cls
    code = rcnn_reg.shape[-1]
    fg = (reg_valid_mask.reshape(-1) > 0).to(x.dtype)
    target = gt_of_rois[..., 0:code].reshape(-1, code).to(x.dtype)
    l1 = (rcnn_reg.reshape(-1, code) - target).abs() * rcnn_reg.new_tensor(code_weights[:code])
    loss_reg = (l1 * fg.unsqueeze(-1)).sum() / torch.clamp(fg.sum(), min=1.0) * w_reg
    return loss_cls, loss_reg


def _roi_train_workspace(floats, dev):
    """the scratch that carries z, the statistics and the backward sums from s2d_roi_mlp_train_forward to _backward: uninitialised - every
    word is written before it is read (tests replace this to fill it with NaN)"""
    return torch.empty((floats,), dtype=torch.float32, device=dev)


class _RoiMlpTrain(torch.autograd.Function):
    """csrc/roi_mlp_train.hip: s2d_roi_mlp_train_forward / _backward.  Inputs behind `mask` are the parameters in the order of the plan's
    layer table: weight, then (gamma, beta) of a hidden layer or the bias of a final one."""
    @staticmethod
    def forward(ctx, head, spec, x, mask, *params):
        lib, dev, st = _device_args("roi_mlp_train", x)
        plan, packed, _ = head._mlp_images(spec, dev, affine=False)
        rows = x.shape[0]
        args = _lib.RoiMlpTrainArgs()
        drops = [d for seq in (head.shared_fc_layer, head.cls_layers, head.reg_layers) for d in _mlp_dropouts(seq)]
        at, k = 0, 0
        for l, ((conv, bn), dp) in enumerate(zip(spec[4], drops)):
            a = args.layer[l]
            a.weight = params[k].data_ptr()
            if bn is None:
                a.bias, k = params[k + 1].data_ptr(), k + 2
                continue
            a.gamma, a.beta, k = params[k + 1].data_ptr(), params[k + 2].data_ptr(), k + 3
            a.running_mean, a.running_var, a.momentum, a.eps, a.keep_scale = bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.momentum, bn.eps, 1.0
            if dp is not None and dp.p > 0:
                a.mask, a.keep_scale = mask.data_ptr() + at, 1.0 / (1.0 - dp.p)
                at += rows * conv.out_channels
        nbytes = lib.s2d_roi_mlp_train_scratch_bytes(ctypes.byref(plan), rows)
        ws = _roi_train_workspace(nbytes // 4, dev)
        rcnn_cls = torch.empty((rows, 1), dtype=torch.float32, device=dev)
        rcnn_reg = torch.empty((rows, 7), dtype=torch.float32, device=dev)
        _lib.check(lib.s2d_roi_mlp_train_forward(ctypes.byref(plan), ctypes.byref(args), x.data_ptr(), rows, packed.data_ptr(), ws.data_ptr(), nbytes,
                                                 rcnn_cls.data_ptr(), rcnn_reg.data_ptr(), st), "s2d_roi_mlp_train_forward")
        # the call is counted as torch.batch_norm counts it: an ordinary in-place add, which moves the version `_mlp_images` keys its
        # scale / shift vector on (the running statistics above were written through raw pointers)
        torch._foreach_add_([bn.num_batches_tracked for _, bn in spec[4] if bn is not None], 1)
        ctx.save_for_backward(x, mask, *params)
        ctx.plan, ctx.args, ctx.ws, ctx.nbytes = plan, args, ws, nbytes
        return rcnn_cls, rcnn_reg

    @staticmethod
    def backward(ctx, d_cls, d_reg):
        x, mask, *params = ctx.saved_tensors
        lib, dev, st = _device_args("roi_mlp_train", x)
        rows = x.shape[0]
        d_cls = torch.zeros((rows, 1), dtype=torch.float32, device=dev) if d_cls is None else _f32c(d_cls)
        d_reg = torch.zeros((rows, 7), dtype=torch.float32, device=dev) if d_reg is None else _f32c(d_reg)
        flat = torch.empty((sum(p.numel() for p in params),), dtype=torch.float32, device=dev)   # every element is written by its one owner
        grads = [g.view(p.shape) for g, p in zip(flat.split([p.numel() for p in params]), params)]
        args, k = ctx.args, 0
        for l in range(ctx.plan.num_layers):
            a = args.layer[l]
            a.d_weight = grads[k].data_ptr()
            if a.bias:
                a.d_bias, k = grads[k + 1].data_ptr(), k + 2
            else:
                a.d_gamma, a.d_beta, k = grads[k + 1].data_ptr(), grads[k + 2].data_ptr(), k + 3
        _lib.check(lib.s2d_roi_mlp_train_backward(ctypes.byref(ctx.plan), ctypes.byref(args), x.data_ptr(), rows, ctx.ws.data_ptr(), ctx.nbytes,
                                                  d_cls.data_ptr(), d_reg.data_ptr(), st), "s2d_roi_mlp_train_backward")
        return (None, None, None, None, *grads)


def roi_mlp_train_fused(head, feats, masks=None):
    """(rcnn_cls [R, 1], rcnn_reg [R, 7]) of feats [..., cin] through the TRAINING branch on the kernels of csrc/roi_mlp_train.hip, with a
    grad_fn: gradients flow to every convolution weight, gamma, beta and the two final biases; the features get none (S2DError if they
    require one).  Moves the running statistics and num_batches_tracked like the module's own training forward.  No host read and no
    blocking call from the first forward launch to the last backward launch.  `masks`: one 0/1 tensor [R, width] per dropout site in the
    order of `roi_mlp_train_sites`.  None: all sites' masks are drawn in ONE call from torch's current CUDA generator (`bernoulli_(1 - p)`
    on one flat uint8 buffer), so the same seed gives the same masks - NOT the bits F.dropout would draw for that seed: the same
    distribution from a different stream.  Raises with `head.train_mlp_reason(feats)` when the kernels do not apply: no fallback."""
    reason, spec = head._train_mlp_check(feats)
    if reason is not None:
        raise _lib.S2DError(f"roi_mlp_train_fused: {reason}")
    x = feats.detach().reshape(-1, feats.shape[-1])
    x = x if x.is_contiguous() else x.contiguous()
    rows = x.shape[0]
    sites = [(w, p) for w, p in roi_mlp_train_sites(head) if p > 0]
    if not sites:
        mask = torch.empty((0,), dtype=torch.uint8, device=x.device)
    elif masks is None:
        if len({p for _, p in sites}) != 1:
            raise _lib.S2DError("roi_mlp_train_fused: dropout sites of different ratios need caller-supplied masks")
        mask = torch.empty((rows * sum(w for w, _ in sites),), dtype=torch.uint8, device=x.device).bernoulli_(1.0 - sites[0][1])
    else:
        given = [m for m, (_, p) in zip(masks, roi_mlp_train_sites(head)) if p > 0]
        if len(masks) != len(roi_mlp_train_sites(head)) or any(tuple(m.shape) != (rows, w) for m, (w, _) in zip(given, sites)):
            raise _lib.S2DError(f"roi_mlp_train_fused: masks of shapes {[(rows, w) for w, _ in roi_mlp_train_sites(head)]} expected")
        mask = torch.cat([(m != 0).to(torch.uint8).reshape(-1) for m in given]).to(x.device)
    params = [t for conv, bn in spec[4] for t in ((conv.weight, conv.bias) if bn is None else (conv.weight, bn.weight, bn.bias))]
    return _RoiMlpTrain.apply(head, spec, x, mask, *params)


class _RoiLoss(torch.autograd.Function):
    """csrc/roi_mlp_train.hip: s2d_roi_loss_forward / _backward.  One launch each; the valid and foreground counts stay on the device."""
    @staticmethod
    def forward(ctx, cls, reg, labels, fg, target, code_weights, w_cls, w_reg):
        lib, dev, st = _device_args("roi_loss", cls, reg, labels, fg, target)
        out = torch.empty((4,), dtype=torch.float32, device=dev)
        cw = (ctypes.c_float * 7)(*code_weights)
        _lib.check(lib.s2d_roi_loss_forward(cls.data_ptr(), reg.data_ptr(), labels.data_ptr(), fg.data_ptr(), target.data_ptr(), cls.numel(), cw, w_cls,
                                            w_reg, out.data_ptr(), st), "s2d_roi_loss_forward")
        ctx.save_for_backward(cls, reg, labels, fg, target, out)
        ctx.cfg = (cw, w_cls, w_reg)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_cls, g_reg):
        cls, reg, labels, fg, target, out = ctx.saved_tensors
        lib, dev, st = _device_args("roi_loss", cls)
        zero = None
        if g_cls is None or g_reg is None:
            zero = torch.zeros((), dtype=torch.float32, device=dev)
        g_cls, g_reg = (zero if g is None else _f32c(g) for g in (g_cls, g_reg))
        d_cls, d_reg = torch.empty_like(cls), torch.empty_like(reg)
        cw, w_cls, w_reg = ctx.cfg
        _lib.check(lib.s2d_roi_loss_backward(cls.data_ptr(), reg.data_ptr(), labels.data_ptr(), fg.data_ptr(), target.data_ptr(), cls.numel(), cw, w_cls,
                                             w_reg, out.data_ptr(), g_cls.data_ptr(), g_reg.data_ptr(), d_cls.data_ptr(), d_reg.data_ptr(), st),
                   "s2d_roi_loss_backward")
        return d_cls, d_reg, None, None, None, None, None, None


def roi_loss_fused(rcnn_cls, rcnn_reg, cls_labels, reg_valid_mask, gt_of_rois, loss_cfg):
    """`roi_loss_reference` on the kernels of csrc/roi_mlp_train.hip: (loss_cls, loss_reg), device scalars with a grad_fn; one launch
    forward and one backward, no host read (the valid and foreground counts stay on the device).  fp32 CUDA tensors, code size 7."""
    try:
        code_weights, w_cls, w_reg = _loss_cfg(loss_cfg)
    except NotImplementedError as e:
        raise _lib.S2DError(f"roi_loss_fused: {e}")
    if rcnn_reg.shape[-1] != 7 or len(code_weights) < 7 or rcnn_cls.numel() * 7 != rcnn_reg.numel() or rcnn_cls.numel() == 0:
        raise _lib.S2DError(f"roi_loss_fused: rcnn_cls {tuple(rcnn_cls.shape)}, rcnn_reg {tuple(rcnn_reg.shape)} (one class, code size 7)")
    if rcnn_cls.dtype != torch.float32 or rcnn_reg.dtype != torch.float32:
        raise _lib.S2DError(f"roi_loss_fused: predictions of dtype {rcnn_cls.dtype} / {rcnn_reg.dtype}")
    rows = rcnn_cls.numel()
    cls = rcnn_cls.reshape(rows, 1)
    reg = rcnn_reg.reshape(rows, 7)
    with torch.no_grad():
        labels, fg = _f32c(cls_labels.reshape(rows)), _f32c(reg_valid_mask.reshape(rows))
        target = _f32c(gt_of_rois[..., 0:7].reshape(rows, 7))
    return _RoiLoss.apply(cls if cls.is_contiguous() else cls.contiguous(), reg if reg.is_contiguous() else reg.contiguous(), labels, fg, target,
                          code_weights[:7], w_cls, w_reg)


class ProposalTargetLayer(nn.Module):
    """IoU-based sampling of the first stage's RoIs and their classification / regression labels
    (proposal_target_layer.py).  The random draws are the reference's (np.random.permutation / np.random.rand on the host,
    torch.randint on the CPU generator), so a seeded run samples the same RoIs."""

    def __init__(self, roi_sampler_cfg, iou_fn=None):
        super().__init__()
        self.cfg = roi_sampler_cfg
        self.iou_fn = iou_fn or boxes_iou3d

    def _c(self, key, default=None):
        return _cfg_get(self.cfg, key, default)

    def forward(self, batch_dict):
        rois, gt_of_rois, ious, scores, labels, feats = self.sample_rois_for_rcnn(batch_dict)
        reg_valid_mask = (ious > self._c("REG_FG_THRESH")).long()
        kind = self._c("CLS_SCORE_TYPE")
        if kind == "cls":
            cls_labels = (ious > self._c("CLS_FG_THRESH")).long()
            ignore = (ious > self._c("CLS_BG_THRESH")) & (ious < self._c("CLS_FG_THRESH"))
            cls_labels[ignore > 0] = -1
        elif kind == "roi_iou":
            bg, fg = self._c("CLS_BG_THRESH"), self._c("CLS_FG_THRESH")
            fg_mask, bg_mask = ious > fg, ious < bg
            interval = (fg_mask == 0) & (bg_mask == 0)
            cls_labels = (fg_mask > 0).float()
            cls_labels[interval] = (ious[interval] - bg) / (fg - bg)
        else:
            raise NotImplementedError(kind)
        return dict(rois=rois, gt_of_rois=gt_of_rois, gt_iou_of_rois=ious, roi_scores=scores, roi_labels=labels, roi_features=feats,
                    reg_valid_mask=reg_valid_mask, rcnn_cls_labels=cls_labels)

    def sample_rois_for_rcnn(self, batch_dict):
        bs, per = batch_dict["batch_size"], self._c("ROI_PER_IMAGE")
        rois, roi_scores, roi_labels = batch_dict["rois"], batch_dict["roi_scores"], batch_dict["roi_labels"]
        gt_boxes, roi_features = batch_dict["gt_boxes_and_cls"], batch_dict["roi_features"]
        code = rois.shape[-1]
        out_rois, out_gt = rois.new_zeros(bs, per, code), rois.new_zeros(bs, per, code + 1)
        out_iou, out_scores = rois.new_zeros(bs, per), rois.new_zeros(bs, per)
        out_labels = rois.new_zeros((bs, per), dtype=torch.long)
        out_feats = roi_features.new_zeros(bs, per, roi_features.shape[-1])
        for i in range(bs):
            cur_gt = gt_boxes[i]
            k = len(cur_gt) - 1
            rowsum = cur_gt.sum(-1).tolist()                    # the reference walks back over the zero padding rows (sum == 0)
            while k > 0 and rowsum[k] == 0:
                k -= 1
            cur_gt = cur_gt[:k + 1]
            cur_gt = cur_gt.new_zeros((1, cur_gt.shape[1])) if len(cur_gt) == 0 else cur_gt
            if self._c("SAMPLE_ROI_BY_EACH_CLASS", False):
                max_overlaps, assignment = self.get_max_iou_with_same_class(rois[i][:, :7], roi_labels[i], cur_gt[:, 0:7], cur_gt[:, -1].long())
            else:
                max_overlaps, assignment = torch.max(self.iou_fn(rois[i], cur_gt[:, 0:7]), dim=1)
            idx = self.subsample_rois(max_overlaps)
            out_rois[i], out_labels[i], out_iou[i], out_scores[i] = rois[i][idx], roi_labels[i][idx], max_overlaps[idx], roi_scores[i][idx]
            out_gt[i], out_feats[i] = cur_gt[assignment[idx]], roi_features[i][idx]
        return out_rois, out_gt, out_iou, out_scores, out_labels, out_feats

    def subsample_rois(self, max_overlaps):
        per = self._c("ROI_PER_IMAGE")
        fg_per = int(np.round(self._c("FG_RATIO") * per))
        fg_thresh = min(self._c("REG_FG_THRESH"), self._c("CLS_FG_THRESH"))
        fg = (max_overlaps >= fg_thresh).nonzero().view(-1)
        easy = (max_overlaps < self._c("CLS_BG_THRESH_LO")).nonzero().view(-1)
        hard = ((max_overlaps < self._c("REG_FG_THRESH")) & (max_overlaps >= self._c("CLS_BG_THRESH_LO"))).nonzero().view(-1)
        n_fg, n_bg = fg.numel(), hard.numel() + easy.numel()
        if n_fg > 0 and n_bg > 0:
            take = min(fg_per, n_fg)
            perm = torch.from_numpy(np.random.permutation(n_fg)).to(max_overlaps.device).long()
            fg = fg[perm[:take]]
            bg = self.sample_bg_inds(hard, easy, per - take, self._c("HARD_BG_RATIO"))
        elif n_fg > 0:
            draw = torch.from_numpy(np.floor(np.random.rand(per) * n_fg)).to(max_overlaps.device).long()
            fg = fg[draw]
            bg = fg.new_zeros(0)
        elif n_bg > 0:
            bg = self.sample_bg_inds(hard, easy, per, self._c("HARD_BG_RATIO"))
        else:
            raise NotImplementedError(f"ProposalTargetLayer: no RoI to sample (max IoU in [{float(max_overlaps.min())}, {float(max_overlaps.max())}])")
        return torch.cat((fg, bg), dim=0)

    def subsample_rois_host(self, max_overlaps):
        """`subsample_rois` + `sample_bg_inds` on a host array [n] (fp32): the SAME draws in the same order (np.random.permutation,
        np.random.rand, torch.randint on the CPU generator), so a seeded run samples the RoIs the torch chain samples.  Returns int64
        indices [ROI_PER_IMAGE] (numpy)."""
        mo = np.asarray(max_overlaps, dtype=np.float32)
        f = np.float32   # python scalars meet an fp32 tensor as their fp32 rounding
        per = self._c("ROI_PER_IMAGE")
        fg_per = int(np.round(self._c("FG_RATIO") * per))
        fg_thresh = min(self._c("REG_FG_THRESH"), self._c("CLS_FG_THRESH"))
        fg = np.nonzero(mo >= f(fg_thresh))[0]
        easy = np.nonzero(mo < f(self._c("CLS_BG_THRESH_LO")))[0]
        hard = np.nonzero((mo < f(self._c("REG_FG_THRESH"))) & (mo >= f(self._c("CLS_BG_THRESH_LO"))))[0]

        def draw(n, k):
            return torch.randint(low=0, high=n, size=(k,)).long().numpy()

        def sample_bg(count):
            ratio = self._c("HARD_BG_RATIO")
            if len(hard) > 0 and len(easy) > 0:
                n_hard = min(int(count * ratio), len(hard))
                h = hard[draw(len(hard), n_hard)]
                return np.concatenate([h, easy[draw(len(easy), count - n_hard)]])
            if len(hard) > 0:
                return hard[draw(len(hard), count)]
            if len(easy) > 0:
                return easy[draw(len(easy), count)]
            raise NotImplementedError

        n_fg, n_bg = len(fg), len(hard) + len(easy)
        bg = fg[:0]
        if n_fg > 0 and n_bg > 0:
            take = min(fg_per, n_fg)
            fg = fg[np.random.permutation(n_fg)[:take]]
            bg = sample_bg(per - take)
        elif n_fg > 0:
            fg = fg[np.floor(np.random.rand(per) * n_fg).astype(np.int64)]
        elif n_bg > 0:
            fg, bg = fg[:0], sample_bg(per)
        else:
            raise NotImplementedError(f"ProposalTargetLayer: no RoI to sample (max IoU in [{float(mo.min())}, {float(mo.max())}])")
        return np.concatenate([fg, bg]).astype(np.int64)

    @staticmethod
    def sample_bg_inds(hard, easy, count, hard_ratio):
        draw = lambda n, k: torch.randint(low=0, high=n, size=(k,)).long()    # CPU generator, as in the reference
        if hard.numel() > 0 and easy.numel() > 0:
            n_hard = min(int(count * hard_ratio), len(hard))
            h = hard[draw(hard.numel(), n_hard).to(hard.device)]
            e = easy[draw(easy.numel(), count - n_hard).to(easy.device)]
            return torch.cat([h, e], dim=0)
        if hard.numel() > 0:
            return hard[draw(hard.numel(), count).to(hard.device)]
        if easy.numel() > 0:
            return easy[draw(easy.numel(), count).to(easy.device)]
        raise NotImplementedError

    def get_max_iou_with_same_class(self, rois, roi_labels, gt_boxes, gt_labels):
        max_overlaps = rois.new_zeros(rois.shape[0])
        assignment = roi_labels.new_zeros(roi_labels.shape[0])
        for k in range(int(gt_labels.min()), int(gt_labels.max()) + 1):
            rm, gm = roi_labels == k, gt_labels == k
            if rm.sum() > 0 and gm.sum() > 0:
                orig = gm.nonzero().view(-1)
                cur_max, cur_arg = torch.max(self.iou_fn(rois[rm], gt_boxes[gm]), dim=1)
                max_overlaps[rm] = cur_max
                assignment[rm] = orig[cur_arg]
        return max_overlaps, assignment


@ROI_HEAD.register_module
class RoIHead(nn.Module):
    def __init__(self, input_channels, model_cfg, num_class=1, code_size=7, test_cfg=None):
        super().__init__()
        self.model_cfg, self.num_class, self.code_size, self.test_cfg = model_cfg, num_class, code_size, test_cfg
        dp = _cfg_get(model_cfg, "DP_RATIO")
        shared, pre = [], input_channels
        fcs = list(_cfg_get(model_cfg, "SHARED_FC"))
        for k, c in enumerate(fcs):
            shared += [nn.Conv1d(pre, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            pre = c
            if k != len(fcs) - 1 and dp > 0:
                shared.append(nn.Dropout(dp))
        self.shared_fc_layer = nn.Sequential(*shared)
        self.cls_layers = self.make_fc_layers(pre, self.num_class, list(_cfg_get(model_cfg, "CLS_FC")), dp)
        self.reg_layers = self.make_fc_layers(pre, code_size, list(_cfg_get(model_cfg, "REG_FC")), dp)
        for m in self.modules():   # init_weights('xavier')
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.xavier_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)
        target_cfg = _cfg_get(model_cfg, "TARGET_CONFIG", None)
        self.proposal_target_layer = ProposalTargetLayer(target_cfg) if target_cfg else None   # no parameters: state_dict unchanged
        self.forward_ret_dict = None
        self.mlp_paths = {"fused": 0, "torch": 0}   # calls of forward() by the path their MLP took
        self._mlp_cache = None                      # the fused kernel's layer table, packed weight image and scale / shift vector
        self.fused_training = False                 # opt-in: forward(training=True, device=True) and get_loss on csrc/roi_mlp_train.hip
        self.train_paths = {"fused": 0, "torch": 0}   # calls of forward(training=True) by the path their MLP took
        self.train_reason = None                    # why the last training forward with fused_training set kept the torch chain

    def assign_targets(self, batch_dict):
        """sampled RoIs + their ground-truth boxes encoded in the RoI's frame (roi_head_template.py:43-92)"""
        if self.proposal_target_layer is None:
            raise ValueError("RoIHead: model_cfg.TARGET_CONFIG is required for training")
        bs = batch_dict["batch_size"]
        with torch.no_grad():
            t = self.proposal_target_layer(batch_dict)
        rois, gt = t["rois"], t["gt_of_rois"]
        t["gt_of_rois_src"] = gt.clone().detach()
        roi_ry = limit_period(rois[:, :, 6], offset=0.5, period=np.pi * 2)
        gt[:, :, :6] = gt[:, :, :6] - rois[:, :, :6]
        gt[:, :, 6] = gt[:, :, 6] - roi_ry
        gt = rotate_points_along_z(gt.view(-1, 1, gt.shape[-1]), -roi_ry.view(-1)).view(bs, -1, gt.shape[-1])
        if rois.shape[-1] == 9:
            gt[:, :, 7:-1] = gt[:, :, 7:-1] - rois[:, :, 7:]
        heading = gt[:, :, 6] % (2 * np.pi)                                  # flip when the RoI points the other way
        opposite = (heading > np.pi * 0.5) & (heading < np.pi * 1.5)
        heading[opposite] = (heading[opposite] + np.pi) % (2 * np.pi)
        flag = heading > np.pi
        heading[flag] = heading[flag] - np.pi * 2
        gt[:, :, 6] = torch.clamp(heading, min=-np.pi / 2, max=np.pi / 2)
        t["gt_of_rois"] = gt
        return t

    def get_box_reg_layer_loss(self, ret):
        cfg = _cfg_get(self.model_cfg, "LOSS_CONFIG")
        if _cfg_get(cfg, "REG_LOSS") != "L1":
            raise NotImplementedError(_cfg_get(cfg, "REG_LOSS"))
        weights = _cfg_get(cfg, "LOSS_WEIGHTS")
        code = ret["rcnn_reg"].shape[-1]
        fg = ret["reg_valid_mask"].view(-1) > 0
        target = ret["gt_of_rois"][..., 0:code].reshape(-1, code)
        loss = F.l1_loss(ret["rcnn_reg"].view(target.shape[0], -1), target, reduction="none")
        loss = loss * loss.new_tensor(weights["code_weights"])
        loss = (loss * fg.unsqueeze(-1).float()).sum() / max(int(fg.long().sum().item()), 1)
        loss = loss * weights["rcnn_reg_weight"]
        return loss, {"rcnn_loss_reg": loss.detach()}

    def get_box_cls_layer_loss(self, ret):
        cfg = _cfg_get(self.model_cfg, "LOSS_CONFIG")
        labels = ret["rcnn_cls_labels"].view(-1)
        kind = _cfg_get(cfg, "CLS_LOSS")
        if kind == "BinaryCrossEntropy":
            per = F.binary_cross_entropy(torch.sigmoid(ret["rcnn_cls"].view(-1)), labels.float(), reduction="none")
        elif kind == "CrossEntropy":
            per = F.cross_entropy(ret["rcnn_cls"], labels, reduction="none", ignore_index=-1)
        else:
            raise NotImplementedError(kind)
        valid = (labels >= 0).float()
        loss = (per * valid).sum() / torch.clamp(valid.sum(), min=1.0)
        loss = loss * _cfg_get(cfg, "LOSS_WEIGHTS")["rcnn_cls_weight"]
        return loss, {"rcnn_loss_cls": loss.detach()}

    def get_loss(self, tb_dict=None):
        tb = {} if tb_dict is None else tb_dict
        ret = self.forward_ret_dict
        if ret.get("fused_training"):   # both losses in one launch, their backward in one more; the counts stay on the device
            cls, reg = roi_loss_fused(ret["rcnn_cls"], ret["rcnn_reg"], ret["rcnn_cls_labels"], ret["reg_valid_mask"], ret["gt_of_rois"],
                                      _cfg_get(self.model_cfg, "LOSS_CONFIG"))
            c, r = {"rcnn_loss_cls": cls.detach()}, {"rcnn_loss_reg": reg.detach()}
        else:
            cls, c = self.get_box_cls_layer_loss(ret)
            reg, r = self.get_box_reg_layer_loss(ret)
        tb.update(c); tb.update(r)
        total = cls + reg
        tb["rcnn_loss"] = total.item()
        return total, tb

    @staticmethod
    def make_fc_layers(input_channels, output_channels, fc_list, dp_ratio):
        layers, pre = [], input_channels
        for k, c in enumerate(fc_list):
            layers += [nn.Conv1d(pre, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            pre = c
            if dp_ratio >= 0 and k == 0:
                layers.append(nn.Dropout(dp_ratio))
        layers.append(nn.Conv1d(pre, output_channels, kernel_size=1, bias=True))
        return nn.Sequential(*layers)

    @staticmethod
    def generate_predicted_boxes(batch_size, rois, cls_preds, box_preds):
        """residuals are predicted in the RoI's frame: add the RoI size / heading, rotate by its yaw, translate to its centre"""
        code_size = box_preds.shape[-1]
        batch_cls = cls_preds.view(batch_size, -1, cls_preds.shape[-1])
        box = box_preds.view(batch_size, -1, code_size)
        ry = rois[:, :, 6].reshape(-1)
        xyz = rois[:, :, 0:3].reshape(-1, 3)
        local = rois.clone().detach()
        local[:, :, 0:3] = 0
        box = (box + local).view(-1, code_size)
        cosa, sina = torch.cos(ry), torch.sin(ry)
        # box_torch_ops.rotate_points_along_z multiplies ROW vectors by [[c, -s, 0], [s, c, 0], [0, 0, 1]]:
        # x' = x*c + y*s, y' = -x*s + y*c
        x = box[:, 0] * cosa + box[:, 1] * sina
        y = -box[:, 0] * sina + box[:, 1] * cosa
        box = torch.cat([x[:, None], y[:, None], box[:, 2:]], dim=1)
        box[:, 0:3] += xyz
        return batch_cls, box.view(batch_size, -1, code_size)

    def assign_targets_device(self, batch_dict):
        """`assign_targets` on the device kernels: IoU match of all samples in one launch, ONE device-to-host copy (max_iou), the
        reference's host draws (`subsample_rois_host`), ONE host-to-device copy (the sampled slots and their rows in the packed box
        list), then the gather + encode launch.  The BEV features are computed for the sampled RoIs only when the caller supplies
        `roi_feature_fn(row)` with `roi_offsets` (TwoStageDetector), or gathered from `roi_features`.  Same keys, shapes and dtypes
        as `assign_targets`."""
        ptl = self.proposal_target_layer
        if ptl is None:
            raise ValueError("RoIHead: model_cfg.TARGET_CONFIG is required for training")
        rois, labels, scores, gt = batch_dict["rois"], batch_dict["roi_labels"], batch_dict["roi_scores"], batch_dict["gt_boxes_and_cls"]
        bs, cap = labels.shape
        with torch.no_grad():
            max_iou, assignment, _ = match_rois_to_gt(rois, labels, gt, by_class=ptl._c("SAMPLE_ROI_BY_EACH_CLASS", False))
            host_iou = max_iou.cpu().numpy()                                   # the device-to-host copy
            idx = np.stack([ptl.subsample_rois_host(host_iou[b]) for b in range(bs)])
            table = np.zeros((2, bs, idx.shape[1]), np.int32)
            table[0] = idx
            offsets = batch_dict.get("roi_offsets")
            if offsets is not None:   # slot -> row of the packed box list; the zero padding behind a sample's RoIs has no row
                off = np.asarray(offsets, np.int64)
                table[1] = np.where(idx < np.minimum(off[1:] - off[:-1], cap)[:, None], idx + off[:-1, None], -1)
            table = torch.from_numpy(table).to(rois.device)                    # the host-to-device copy
            t = roi_targets(table[0], rois, labels, scores, max_iou, assignment, gt, ptl.cfg)
            if "roi_feature_fn" in batch_dict:
                t["roi_features"] = batch_dict["roi_feature_fn"](table[1])
            else:
                t["roi_features"] = batch_dict["roi_features"][torch.arange(bs, device=rois.device)[:, None], table[0].long()]
        return t

    def _mlp_spec(self):
        """(cin, shared widths, cls hidden widths, reg hidden widths, chains) of the three nn.Sequential's, or the reason (str) why
        they lie outside the shape family of csrc/roi_mlp.hip"""
        chains = [_mlp_chain(m) for m in (self.shared_fc_layer, self.cls_layers, self.reg_layers)]
        if any(c is None for c in chains):
            return "layers other than Conv1d(kernel_size=1) [+ BatchNorm1d + ReLU] groups"
        shared, cls, reg = chains
        if any(bn is None for _, bn in shared) or any(bn is None for _, bn in cls[:-1] + reg[:-1]) or not cls or not reg \
                or cls[-1][1] is not None or reg[-1][1] is not None:
            return "hidden layers without a batch norm, or a final layer with one"
        if self.code_size != 7 or self.num_class != 1:
            return f"code_size {self.code_size}, num_class {self.num_class} (code size 7 and one RoI class only)"
        if not 1 <= len(shared) <= 2:
            return f"{len(shared)} shared layers (1 or 2)"
        if len(cls) - 1 > 2 or len(reg) - 1 > 2:
            return f"{len(cls) - 1} cls / {len(reg) - 1} reg hidden layers (at most 2 each)"
        cin = shared[0][0].in_channels
        if cin % 4 != 0 or not 4 <= cin <= ROI_MLP_MAX_CIN:
            return f"{cin} input channels (a multiple of 4, at most {ROI_MLP_MAX_CIN})"
        widths = [[c.out_channels for c, _ in shared], [c.out_channels for c, _ in cls[:-1]], [c.out_channels for c, _ in reg[:-1]]]
        for w in sum(widths, []):
            if w % 16 != 0 or not 16 <= w <= ROI_MLP_MAX_WIDTH:
                return f"width {w} (multiples of 16, at most {ROI_MLP_MAX_WIDTH})"
        if cls[-1][0].out_channels != 1 or reg[-1][0].out_channels != 7:
            return f"final layers of {cls[-1][0].out_channels} and {reg[-1][0].out_channels} channels (1 and 7)"
        return (cin, *widths, shared + cls + reg)

    def _mlp_check(self, feats):
        """(reason | None, spec)"""
        cuda = torch.is_tensor(feats) and feats.is_cuda
        return self._mlp_check_for(cuda, feats.dtype if cuda else None, feats.shape[-1] if cuda else None, feats.device if cuda else None,
                                   bool(cuda and feats.requires_grad))

    def _mlp_check_for(self, cuda, dtype, channels, device, feats_grad):
        """`_mlp_check` from what it reads of the features: whether they are a CUDA tensor, their dtype, channel count and device, and
        whether they require a gradient (StaticRoIPlan asks before its feature buffer exists)"""
        if os.environ.get("S2D_ROI_MLP") == "0":
            return "S2D_ROI_MLP=0", None
        if self.training:
            return "the head is in training mode (batch statistics, dropout)", None
        spec = self._mlp_spec()
        if isinstance(spec, str):
            return spec, None
        if not cuda:
            return "the features are not a CUDA tensor (CPU tensor)", None
        if dtype != torch.float32:
            return f"feature dtype {dtype}", None
        if channels != spec[0]:
            return f"{channels} feature channels for a head of {spec[0]}", None
        tensors = []
        for conv, bn in spec[4]:
            tensors += [conv.weight, conv.bias] if bn is None else [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        tensors = [t for t in tensors if t is not None]
        if any(t.device != device or t.dtype != torch.float32 for t in tensors):
            return "parameters on another device or not fp32", None
        if torch.is_grad_enabled() and (feats_grad or any(t.requires_grad for t in tensors)):
            return "a gradient is required (no backward through the fused MLP)", None
        return None, spec

    def mlp_reason(self, feats):
        """None when forward(training=False, device=True) can run the MLP as the one fused launch of csrc/roi_mlp.hip, else why it
        runs the three nn.Sequential's through torch"""
        return self._mlp_check(feats)[0]

    def _train_mlp_check(self, feats):
        """(reason | None, spec) for the training branch on csrc/roi_mlp_train.hip"""
        cuda = torch.is_tensor(feats) and feats.is_cuda
        return self._train_mlp_check_for(cuda, feats.dtype if cuda else None, feats.shape[-1] if cuda else None,
                                         feats.numel() // max(feats.shape[-1], 1) if cuda else None, feats.device if cuda else None,
                                         bool(cuda and feats.requires_grad))

    def _train_mlp_check_for(self, cuda, dtype, channels, rows, device, feats_grad):
        """`_train_mlp_check` from what it reads of the features (as `_mlp_check_for`)"""
        if os.environ.get("S2D_ROI_MLP") == "0":
            return "S2D_ROI_MLP=0", None
        if not self.training:
            return "the head is in eval mode (running statistics, no dropout)", None
        spec = self._mlp_spec()
        if isinstance(spec, str):
            return spec, None
        dp = float(_cfg_get(self.model_cfg, "DP_RATIO"))
        if not dp < 1:
            return f"DP_RATIO {dp} (below 1)", None
        for conv, bn in spec[4]:
            if bn is not None and (conv.bias is not None or bn.momentum is None or not bn.track_running_stats):
                return "a hidden convolution with a bias, or a batch norm without momentum or running statistics", None
        loss_cfg = _cfg_get(self.model_cfg, "LOSS_CONFIG", None)
        if loss_cfg is not None and (_cfg_get(loss_cfg, "CLS_LOSS") != "BinaryCrossEntropy" or _cfg_get(loss_cfg, "REG_LOSS") != "L1"):
            return f"{_cfg_get(loss_cfg, 'CLS_LOSS')} / {_cfg_get(loss_cfg, 'REG_LOSS')} losses (BinaryCrossEntropy and L1 only)", None
        if not cuda:
            return "the features are not a CUDA tensor (CPU tensor)", None
        if dtype != torch.float32:
            return f"feature dtype {dtype}", None
        if channels != spec[0]:
            return f"{channels} feature channels for a head of {spec[0]}", None
        if not ROI_MLP_TRAIN_ROWS[0] <= rows <= ROI_MLP_TRAIN_ROWS[1]:
            return f"{rows} rows ({ROI_MLP_TRAIN_ROWS[0]} .. {ROI_MLP_TRAIN_ROWS[1]}: batch statistics)", None
        tensors = [t for conv, bn in spec[4] for t in ((conv.weight, conv.bias) if bn is None else
                                                       (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var))]
        if any(t is None or t.device != device or t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
            return "parameters on another device or not fp32", None
        if not torch.is_grad_enabled():
            return "grad mode is disabled (the training branch exists for its backward)", None
        if feats_grad:
            return "the features require a gradient (the kernels give them none)", None
        return None, spec

    def train_mlp_reason(self, feats):
        """None when forward(training=True, device=True) with `fused_training` set can run the MLP on csrc/roi_mlp_train.hip, else why it
        keeps the three nn.Sequential's and autograd"""
        return self._train_mlp_check(feats)[0]

    def _mlp_images(self, spec, dev, affine=True):
        """(plan, packed weight image, scale / shift vector) of the fused MLP, cached on the head.  Keyed like dense2d.cached_pack on
        (data_ptr, _version) of every tensor that enters each of the two: an optimizer step, load_state_dict or an in-place edit of a
        running statistic rebuilds what it changed (and only that); dense2d.clear_pack_cache() - checkpoint.load - and
        dense2d.refresh_pack_cache() - the fused Adam, which writes through raw pointers - drop both."""
        from . import dense2d
        cin, shared_w, cls_w, reg_w, chain = spec
        lib = _lib.load()
        cache = self._mlp_cache
        shape = (cin, tuple(shared_w), tuple(cls_w), tuple(reg_w), str(dev), dense2d.pack_epoch())
        if cache is None or cache["shape"] != shape:
            pad = lambda w: (list(w) + [0, 0])[:2]
            plan = _lib.RoiMlpPlan()
            _lib.check(lib.s2d_roi_mlp_plan_make(cin, len(shared_w), *pad(shared_w), len(cls_w), *pad(cls_w), len(reg_w), *pad(reg_w), self.num_class,
                                                 self.code_size, ctypes.byref(plan)), "s2d_roi_mlp_plan_make")
            cache = self._mlp_cache = dict(shape=shape, plan=plan, w_key=None, packed=None, a_key=None, affine=None)
        plan = cache["plan"]
        key = lambda ts: tuple((t.data_ptr(), t._version) for t in ts if t is not None)
        w_key = key([conv.weight for conv, _ in chain])
        if cache["w_key"] != w_key:
            weights = [conv.weight.detach() for conv, _ in chain]   # [cout, cin, 1] contiguous = [cout][cin] row-major
            weights = [w if w.is_contiguous() else w.contiguous() for w in weights]
            packed = torch.empty((plan.packed_elems,), dtype=torch.float32, device=dev)
            ptrs = (ctypes.c_void_p * len(weights))(*[w.data_ptr() for w in weights])
            _lib.check(lib.s2d_roi_mlp_pack(ctypes.byref(plan), ptrs, packed.data_ptr(), torch._C._cuda_getCurrentRawStream(dev.index)), "s2d_roi_mlp_pack")
            cache["w_key"], cache["packed"] = w_key, packed
        if not affine:   # the training branch normalises with batch statistics
            return plan, cache["packed"], None
        # (a training-mode batch norm moves its running statistics WITHOUT moving their version counters - torch.batch_norm does not declare
        # them as written - but it counts the call in num_batches_tracked with an ordinary in-place add: that counter is part of the key)
        a_key = key([t for conv, bn in chain for t in ((conv.bias,) if bn is None else
                                                       (conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked))])
        if cache["a_key"] != a_key:
            parts = []
            with torch.no_grad():
                for l, (conv, bn) in enumerate(chain):
                    fill = plan.layer[l].cout_pad - conv.out_channels
                    parts += [F.pad(v.float(), (0, fill)) for v in _mlp_affine(conv, bn)]
                affine = torch.cat(parts).contiguous()
            assert affine.numel() == plan.affine_elems
            cache["a_key"], cache["affine"] = a_key, affine
        return plan, cache["packed"], cache["affine"]

    def _mlp_fused(self, feats, spec):
        """rcnn_cls [R, 1], rcnn_reg [R, 7] of feats [..., cin] in one launch"""
        lib, dev, st = _device_args("roi_mlp", feats)
        x = feats.detach().reshape(-1, feats.shape[-1])
        x = x if x.is_contiguous() and x.data_ptr() % 16 == 0 else x.clone(memory_format=torch.contiguous_format)
        plan, packed, affine = self._mlp_images(spec, dev)
        rcnn_cls = torch.empty((x.shape[0], 1), dtype=torch.float32, device=dev)
        rcnn_reg = torch.empty((x.shape[0], 7), dtype=torch.float32, device=dev)
        _lib.check(lib.s2d_roi_mlp_run(ctypes.byref(plan), x.data_ptr(), x.shape[0], packed.data_ptr(), affine.data_ptr(), rcnn_cls.data_ptr(),
                                       rcnn_reg.data_ptr(), st), "s2d_roi_mlp_run")
        return rcnn_cls, rcnn_reg

    def forward(self, batch_dict, training=True, device=False):
        """device=True: targets (training) and refinement (inference) on the kernels of csrc/roi_head.hip - CUDA tensors, code size 7"""
        batch_dict["batch_size"] = len(batch_dict["rois"])
        targets = None
        if training:   # roi_head.py:76-80
            targets = self.assign_targets_device(batch_dict) if device else self.assign_targets(batch_dict)
            batch_dict["rois"], batch_dict["roi_labels"], batch_dict["roi_features"] = targets["rois"], targets["roi_labels"], targets["roi_features"]
        reason, spec = self._mlp_check(batch_dict["roi_features"]) if device and not training else ("training or the torch chain", None)
        fused_training = False
        if training:
            self.train_reason = self.train_mlp_reason(batch_dict["roi_features"]) if device and self.fused_training else None
            fused_training = device and self.fused_training and self.train_reason is None
            self.train_paths["fused" if fused_training else "torch"] += 1
        if fused_training:   # batch statistics, dropout and a backward on csrc/roi_mlp_train.hip
            rcnn_cls, rcnn_reg = roi_mlp_train_fused(self, batch_dict["roi_features"])
            targets["fused_training"] = True
        elif reason is None:   # the whole eval MLP in one launch (csrc/roi_mlp.hip)
            self.mlp_paths["fused"] += 1
            rcnn_cls, rcnn_reg = self._mlp_fused(batch_dict["roi_features"], spec)
        else:
            self.mlp_paths["torch"] += 1
            pooled = batch_dict["roi_features"].reshape(-1, 1, batch_dict["roi_features"].shape[-1]).permute(0, 2, 1).contiguous()
            shared = self.shared_fc_layer(pooled)
            rcnn_cls = self.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
            rcnn_reg = self.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        if training:
            targets["rcnn_cls"], targets["rcnn_reg"] = rcnn_cls, rcnn_reg
            self.forward_ret_dict = targets
            return batch_dict
        if device:
            box, scores, labels = refine_rois(batch_dict["rois"], batch_dict["roi_scores"], batch_dict["roi_labels"], rcnn_cls, rcnn_reg)
            batch_dict["batch_cls_preds"], batch_dict["batch_box_preds"] = rcnn_cls.view(batch_dict["batch_size"], -1, rcnn_cls.shape[-1]), box
            batch_dict["refined_scores"], batch_dict["refined_labels"], batch_dict["cls_preds_normalized"] = scores, labels, False
            return batch_dict
        cls, box = self.generate_predicted_boxes(batch_dict["batch_size"], batch_dict["rois"], rcnn_cls, rcnn_reg)
        batch_dict["batch_cls_preds"], batch_dict["batch_box_preds"], batch_dict["cls_preds_normalized"] = cls, box, False
        return batch_dict


# ---- the second stage without the host: fixed-capacity buffers, launches only, capturable into one HIP graph behind predict_static -------
STATIC_ROI_LAUNCHES = 4   # s2d_roi_pack_static, s2d_roi_bev_features, s2d_roi_mlp_run, s2d_roi_refine_static


class StaticRefinedDetections(center_predict.StaticDetections):
    """`StaticRoIPlan.run`'s results: a `StaticDetections` (boxes [B, cap, 7], scores, labels [B, cap], counts [B]; zero rows with label
    -1 behind the counts; overflow = the first stage's, passed through) that also carries the example's `metadata`, which `as_list()`
    then hands out without being given it."""
    __slots__ = ("metadata",)

    def __init__(self, boxes, scores, labels, counts, overflow=None, metadata=None):
        super().__init__(boxes, scores, labels, counts, overflow)
        self.metadata = metadata

    def as_list(self, metadata=None):
        """what `TwoStageDetector.forward(return_loss=False)` returns: one dict per sample (box3d_lidar, scores, label_preds,
        metadata), views into the padded buffers.  The ONE host read of the static path: the counts."""
        return super().as_list(self.metadata if metadata is None else metadata)


class StaticRoIPlan:
    """The inference second stage on `CenterHead.predict_static`'s padded, device-counted detections (center_predict.StaticDetections),
    for one (RoI head MLP spec, BEVFeatureExtractor geometry, num_point, samples B, det_cap, cap = NMS_POST_MAXSIZE, map channels and
    dtype, device).  Everything is allocated here, once: rois, roi_scores, roi_labels, row, counts, feats [B * cap, num_point * C],
    rcnn_cls, rcnn_reg and the outputs; the MLP's packed weight image and scale / shift vector come from the head's `_mlp_images`.

    `run(det, bev)` only launches on the current stream - s2d_roi_pack_static, s2d_roi_bev_features, s2d_roi_mlp_run,
    s2d_roi_refine_static: 4 launches - with no host read, no host-to-device copy and, in the steady state, no allocation and no torch
    operator, so it can be captured into a HIP graph (one stream, a linear chain), alone or behind StaticPredictPlan.run.  The boxes are
    read where `det` holds them (the row table indexes det.boxes as [B * det_cap, 7]), the map where it lies with its own strides.

    The MLP images are checked at every call on the host by the (data_ptr, _version) keys `_mlp_images` keeps: after an optimizer step,
    load_state_dict or an in-place edit the stale image is rebuilt BEFORE the launches (such a call may allocate and runs torch
    operators) and counted in `repacks`.  A graph captured earlier holds the old images' addresses: it must be captured again after the
    weights change.

    Refused with S2DError before any HIP call, no fallback: a non-CUDA device, B > 64, boxes that are not 7-column, a detection set of
    another B or det_cap, a head whose `mlp_reason` is not None (training mode, a required gradient, a shape outside the kernel's
    family), num_point other than 1 or 5, a code size other than 7 or more than one RoI class, second-stage modules other than one
    BEVFeatureExtractor, a map of another dtype, channel count or batch."""

    def __init__(self, roi_head, second_stage, num_point, samples, det_cap, cap, channels, map_dtype, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.S2DError("StaticRoIPlan: a CUDA device expected (no CPU fallback)")
        if not 1 <= samples <= ROI_MAX_BATCH:
            raise _lib.S2DError(f"StaticRoIPlan: {samples} samples (1..{ROI_MAX_BATCH} supported)")
        if det_cap < 1 or cap < 1 or samples * det_cap >= 2 ** 31:
            raise _lib.S2DError(f"StaticRoIPlan: det_cap {det_cap}, cap {cap} (>= 1 each, samples x det_cap below 2^31)")
        if num_point not in (1, 5):
            raise _lib.S2DError(f"StaticRoIPlan: num_point {num_point} (1 or 5 supported)")
        if roi_head.code_size != 7 or roi_head.num_class != 1:
            raise _lib.S2DError(f"StaticRoIPlan: code_size {roi_head.code_size}, num_class {roi_head.num_class} (code size 7 and one RoI class only)")
        modules = list(second_stage)
        if len(modules) != 1 or type(modules[0]) is not BEVFeatureExtractor:
            raise _lib.S2DError("StaticRoIPlan: second-stage modules other than one BEVFeatureExtractor")
        if map_dtype not in (torch.float32, torch.bfloat16) or channels < 1:
            raise _lib.S2DError(f"StaticRoIPlan: a map of {channels} channels in {map_dtype} (fp32 or bf16)")
        if device.index is None:   # (without a GPU the head's reason below is still given before any HIP call)
            device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.head, self.device = roi_head, device
        self.samples, self.det_cap, self.cap, self.num_point = int(samples), int(det_cap), int(cap), int(num_point)
        self.channels, self.map_dtype, self.cin = int(channels), map_dtype, int(num_point) * int(channels)
        reason, spec = roi_head._mlp_check_for(True, torch.float32, self.cin, device, False)
        if reason is not None:
            raise _lib.S2DError(f"StaticRoIPlan: {reason}")
        ext = modules[0]
        self.geo = (float(ext.pc_start[0]), float(ext.pc_start[1]), float(ext.voxel_size[0]), float(ext.voxel_size[1]), float(ext.out_stride))
        _lib.load()
        b, rows = self.samples, self.samples * self.cap
        new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)
        self.rois, self.roi_scores, self.roi_labels = new((b, cap, 7), torch.float32), new((b, cap), torch.float32), new((b, cap), torch.int64)
        self.row, self.counts = new((b, cap), torch.int32), new((b,), torch.int32)
        self.feats = new((rows, self.cin), torch.float32)
        self.rcnn_cls, self.rcnn_reg = new((rows, 1), torch.float32), new((rows, 7), torch.float32)
        self.boxes, self.scores, self.labels = new((b, cap, 7), torch.float32), new((b, cap), torch.float32), new((b, cap), torch.int64)
        self.out = StaticRefinedDetections(self.boxes, self.scores, self.labels, self.counts)
        self.repacks = 0
        self._mlp_plan, self._packed, self._affine = roi_head._mlp_images(spec, device)

    def buffers(self):
        """every device buffer the plan owns by name (none is ever reallocated; the MLP images belong to the head)"""
        names = ("rois", "roi_scores", "roi_labels", "row", "counts", "feats", "rcnn_cls", "rcnn_reg", "boxes", "scores", "labels")
        return {n: getattr(self, n) for n in names}

    def _check(self, det, bev):
        boxes, scores, labels, counts = det.boxes, det.scores, det.labels, det.counts
        if boxes.dim() != 3 or boxes.shape[-1] != 7:
            raise _lib.S2DError(f"StaticRoIPlan.run: boxes {tuple(boxes.shape)}: 7-column boxes [B, det_cap, 7] expected (the velocity columns of "
                                "9-column first-stage boxes are not supported)")
        b, d = self.samples, self.det_cap
        if tuple(boxes.shape) != (b, d, 7):
            raise _lib.S2DError(f"StaticRoIPlan.run: boxes {tuple(boxes.shape)}, the plan was built for {(b, d, 7)} (samples, det_cap, 7)")
        for name, t, dtype, shape in (("boxes", boxes, torch.float32, (b, d, 7)), ("scores", scores, torch.float32, (b, d)),
                                      ("labels", labels, torch.int64, (b, d)), ("counts", counts, torch.int32, (b,))):
            if t.device != self.device or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise _lib.S2DError(f"StaticRoIPlan.run: {name} is {t.dtype} {tuple(t.shape)} on {t.device}"
                                    f"{'' if t.is_contiguous() else ', not contiguous'}: contiguous {dtype} {shape} on {self.device} expected "
                                    "(the static second stage neither copies nor converts)")
        if not (torch.is_tensor(bev) and bev.dim() == 4 and bev.device == self.device):
            raise _lib.S2DError(f"StaticRoIPlan.run: the neck map is not a [B, C, H, W] tensor on {self.device}")
        if bev.dtype != self.map_dtype or bev.shape[0] != b or bev.shape[1] != self.channels or bev.shape[2] < 1 or bev.shape[3] < 1:
            raise _lib.S2DError(f"StaticRoIPlan.run: the neck map is {bev.dtype} {tuple(bev.shape)}, the plan was built for {self.map_dtype} "
                                f"[{b}, {self.channels}, H, W]")
        if any(s < 0 for s in bev.stride()):
            raise _lib.S2DError("StaticRoIPlan.run: a neck map with a negative stride")
        reason, spec = self.head._mlp_check_for(True, torch.float32, self.cin, self.device, False)
        if reason is not None:
            raise _lib.S2DError(f"StaticRoIPlan.run: {reason}")
        return spec

    def run(self, det, bev):
        """det: the StaticDetections of a StaticPredictPlan with this plan's samples and det_cap; bev [B, C, H, W] fp32 or bf16, NCHW or
        channels_last, read in place.  Launches only, on the current stream; returns the plan's `StaticRefinedDetections` (the same
        tensors at every call, overwritten by the next one)."""
        spec = self._check(det, bev)   # host only
        mlp_plan, packed, affine = self.head._mlp_images(spec, self.device)   # host only unless a key moved
        if packed is not self._packed or affine is not self._affine:
            self.repacks += 1
            self._mlp_plan, self._packed, self._affine = mlp_plan, packed, affine
        lib, st, ptr = _lib.load(), torch._C._cuda_getCurrentRawStream(self.device.index), lambda t: t.data_ptr()
        b, d, cap, rows = self.samples, self.det_cap, self.cap, self.samples * self.cap
        _lib.check(lib.s2d_roi_pack_static(ptr(det.boxes), ptr(det.scores), ptr(det.labels), ptr(det.counts), b, d, cap, ptr(self.rois),
                                           ptr(self.roi_scores), ptr(self.roi_labels), ptr(self.row), ptr(self.counts), st), "s2d_roi_pack_static")
        _lib.check(lib.s2d_roi_bev_features(ptr(bev), int(bev.dtype == torch.bfloat16), b, self.channels, bev.shape[2], bev.shape[3], *bev.stride(),
                                            ptr(det.boxes), b * d, 7, ptr(self.row), cap, self.num_point, *self.geo, ptr(self.feats), st),
                   "s2d_roi_bev_features")
        _lib.check(lib.s2d_roi_mlp_run(ctypes.byref(mlp_plan), ptr(self.feats), rows, ptr(packed), ptr(affine), ptr(self.rcnn_cls),
                                       ptr(self.rcnn_reg), st), "s2d_roi_mlp_run")
        _lib.check(lib.s2d_roi_refine_static(ptr(self.rois), ptr(self.roi_scores), ptr(self.roi_labels), ptr(self.rcnn_cls), ptr(self.rcnn_reg),
                                             ptr(self.counts), b, cap, ptr(self.boxes), ptr(self.scores), ptr(self.labels), st),
                   "s2d_roi_refine_static")
        self.out.overflow = det.overflow
        return self.out


def static_roi_plan_key(roi_head, second_stage, num_point, samples, det_cap, cap, channels, map_dtype, device):
    """what a StaticRoIPlan depends on, as a hashable key (TwoStageDetector.forward_static caches plans by it)"""
    spec = roi_head._mlp_spec()
    shape = spec if isinstance(spec, str) else (spec[0], tuple(spec[1]), tuple(spec[2]), tuple(spec[3]))
    geo = tuple((type(m).__name__, tuple(float(v) for v in getattr(m, "pc_start", ())), tuple(float(v) for v in getattr(m, "voxel_size", ())),
                 float(getattr(m, "out_stride", 0))) for m in second_stage)
    # (the plan holds the head it was built for - and so keeps its id from being reused: another head of the same shape gets its own plan)
    return (id(roi_head), shape, geo, int(num_point), int(samples), int(det_cap), int(cap), int(channels), map_dtype, str(device))


def box_side_centers(box3d):
    """centre + the four face-centre points of each BEV box (two_stage.py:50-74, box_torch_ops.center_to_corner_box2d):
    [5*n, 3], the five sets stacked along dim 0"""
    center2d, height, dim2d, yaw = box3d[:, :2], box3d[:, 2:3], box3d[:, 3:5], box3d[:, -1]
    # unit corners clockwise from the minimum point, origin 0.5: (-.5,-.5), (-.5,.5), (.5,.5), (.5,-.5)
    unit = box3d.new_tensor([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]])
    corners = dim2d[:, None, :] * unit[None]                                   # [n, 4, 2]
    s, c = torch.sin(yaw), torch.cos(yaw)
    # rotation_2d: corners @ [[c, -s], [s, c]] per box (einsum "aij,jka->aik" with rot_mat_T = [[c, -s], [s, c]])
    rx = corners[..., 0] * c[:, None] + corners[..., 1] * s[:, None]
    ry = -corners[..., 0] * s[:, None] + corners[..., 1] * c[:, None]
    corners = torch.stack([rx, ry], dim=-1) + center2d[:, None, :]
    mid = lambda a, b: torch.cat([(corners[:, a] + corners[:, b]) / 2, height], dim=-1)
    return torch.cat([box3d[:, :3], mid(0, 1), mid(2, 3), mid(0, 3), mid(1, 2)], dim=0)


@DETECTORS.register_module
class TwoStageDetector(nn.Module):
    def __init__(self, first_stage_cfg, second_stage_modules, roi_head, NMS_POST_MAXSIZE, num_point=1, freeze=False,
                 train_cfg=None, test_cfg=None, pretrained=None, **kwargs):
        super().__init__()
        self.single_det = registry.build_detector(first_stage_cfg, train_cfg=train_cfg, test_cfg=test_cfg)
        self.NMS_POST_MAXSIZE = NMS_POST_MAXSIZE
        if freeze:   # the reference trains in two steps: the first stage is frozen (two_stage.py:24-27)
            for p in self.single_det.parameters():
                p.requires_grad = False
            self.single_det.eval()
        self.freeze = freeze
        self.bbox_head = self.single_det.bbox_head
        self.second_stage = nn.ModuleList([registry.build(m, SECOND_STAGE) for m in second_stage_modules])
        self.roi_head = registry.build(roi_head, ROI_HEAD)
        self.num_point = num_point
        self.roi_paths = {"device": 0, "torch": 0}   # calls of forward() by the path their second stage took
        self.static_calls = 0                        # calls of forward_static()
        self._static_roi_plans = {}                  # StaticRoIPlan by static_roi_plan_key

    def train(self, mode=True):
        super().train(mode)
        if self.freeze:
            self.single_det.eval()
        return self

    def get_box_center(self, boxes):
        out = []
        for box in boxes:
            b = box["box3d_lidar"]
            if self.num_point == 1 or len(b) == 0:
                out.append(b[:, :3])
            elif self.num_point == 5:
                out.append(box_side_centers(b))
            else:
                raise NotImplementedError()
        return out

    def reorder_first_stage_pred_and_feature(self, first_pred, example, features):
        n, cap = len(first_pred), self.NMS_POST_MAXSIZE
        box_len = first_pred[0]["box3d_lidar"].shape[1]
        flen = sum(f[0].shape[-1] for f in features)
        rois = first_pred[0]["box3d_lidar"].new_zeros((n, cap, box_len))
        scores = first_pred[0]["scores"].new_zeros((n, cap))
        labels = first_pred[0]["label_preds"].new_zeros((n, cap), dtype=torch.long)
        feats = features[0][0].new_zeros((n, cap, flen))
        for i in range(n):
            k = features[0][i].shape[0]
            bp = first_pred[i]["box3d_lidar"]
            if self.roi_head.code_size == 9:   # (x, y, z, w, l, h, yaw, vx, vy)
                bp = bp[:, [0, 1, 2, 3, 4, 5, 8, 6, 7]]
            rois[i, :k], labels[i, :k], scores[i, :k] = bp, first_pred[i]["label_preds"] + 1, first_pred[i]["scores"]
            feats[i, :k] = torch.cat([f[i] for f in features], dim=-1)
        example.update(rois=rois, roi_labels=labels, roi_scores=scores, roi_features=feats, has_class_labels=True)
        return example

    def post_process(self, batch_dict):
        out = []
        meta = batch_dict.get("metadata")
        for i in range(batch_dict["batch_size"]):
            box, cls, lab = batch_dict["batch_box_preds"][i], batch_dict["batch_cls_preds"][i], batch_dict["roi_labels"][i]
            if box.shape[-1] == 9:
                box = box[:, [0, 1, 2, 3, 4, 5, 7, 8, 6]]
            scores = torch.sqrt(torch.sigmoid(cls).reshape(-1) * batch_dict["roi_scores"][i].reshape(-1))
            m = (lab != 0).reshape(-1)
            out.append(dict(box3d_lidar=box[m, :], scores=scores[m], label_preds=lab[m] - 1, metadata=meta[i] if meta else None))
        return out

    @staticmethod
    def combine_loss(one_stage_loss, roi_loss, tb_dict):
        """two_stage.py:40-47: the RoI loss is added to the first task's loss; its two terms are logged per task"""
        one_stage_loss["loss"][0] = one_stage_loss["loss"][0] + roi_loss
        one_stage_loss.setdefault("roi_reg_loss", [])
        one_stage_loss.setdefault("roi_cls_loss", [])
        for _ in range(len(one_stage_loss["loss"])):
            one_stage_loss["roi_reg_loss"].append(tb_dict["rcnn_loss_reg"])
            one_stage_loss["roi_cls_loss"].append(tb_dict["rcnn_loss_cls"])
        return one_stage_loss

    def device_path_reason(self, one_stage_pred, bev_feature, example, return_loss):
        """None when the second stage can run on the kernels of csrc/roi_head.hip, else why it takes the torch chain"""
        if os.environ.get("S2D_ROI_DEVICE") == "0":
            return "S2D_ROI_DEVICE=0"
        if not (torch.is_tensor(bev_feature) and bev_feature.is_cuda and bev_feature.dim() == 4):
            return "the neck map is not a CUDA tensor"
        if bev_feature.dtype not in (torch.float32, torch.bfloat16):
            return f"neck map dtype {bev_feature.dtype}"
        if bev_feature.requires_grad and torch.is_grad_enabled():
            return "the neck map carries a gradient (no backward through the BEV sampling)"
        if self.roi_head.code_size != 7 or self.roi_head.num_class != 1:
            return "code size 7 and one RoI class only"
        if self.num_point not in (1, 5):
            return f"num_point {self.num_point}"
        if len(self.second_stage) != 1 or type(self.second_stage[0]) is not BEVFeatureExtractor:
            return "second-stage modules other than one BEVFeatureExtractor"
        if not 1 <= len(one_stage_pred) <= ROI_MAX_BATCH or len(one_stage_pred) != bev_feature.shape[0]:
            return f"{len(one_stage_pred)} samples"
        for p in one_stage_pred:
            b = p["box3d_lidar"]
            if not b.is_cuda or b.dim() != 2 or b.shape[1] != 7 or b.shape[0] > self.NMS_POST_MAXSIZE:
                return f"first-stage boxes {tuple(b.shape)}"
        if return_loss:
            gt = example.get("gt_boxes_and_cls")
            ptl = self.roi_head.proposal_target_layer
            if ptl is None or ptl.iou_fn is not boxes_iou3d or ptl._c("CLS_SCORE_TYPE") not in ("cls", "roi_iou"):
                return "no or a custom proposal target layer"
            if not (torch.is_tensor(gt) and gt.is_cuda and gt.dim() == 3 and gt.shape[2] >= 8 and 1 <= gt.shape[1] <= ROI_MAX_GT):
                return f"ground truth outside the match kernel's bound ({ROI_MAX_GT} rows per sample)"
        return None

    @staticmethod
    def _packed_first_stage(preds):
        """(boxes, scores, labels, offsets) of the whole batch.  CenterHead.predict's device path hands out per-sample views of one packed
        tensor each: those are taken as they are, anything else is concatenated."""
        counts = [int(p["box3d_lidar"].shape[0]) for p in preds]
        offsets = [0]
        for c in counts:
            offsets.append(offsets[-1] + c)

        def packed(key):
            parts = [p[key] for p in preds]
            base = parts[0]._base
            if base is not None and base.is_contiguous() and base.shape[0] == offsets[-1] and base.shape[1:] == parts[0].shape[1:]:
                row = base[0].numel() if base.shape[0] else 1
                if all(q._base is base and q.is_contiguous() and q.storage_offset() == base.storage_offset() + o * row for q, o in zip(parts, offsets)):
                    return base
            return torch.cat(parts, dim=0)
        return packed("box3d_lidar"), packed("scores"), packed("label_preds"), offsets

    def _forward_device(self, one_stage_pred, bev_feature, example, return_loss):
        """the second stage on the device kernels: pack -> (match -> host sampling -> targets) -> BEV features of the RoIs the MLP
        will see -> RoI MLP -> (refine).  `example` gets the RoI tensors the chain puts there; the fp32 NHWC copy of the neck map
        (`example["bev_feature"]`) is NOT made - the map is sampled where it lies."""
        boxes, scores, labels, offsets = self._packed_first_stage(one_stage_pred)
        bs, cap, ext = len(one_stage_pred), self.NMS_POST_MAXSIZE, self.second_stage[0]
        bev = bev_feature.detach()
        rois, roi_scores, roi_labels = pack_rois(boxes, scores, labels, offsets, cap)
        feature_fn = lambda row: roi_bev_features(bev, boxes, row, ext.pc_start, ext.voxel_size, ext.out_stride, self.num_point)
        example.update(rois=rois, roi_labels=roi_labels, roi_scores=roi_scores, has_class_labels=True)
        if return_loss:
            example["gt_boxes_and_cls"] = example["gt_boxes_and_cls"][:, :, [0, 1, 2, 3, 4, 5, 6, -1]]   # two_stage.py:173-175
            example.update(roi_feature_fn=feature_fn, roi_offsets=offsets)
            try:
                self.roi_head(example, training=True, device=True)
            finally:
                del example["roi_feature_fn"], example["roi_offsets"]
            return None
        row = np.full((bs, cap), -1, np.int32)
        for b in range(bs):
            n = offsets[b + 1] - offsets[b]
            row[b, :n] = np.arange(offsets[b], offsets[b + 1], dtype=np.int32)
        with torch.no_grad():
            example["roi_features"] = feature_fn(torch.from_numpy(row).to(rois.device))
        batch_dict = self.roi_head(example, training=False, device=True)
        meta = batch_dict.get("metadata")
        out = []
        for b in range(bs):   # the valid RoIs of a sample are its first slots: the host slices, no mask and no read
            n = offsets[b + 1] - offsets[b]
            out.append(dict(box3d_lidar=batch_dict["batch_box_preds"][b, :n], scores=batch_dict["refined_scores"][b, :n],
                            label_preds=batch_dict["refined_labels"][b, :n], metadata=meta[b] if meta else None))
        return out

    @torch.no_grad()
    def forward_static(self, example, max_candidates=4096):
        """Inference with both stages behind the head maps on the static path (opt-in; `forward`, `forward_two_stage`, `_forward_device`,
        `roi_paths` and every environment switch are untouched; `static_calls` counts the calls):
          1. the first stage up to the head maps, by the route `forward_two_stage` takes (`single_det.first_stage_maps`: extract_feat,
             then the head);
          2. `bbox_head.predict_static` (center_predict.StaticPredictPlan);
          3. `StaticRoIPlan.run` on its detections and the neck map, the plan cached on the detector by `static_roi_plan_key`.
        Returns the plan's StaticRefinedDetections - padded device tensors that the next call overwrites; `.as_list()` does the one host
        read and gives what `forward(return_loss=False)` returns.  Only steps 2 and 3 are launches-only and can be captured into a HIP
        graph (capture `StaticPredictPlan.run` + `StaticRoIPlan.run` on static input tensors): the sparse first stage is shape-dynamic.
        Whatever either plan refuses is an S2DError here: there is no fallback to `forward`."""
        bev, preds = self.single_det.first_stage_maps(example)
        det, meta = self.bbox_head.predict_static(example, preds, self.single_det.test_cfg, max_candidates)
        if not (torch.is_tensor(bev) and bev.dim() == 4):
            raise _lib.S2DError("forward_static: the neck map is not a [B, C, H, W] tensor")
        if det.boxes.dim() != 3:
            raise _lib.S2DError(f"forward_static: first-stage boxes {tuple(det.boxes.shape)}")
        bev = bev.detach()
        samples, det_cap = det.boxes.shape[:2]
        key = static_roi_plan_key(self.roi_head, self.second_stage, self.num_point, samples, det_cap, self.NMS_POST_MAXSIZE, bev.shape[1], bev.dtype,
                                  bev.device)
        plan = self._static_roi_plans.get(key)
        if plan is None:
            plan = self._static_roi_plans[key] = StaticRoIPlan(self.roi_head, self.second_stage, self.num_point, samples, det_cap,
                                                               self.NMS_POST_MAXSIZE, bev.shape[1], bev.dtype, bev.device)
        out = plan.run(det, bev)
        out.metadata = meta
        self.static_calls += 1
        return out

    def forward(self, example, return_loss=True, return_feature=False, **kwargs):
        out = self.single_det.forward_two_stage(example, return_loss, **kwargs)
        f_a = f_b = None
        if len(out) == 6:
            one_stage_pred, bev_feature, voxel_feature, one_stage_loss, f_a, f_b = out
        else:
            one_stage_pred, bev_feature, voxel_feature, one_stage_loss = out
        example["voxel_feature"] = voxel_feature
        if self.device_path_reason(one_stage_pred, bev_feature, example, return_loss) is None:
            self.roi_paths["device"] += 1
            res = self._forward_device(one_stage_pred, bev_feature, example, return_loss)
            if return_loss:
                roi_loss, tb = self.roi_head.get_loss()
                return self.combine_loss(one_stage_loss, roi_loss, tb)
            return (res, f_a, f_b) if return_feature else res
        self.roi_paths["torch"] += 1
        example["bev_feature"] = bev_feature.float().permute(0, 2, 3, 1).contiguous()   # N C H W -> N H W C
        centers = self.get_box_center(one_stage_pred)
        if self.roi_head.code_size == 7 and return_loss:   # drop the velocity columns (two_stage.py:173-175)
            example["gt_boxes_and_cls"] = example["gt_boxes_and_cls"][:, :, [0, 1, 2, 3, 4, 5, 6, -1]]
        features = [m(example, centers, self.num_point) for m in self.second_stage]
        example = self.reorder_first_stage_pred_and_feature(one_stage_pred, example, features)
        batch_dict = self.roi_head(example, training=return_loss)
        if return_loss:
            roi_loss, tb = self.roi_head.get_loss()
            return self.combine_loss(one_stage_loss, roi_loss, tb)
        res = self.post_process(batch_dict)
        return (res, f_a, f_b) if return_feature else res
