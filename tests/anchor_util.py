"""Shared pieces of the anchor-head tests and of tests/golden/make_golden_anchor.py: the seeded inputs (so that the fixtures store no
inputs) and the float64 torch restatement of MultiGroupHead.loss that the GPU tests use as their second reference
(tests/test_anchor_head_cpu.py pins it to the reference's own numbers in anchor_loss.npz)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

H = W = 188
SLOTS = 6
A = H * W * SLOTS
CLASS_SIZES = np.array([[2.08, 4.73, 1.77], [0.84, 0.91, 1.74], [0.84, 1.81, 1.77]], np.float32)
# pos_cls_weight, neg_cls_weight, alpha, gamma, sigma, loc / cls / dir loss weights, direction_offset (the Waymo SECOND config)
LOSS_PARAMS = [1.0, 2.0, 0.25, 2.0, 3.0, 2.0, 1.0, 0.2, 0.0]


def random_boxes(rng, n, classes=(1, 2, 3)):
    """n boxes (x,y,z,w,l,h,r) fp32 of mixed classes: class sizes x U(0.8, 1.25), centres U(-70, 70), yaw U(-3.14, 3.14)"""
    cls = rng.choice(np.asarray(classes), size=n).astype(np.int32)
    size = CLASS_SIZES[cls - 1] * rng.uniform(0.8, 1.25, (n, 3))
    xy = rng.uniform(-70, 70, (n, 2))
    z = rng.uniform(-1.0, 1.0, (n, 1))
    yaw = rng.uniform(-3.14, 3.14, (n, 1))
    return np.concatenate([xy, z, size, yaw], 1).astype(np.float32), cls


def target_frames(anchors, seed=0):
    """the three frames of anchor_targets.npz: (i) 60 mixed boxes; (ii) no PEDESTRIAN, one VEHICLE centred exactly between two cell
    centres (several anchors share its maximum), one box outside the anchor range (its maximum is 0: never forced); (iii) empty.
    anchors: the [A, 7] table (the tie box is placed from its cell centres).  -> list of (boxes [K,7] f32, classes [K] i32)"""
    rng = np.random.default_rng(seed)
    f0 = random_boxes(rng, 60)
    b1, c1 = random_boxes(rng, 20, classes=(1, 3))
    cells = anchors.reshape(H, W, SLOTS, 7)
    x = np.float32((cells[90, 100, 0, 0] + cells[90, 101, 0, 0]) / np.float32(2))
    tie = np.array([[x, cells[90, 100, 0, 1], 0.3, 1.6, 3.6, 1.5, 0.0]], np.float32)
    outside = np.array([[95.0, 10.0, 0.0, 2.0, 4.5, 1.6, 0.3]], np.float32)
    b1 = np.concatenate([b1, tie, outside]).astype(np.float32)
    c1 = np.concatenate([c1, [1, 1]]).astype(np.int32)
    return [f0, (b1, c1), (np.zeros((0, 7), np.float32), np.zeros((0,), np.int32))]


def pad_frames(frames):
    k = max([len(b) for b, _ in frames] + [1])
    boxes = np.zeros((len(frames), k, 7), np.float32)
    classes = np.zeros((len(frames), k), np.int32)
    for i, (b, c) in enumerate(frames):
        boxes[i, :len(b)] = b
        classes[i, :len(b)] = c
    return boxes, classes


def loss_inputs(batch=2, seed=4100):
    """seeded head outputs in the NHWC layout Head.forward returns: boxes randn * 0.3, class logits randn - 3, direction logits randn"""
    g = torch.Generator().manual_seed(seed)
    box = torch.randn((batch, H, W, SLOTS * 7), generator=g) * 0.3
    cls = torch.randn((batch, H, W, SLOTS * 3), generator=g) - 3.0
    dirs = torch.randn((batch, H, W, SLOTS * 2), generator=g)
    return box, cls, dirs


def negative_sample(labels, n=4096, seed=4200):
    """flat indices (into [B*A]) of n seeded negative anchors"""
    neg = np.flatnonzero(np.asarray(labels).reshape(-1) == 0)
    return np.sort(np.random.default_rng(seed).choice(neg, size=n, replace=False))


def loss_restatement(box_preds, cls_preds, dir_preds, labels, reg_targets, anchors, params=LOSS_PARAMS, dtype=torch.float64):
    """MultiGroupHead.loss of the Waymo SECOND head for one task, restated with torch ops in `dtype`; returns the reference's dictionary
    (tensors).  anchors: [A, 7]."""
    pos_w, neg_w, alpha, gamma, sigma, loc_w, cls_w, dir_w, dir_offset = params
    b = labels.shape[0]
    box = box_preds.reshape(b, -1, 7).to(dtype)
    n_anchor = box.shape[1]
    cls = cls_preds.reshape(b, n_anchor, -1).to(dtype)
    dirs = dir_preds.reshape(b, n_anchor, 2).to(dtype)
    tgt = reg_targets.reshape(b, n_anchor, 7).to(dtype)
    labels = labels.long()
    pos, neg = labels > 0, labels == 0
    norm = pos.sum(1, keepdim=True).to(dtype).clamp(min=1.0)
    cls_weights = (neg.to(dtype) * neg_w + pos.to(dtype) * pos_w) / norm
    reg_weights = pos.to(dtype) / norm
    one_hot = F.one_hot(labels.clamp(min=0), cls.shape[-1] + 1)[..., 1:].to(dtype)
    ce = cls.clamp(min=0) - cls * one_hot + torch.log1p(torch.exp(-cls.abs()))
    p = torch.sigmoid(cls)
    p_t = one_hot * p + (1 - one_hot) * (1 - p)
    focal = (1 - p_t) ** gamma * (one_hot * alpha + (1 - one_hot) * (1 - alpha)) * ce * cls_weights.unsqueeze(-1)
    pred_r = torch.sin(box[..., 6:]) * torch.cos(tgt[..., 6:])
    tgt_r = torch.cos(box[..., 6:]) * torch.sin(tgt[..., 6:])
    diff = torch.cat([box[..., :6] - tgt[..., :6], pred_r - tgt_r], -1).abs()
    small = (diff <= 1 / sigma ** 2).to(dtype)
    loc = (small * 0.5 * (diff * sigma) ** 2 + (diff - 0.5 / sigma ** 2) * (1 - small)) * reg_weights.unsqueeze(-1)
    loc_red = loc.sum() / b * loc_w
    cls_red = focal.sum() / b * cls_w
    rot_gt = tgt[..., 6] + anchors.to(dtype)[None, :, 6] - dir_offset
    period = 2 * math.pi
    dir_tgt = ((rot_gt - torch.floor(rot_gt / period + 0.5) * period) > 0).long()
    dir_loss = (F.cross_entropy(dirs.reshape(-1, 2), dir_tgt.reshape(-1), reduction="none").reshape(b, n_anchor) * reg_weights).sum() / b
    return {"loss": loc_red + cls_red + dir_loss * dir_w, "cls_pos_loss": focal[..., 1:].sum() / b / pos_w,
            "cls_neg_loss": focal[..., 0].sum() / b / neg_w, "dir_loss_reduced": dir_loss, "cls_loss_reduced": cls_red,
            "loc_loss_reduced": loc_red, "loc_loss_elem": [loc[..., i].sum() / b for i in range(7)],
            "num_pos": pos[0].sum(), "num_neg": neg[0].sum()}


PREDICT_OBJECTS = 40


def predict_inputs(batch=2, seed=4300):
    """seeded head outputs for `predict`: every class logit sits at -6 except around PREDICT_OBJECTS fake objects per sample, where the
    two rotation slots of the object's class (and, for VEHICLE, of the cell to its right) get logits U(-1.5, 3): ~200 anchors pass
    score_threshold 0.1.  Objects sit on a 14-cell lattice so that different objects never touch."""
    g = torch.Generator().manual_seed(seed)
    box = torch.randn((batch, H, W, SLOTS, 7), generator=g) * 0.05
    dirs = torch.randn((batch, H, W, SLOTS, 2), generator=g)
    cls = torch.full((batch, H, W, SLOTS, 3), -6.0)
    lattice = [(y, x) for y in range(10, H - 10, 14) for x in range(10, W - 10, 14)]
    for b in range(batch):
        pick = torch.randperm(len(lattice), generator=g)[:PREDICT_OBJECTS].tolist()
        for i in pick:
            y, x = lattice[i]
            c = int(torch.randint(0, 3, (1,), generator=g))
            for dx in ((0, 1) if c == 0 else (0,)):
                for r in range(2):
                    cls[b, y, x + dx, 2 * c + r, c] = float(torch.rand(1, generator=g) * 4.5 - 1.5)
    return box.reshape(batch, H, W, -1), cls.reshape(batch, H, W, -1), dirs.reshape(batch, H, W, -1)


def _near_bbox(rb):
    lim = (rb[:, 4] - torch.floor(rb[:, 4] / np.float32(np.pi) + 0.5) * np.float32(np.pi)).abs()
    dims = torch.where((lim > np.float32(np.pi / 4))[:, None], rb[:, [3, 2]], rb[:, 2:4])
    return torch.cat([rb[:, :2] - dims / 2, rb[:, :2] + dims / 2], 1)


def assign_restatement(boxes, classes, anchors, matched, unmatched):
    """vectorised restatement of the assignment rules with torch ops on the tensors' device (float64 overlaps rounded once to fp32),
    frame by frame, class by class: boxes [B,K,7], classes [B,K] (0 = padding), anchors [A,7] -> labels i32[B,A], reg_targets
    f32[B,A,7], reg_weights f32[B,A].  tests/test_anchor_head_cpu.py pins it to the reference's labels."""
    from sparse2dense_amd.anchors import GroundBox3dCoder
    coder = GroundBox3dCoder()
    b, a = boxes.shape[0], anchors.shape[0]
    cells = anchors.view(-1, 6, 7)
    labels = torch.zeros((b, cells.shape[0], 6), dtype=torch.int32, device=boxes.device)
    targets = torch.zeros((b, cells.shape[0], 6, 7), device=boxes.device)
    two_pi = np.float32(np.pi * 2)
    for f in range(b):
        for c in range(3):
            sel = boxes[f][classes[f] == c + 1]
            if sel.shape[0] == 0:
                continue
            sel = torch.cat([sel[:, :6], (sel[:, 6] - torch.floor(sel[:, 6] / two_pi + 0.5) * two_pi)[:, None]], 1)
            an = cells[:, 2 * c:2 * c + 2].reshape(-1, 7)
            p, q = _near_bbox(an[:, [0, 1, 3, 4, 6]]).double(), _near_bbox(sel[:, [0, 1, 3, 4, 6]]).double()
            iw = torch.minimum(p[:, None, 2], q[None, :, 2]) - torch.maximum(p[:, None, 0], q[None, :, 0])
            ih = torch.minimum(p[:, None, 3], q[None, :, 3]) - torch.maximum(p[:, None, 1], q[None, :, 1])
            ok = (iw > 0) & (ih > 0)
            ua = ((p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]))[:, None] + ((q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1]))[None] - iw * ih
            iou = torch.where(ok, iw * ih / torch.where(ok, ua, torch.ones_like(ua)), torch.zeros_like(ua)).float()
            best, arg = iou.max(1)
            col = iou.max(0)[0]
            col = torch.where(col == 0, -torch.ones_like(col), col)
            pos = (iou == col[None]).any(1) | (best >= matched[c])
            lab = torch.where(pos, torch.full_like(arg, c + 1), torch.where(best < unmatched[c], torch.zeros_like(arg), -torch.ones_like(arg)))
            enc = coder.encode_torch(sel[arg], an) * pos[:, None]
            labels[f, :, 2 * c:2 * c + 2] = lab.view(-1, 2).int()
            targets[f, :, 2 * c:2 * c + 2] = enc.view(-1, 2, 7)
    labels = labels.view(b, a)
    return labels, targets.view(b, a, 7), (labels > 0).float()


def golden_targets(npz):
    """dense labels i32[3,A], reg_targets f32[3,A,7], reg_weights f32[3,A] of anchor_targets.npz (the targets are stored sparse)"""
    labels = npz["labels"].astype(np.int32)
    targets = np.zeros(labels.shape + (7,), np.float32)
    idx = npz["pos_index"]
    targets[idx[:, 0], idx[:, 1]] = npz["pos_targets"]
    return labels, targets, (labels > 0).astype(np.float32)
