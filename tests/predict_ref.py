"""Float64 numpy restatement of CenterHead.predict (/root/reference/det3d/models/bbox_heads/center_head.py:293-507): several tasks, the
velocity branch, double-flip averaging, score / centre-range filter and both NMS forms (over oracle.iou_nms).  Test infrastructure only.

`predict` also measures how far the inputs keep from every decision a last-ulp difference could flip (`Margins`); the GPU tests assert
those distances before they compare keep lists exactly."""
from dataclasses import dataclass

import numpy as np

from oracle import iou_nms as O


@dataclass
class Margins:
    score_threshold: float = np.inf   # min |score - threshold| over all pixels
    score_gap: float = np.inf         # min difference of two candidate scores of one segment
    nms: float = np.inf               # min |IoU - threshold| (rotated) or |d2 - radius| / radius (circle) over candidate pairs
    range: float = np.inf             # min distance of a score-passing centre coordinate from a range limit
    candidates: tuple = ()            # candidates per segment (task-major), before the pre_max cut

    def check(self):
        assert self.score_threshold >= 1e-4, self
        assert self.score_gap >= 1e-6, self
        assert self.nms >= 1e-4, self
        assert self.range >= 1e-3, self


def _get(cfg, k, d=None):
    return cfg.get(k, d) if hasattr(cfg, "get") else getattr(cfg, k, d)


def decode(preds, cfg, double_flip):
    """one task: maps [images, C, H, W] -> (boxes [B, H*W, 7|9], class scores [B, H*W, classes]) in float64"""
    p = {k: np.asarray(v, np.float64).transpose(0, 2, 3, 1) for k, v in preds.items()}
    n, h, w, _ = p["hm"].shape
    if double_flip:
        assert n % 4 == 0
        n //= 4
        for k in p:
            v = p[k].reshape(n, 4, h, w, -1)
            p[k] = np.stack([v[:, 0], v[:, 1, ::-1], v[:, 2, :, ::-1], v[:, 3, ::-1, ::-1]], 1)
    with np.errstate(over="ignore", invalid="ignore"):
        hm, dim = 1 / (1 + np.exp(-p["hm"])), np.exp(p["dim"])
    rots, rotc = p["rot"][..., 0:1].copy(), p["rot"][..., 1:2].copy()
    reg, hei = p["reg"].copy(), p["height"]
    vel = p["vel"].copy() if "vel" in p else None
    if double_flip:
        hm, hei, dim = hm.mean(1), hei.mean(1), dim.mean(1)
        reg[:, 1, ..., 1] = 1 - reg[:, 1, ..., 1]
        reg[:, 2, ..., 0] = 1 - reg[:, 2, ..., 0]
        reg[:, 3, ..., 0] = 1 - reg[:, 3, ..., 0]
        reg[:, 3, ..., 1] = 1 - reg[:, 3, ..., 1]
        reg = reg.mean(1)
        rotc[:, 1] *= -1
        rots[:, 2] *= -1
        rots[:, 3] *= -1
        rotc[:, 3] *= -1
        rots, rotc = rots.mean(1), rotc.mean(1)
        if vel is not None:
            vel[:, 1, ..., 1] *= -1
            vel[:, 2, ..., 0] *= -1
            vel[:, 3] *= -1
            vel = vel.mean(1)
    rot = np.arctan2(rots, rotc)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    factor, vs, pc0 = _get(cfg, "out_size_factor"), _get(cfg, "voxel_size"), _get(cfg, "pc_range")
    x = (xs[None, :, :, None] + reg[..., 0:1]) * factor * vs[0] + pc0[0]
    y = (ys[None, :, :, None] + reg[..., 1:2]) * factor * vs[1] + pc0[1]
    parts = [x, y, hei, dim] + ([vel] if vel is not None else []) + [rot]
    boxes = np.concatenate(parts, -1).reshape(n, h * w, -1)
    return boxes, hm.reshape(n, h * w, -1)


def _pair_margin(boxes32, circular, thr):
    n = len(boxes32)
    if n < 2:
        return np.inf
    iu = np.triu_indices(n, 1)
    if circular:
        xy = boxes32[:, :2].astype(np.float64)
        d2 = ((xy[:, None] - xy[None]) ** 2).sum(-1)[iu]
        return float(np.min(np.abs(d2 - thr) / thr))
    return float(np.min(np.abs(O.bev_iou(boxes32, boxes32).astype(np.float64)[iu] - thr)))


def predict(preds_list, cfg, num_classes=None, pair_margins=True):
    """preds_list: one dict of numpy maps per task.  Returns (one dict per sample: box3d_lidar float32, scores float32, label_preds int64
    - tasks concatenated in task order, labels offset by the earlier tasks' class counts; Margins).  pair_margins=False skips the
    O(n^2) NMS margin of large candidate sets (Margins.nms stays inf)."""
    double_flip, circular = bool(_get(cfg, "double_flip", False)), bool(_get(cfg, "circular_nms", False))
    nms = _get(cfg, "nms")
    pre, post, iou_thr = nms["nms_pre_max_size"], nms["nms_post_max_size"], nms["nms_iou_threshold"]
    thr = _get(cfg, "score_threshold")
    rng = _get(cfg, "post_center_limit_range")
    rng = np.asarray(rng, np.float64) if rng is not None and len(rng) > 0 else None
    num_classes = num_classes or [p["hm"].shape[1] for p in preds_list]
    m = Margins()
    cands, per_task = [], []
    for t, preds in enumerate(preds_list):
        boxes, hm = decode(preds, cfg, double_flip)
        res = []
        for b in range(len(boxes)):
            with np.errstate(invalid="ignore"):
                scores, labels = hm[b].max(-1), hm[b].argmax(-1)   # numpy's max propagates NaN as torch.max does
                mask = scores > thr
                m.score_threshold = min(m.score_threshold, float(np.nanmin(np.abs(scores - thr))))
                if rng is not None:
                    c = boxes[b][mask, :3]
                    if len(c):
                        m.range = min(m.range, float(np.min(np.abs(c - rng[:3]))), float(np.min(np.abs(c - rng[3:]))))
                    mask &= np.all(boxes[b][:, :3] >= rng[:3], 1) & np.all(boxes[b][:, :3] <= rng[3:], 1)
            bx, sc, lb = boxes[b][mask], scores[mask], labels[mask]
            cands.append(int(mask.sum()))
            if len(sc) > 1:
                m.score_gap = min(m.score_gap, float(np.min(np.diff(np.sort(sc)))))
            bx32 = bx.astype(np.float32)
            order = np.argsort(-sc, kind="stable")
            if circular:
                radius = _get(cfg, "min_radius")[t]
                if pair_margins:
                    m.nms = min(m.nms, _pair_margin(bx32[order], True, radius))
                sel = O.circle_nms(bx32[:, :2], sc.astype(np.float32), radius, post)
            else:
                b7 = bx32[:, [0, 1, 2, 3, 4, 5, -1]]
                if pair_margins:
                    m.nms = min(m.nms, _pair_margin(b7[order[:pre]], False, iou_thr))
                sel = O.rotate_nms(b7, sc.astype(np.float32), iou_thr, pre, post)
            res.append((bx32[sel], sc[sel].astype(np.float32), lb[sel].astype(np.int64) + sum(num_classes[:t])))
        per_task.append(res)
    m.candidates = tuple(cands)
    out = []
    for b in range(len(per_task[0])):
        out.append(dict(box3d_lidar=np.concatenate([r[b][0] for r in per_task]), scores=np.concatenate([r[b][1] for r in per_task]),
                        label_preds=np.concatenate([r[b][2] for r in per_task])))
    return out, m
