"""numpy restatement of the whole of MultiGroupHead.predict (single-class rotated-NMS branch, mg_head.py:697-1086) for any task table, and
the seeded inputs of the small-shape tests.  fp32 throughout: GroundBox3dCoder's decode, the sigmoid class maximum, the `>=` threshold, the
stable top nms_pre_max_size by descending score, oracle.iou_nms.rotate_nms on the converted boxes (heading negated), nms_post_max_size,
the direction flip, the centre-range mask, the label bases.  tests/test_anchor_predict_cpu.py pins it to tests/golden/anchor_predict.npz;
tests/test_anchor_predict_gpu.py uses it as the second reference of the device path."""
import copy

import numpy as np
import torch

from oracle import iou_nms
from sparse2dense_amd import anchors as A, waymo_configs as WC


def _np(t):
    return t.detach().float().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float32)


def candidates(box, cls, dirs, anchors, threshold):
    """one sample of one task: box [A, 7], cls [A, C], dirs [A, 2] or None, anchors [A, 7] -> the anchors with score >= threshold in anchor
    order: (index, boxes [n, 7], scores, labels, direction labels)"""
    e = np.exp(-np.abs(cls)).astype(np.float32)
    p = np.where(cls >= 0, np.float32(1) / (np.float32(1) + e), e / (np.float32(1) + e)).astype(np.float32)
    label = p.argmax(1)   # the first maximum wins
    score = p.max(1)
    idx = np.flatnonzero(score >= np.float32(threshold))
    boxes = A.GroundBox3dCoder().decode(box[idx], anchors[idx]).astype(np.float32)
    d = (dirs[idx, 1] > dirs[idx, 0]).astype(np.int32) if dirs is not None else np.zeros(len(idx), np.int32)
    return idx.astype(np.int32), boxes, score[idx], label[idx].astype(np.int32), d


def finish(cand, test_cfg, use_direction=True, direction_offset=0.0, range_first=False):
    """NMS, post_max, direction flip, range mask of one segment -> dict(box3d_lidar, scores, label_preds, index (anchor indices), flipped,
    nms_index (the anchors the NMS kept, before the range mask)).  range_first=True is the WRONG order (range mask in front of the NMS):
    the tests use it to show that their inputs tell the two orders apart."""
    idx, b, s, l, d = cand
    nms = test_cfg["nms"]
    pcr = test_cfg.get("post_center_limit_range")
    pcr = np.asarray(pcr, np.float32) if pcr is not None and len(pcr) > 0 else None

    def inside(x):
        return (x[:, :3] >= pcr[:3]).all(1) & (x[:, :3] <= pcr[3:]).all(1) if pcr is not None else np.ones(len(x), bool)
    if range_first:
        m = inside(b)
        idx, b, s, l, d = idx[m], b[m], s[m], l[m], d[m]
    if len(idx):
        sel = iou_nms.rotate_nms(np.concatenate([b[:, :6], -b[:, 6:7]], 1), s, nms["nms_iou_threshold"], nms["nms_pre_max_size"],
                                 nms["nms_post_max_size"])
        idx, b, s, l, d = idx[sel], b[sel].copy(), s[sel], l[sel], d[sel]
    nms_index = idx.copy()
    flipped = np.zeros(len(idx), bool)
    if len(idx) and use_direction:
        flipped = ((b[:, 6] - np.float32(direction_offset)) > 0) ^ d.astype(bool)
        b[:, 6] += np.where(flipped, np.float32(np.pi), np.float32(0.0))
    m = inside(b)
    return dict(box3d_lidar=b[m], scores=s[m], label_preds=l[m].astype(np.int64), index=idx[m], flipped=flipped[m], nms_index=nms_index)


def predict(preds_dicts, anchors, test_cfg, num_classes, use_direction=True, direction_offset=0.0, range_first=False):
    """preds_dicts: one dict per task (box_preds, cls_preds, dir_cls_preds: tensors or arrays, [B, ...]); anchors: one [A_t, 7] table per task.
    -> (per-sample dicts with the tasks concatenated in task order and the labels offset, segments[task][sample] = (candidates, finish))"""
    segments = []
    for preds, table in zip(preds_dicts, anchors):
        table = _np(table)
        a = table.shape[0]
        box, cls = _np(preds["box_preds"]), _np(preds["cls_preds"])
        b = box.shape[0]
        box, cls = box.reshape(b, a, 7), cls.reshape(b, a, -1)
        dirs = _np(preds["dir_cls_preds"]).reshape(b, a, 2) if use_direction and preds.get("dir_cls_preds") is not None else None
        task = []
        for i in range(b):
            cand = candidates(box[i], cls[i], None if dirs is None else dirs[i], table, test_cfg["score_threshold"])
            task.append((cand, finish(cand, test_cfg, use_direction, direction_offset, range_first)))
        segments.append(task)
    out = []
    for i in range(len(segments[0])):
        fins = [task[i][1] for task in segments]
        bases = [sum(num_classes[:t]) for t in range(len(fins))]
        out.append(dict(box3d_lidar=np.concatenate([f["box3d_lidar"] for f in fins]), scores=np.concatenate([f["scores"] for f in fins]),
                        label_preds=np.concatenate([f["label_preds"] + base for f, base in zip(fins, bases)])))
    return out, segments


# ---- the small-shape case -------------------------------------------------------------------------------------------------------------
SMALL_H, SMALL_W, SMALL_B = 5, 7, 3
SMALL_SPECIAL = (2, 3)   # the cell whose best box lies just outside the range and suppresses one just inside


def second_table(h, w):
    return A.get_assigner(WC.SECOND_ASSIGNER).anchors_numpy([1, h, w])


def small_case(seed=4400):
    """(box, cls, dirs [3, 5, 7, .] tensors, anchors [210, 7] array, test_cfg): the Waymo SECOND head on a 5 x 7 grid - 210 anchors, no multiple
    of 64 - with nms_pre_max_size 16, nms_post_max_size 5 and a range whose xmax is the centre of column 3.  Every class logit sits at
    -6 except (the lattice idea of anchor_util.predict_inputs: a cell is ~21 m wide, boxes of different cells never touch):
      frame 0: three slots in each of 8 cells pass (24 > 16: the pre_max cut is taken)
      frame 1: one slot in each of 7 cells passes, two of them with the SAME logit 3.5 (the tie, and the two best of the frame); in the
               special cell slot 0 (logit 3.2, the third best) is shifted by +0.05 diagonals to x > xmax and slot 1 (logit 1.0) by -0.05
               to x < xmax: the NMS keeps slot 0, which suppresses slot 1, and the range mask then drops slot 0.  8 boxes survive the
               NMS (> 5: the post_max cut is taken)
      frame 2: nothing passes"""
    g = torch.Generator().manual_seed(seed)
    b, h, w = SMALL_B, SMALL_H, SMALL_W
    box = torch.randn((b, h, w, 6, 7), generator=g) * 0.05
    dirs = torch.randn((b, h, w, 6, 2), generator=g)
    cls = torch.full((b, h, w, 6, 3), -6.0)
    cells = [(y, x) for y in range(h) for x in range(w) if (y, x) != SMALL_SPECIAL]

    def logit():
        return float(torch.rand(1, generator=g) * 4.5 - 1.5)
    for i in torch.randperm(len(cells), generator=g)[:8].tolist():
        y, x = cells[i]
        for slot in torch.randperm(6, generator=g)[:3].tolist():
            cls[0, y, x, slot, slot // 2] = logit()
    left = [c for c in cells if c[1] < SMALL_SPECIAL[1]]   # the tied boxes lie inside the range
    tied = [left[i] for i in torch.randperm(len(left), generator=g)[:2].tolist()]
    rest = [c for c in cells if c not in tied]
    for n, (y, x) in enumerate(tied + [rest[i] for i in torch.randperm(len(rest), generator=g)[:5].tolist()]):
        slot = int(torch.randint(0, 6, (1,), generator=g))
        cls[1, y, x, slot, slot // 2] = 3.5 if n < 2 else logit()
    y, x = SMALL_SPECIAL
    cls[1, y, x, 0, 0], cls[1, y, x, 1, 0] = 3.2, 1.0
    box[1, y, x, 0, 0], box[1, y, x, 1, 0] = 0.05, -0.05
    table = second_table(h, w)
    cfg = copy.deepcopy(WC.SECOND_TEST_CFG)
    cfg["nms"].update(nms_pre_max_size=16, nms_post_max_size=5)
    xmax = float(table.reshape(h, w, 6, 7)[y, x, 0, 0])
    cfg["post_center_limit_range"] = [-80, -80, -10.0, xmax, 80, 10.0]
    return box.reshape(b, h, w, -1), cls.reshape(b, h, w, -1), dirs.reshape(b, h, w, -1), table, cfg


def check_small_case(box, cls, dirs, table, cfg):
    """asserts, on the host, every property the small case is built for; returns the restatement's result"""
    preds = [dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)]
    out, segments = predict(preds, [table], cfg, [3])
    _, wrong = predict(preds, [table], cfg, [3], range_first=True)
    nms, thr = cfg["nms"], cfg["nms"]["nms_iou_threshold"]
    passed = [len(c[0]) for c, _ in segments[0]]
    assert passed[0] > nms["nms_pre_max_size"] and passed[2] == 0 and 0 < passed[1] <= nms["nms_pre_max_size"], passed
    for (idx, b, s, l, d), _ in segments[0]:   # no candidate pair near the NMS decision boundary
        nb = np.concatenate([b[:, :6], -b[:, 6:7]], 1)
        iou = iou_nms.bev_iou(nb, nb)
        assert not ((iou > thr / 2) & (iou < 2 * thr)).any()
    cand1, fin1 = segments[0][1]
    uncut = finish(cand1, dict(cfg, nms=dict(nms, nms_post_max_size=None)), range_first=False)
    assert len(uncut["nms_index"]) > nms["nms_post_max_size"] and len(fin1["nms_index"]) == nms["nms_post_max_size"]   # the post_max cut
    # a kept box outside the range suppresses a box inside it: the range mask in front of the NMS gives another result
    special = (SMALL_SPECIAL[0] * SMALL_W + SMALL_SPECIAL[1]) * 6
    assert special in fin1["nms_index"] and special not in fin1["index"] and special + 1 not in fin1["index"]
    assert special + 1 in wrong[0][1][1]["index"]
    flipped = np.concatenate([f["flipped"] for _, f in segments[0]])
    assert flipped.any() and not flipped.all()
    s1 = cand1[2]
    assert (s1 == s1.max()).sum() == 2 and np.array_equal(fin1["scores"][:2], [s1.max()] * 2) and fin1["index"][0] < fin1["index"][1]   # the tie
    return out, segments


# ---- the two-task case ----------------------------------------------------------------------------------------------------------------
TWO_TASKS = [dict(num_class=1, class_names=["VEHICLE"]), dict(num_class=2, class_names=["PEDESTRIAN", "CYCLIST"])]


def two_task_head():
    from sparse2dense_amd.registry import build_head
    cfg = copy.deepcopy(WC.second_voxelnet_train()["bbox_head"])
    cfg.update(tasks=copy.deepcopy(TWO_TASKS), weights=[1, 1])
    return build_head(cfg)


def two_task_case(seed=4500, h=8, w=8, batch=2):
    """(preds_dicts, anchor tables): task 0 with one class (2 anchors per cell, 128 anchors), task 1 with two (4 per cell, 256 anchors) on an
    8 x 8 grid: the score maps of task 0 are padded to 256 columns.  Logits -6 except one or two slots in 10 cells per task and sample."""
    gens = A.get_assigner(WC.SECOND_ASSIGNER).generators
    tables = [A.generate_anchors(gens[:1], [1, h, w]), A.generate_anchors(gens[1:], [1, h, w])]
    g = torch.Generator().manual_seed(seed)
    preds = []
    for classes in (1, 2):
        slots = 2 * classes
        box = torch.randn((batch, h, w, slots, 7), generator=g) * 0.05
        dirs = torch.randn((batch, h, w, slots, 2), generator=g)
        cls = torch.full((batch, h, w, slots, classes), -6.0)
        for b in range(batch):
            for i in torch.randperm(h * w, generator=g)[:10].tolist():
                for slot in torch.randperm(slots, generator=g)[:int(torch.randint(1, 3, (1,), generator=g))].tolist():
                    cls[b, i // w, i % w, slot, slot // 2] = float(torch.rand(1, generator=g) * 4.5 - 1.5)
        preds.append(dict(box_preds=box.reshape(batch, h, w, -1), cls_preds=cls.reshape(batch, h, w, -1),
                          dir_cls_preds=dirs.reshape(batch, h, w, -1)))
    return preds, tables
