"""MultiGroupHead.predict on the device (csrc/anchor_predict.hip): the score of every anchor of every task and sample in one launch, one
sort, the decode of the candidates only, the batched rotated NMS (nms.rotate_nms_batched) and one finishing launch (range cut, direction
flip, label bases) - instead of the dense decode of anchors.decode_anchors and the per-(task, sample) torch chain of
MultiGroupHead.predict_torch (det3d/models/bbox_heads/mg_head.py:697-1086, single-class rotated-NMS branch).
A SEGMENT is one (task, sample) pair, segment = task * samples + sample."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .center_predict import MAX_TASKS, NMS_MAX_BOXES, NMS_MAX_WORKSPACE_BYTES, _cfg_get, _stream  # noqa: F401  (the same bounds)

# boxes [N, 7] fp32 in the NMS form (x, y, z, w, l, h, -r), scores [N] fp32, labels [N] int32 (class inside the task), dirs [N] int32,
# in_range [N] uint8: the candidates of all segments, each segment's sorted by descending score (ties by anchor index); counts / offsets:
# per segment, python lists; segments: int32 [2, S] on the device (offsets, counts); passed: the anchors of each segment that passed the
# score threshold (>= counts when nms_pre_max_size cuts); table: the s2d_anchor_predict_task array the kernels took
Candidates = namedtuple("Candidates", "boxes scores labels dirs in_range counts offsets segments passed samples tasks table")


def segment_layout(passed, pre_max_size=None):
    """(counts, offsets, total) of the packed candidate lists from the per-segment pass counts: every segment keeps its pre_max_size best
    (None: all), its rows start where the previous segment's end"""
    counts = [int(c) if pre_max_size is None else min(int(c), int(pre_max_size)) for c in passed]
    offsets, total = [], 0
    for c in counts:
        offsets.append(total)
        total += c
    return counts, offsets, total


def assembly_rows(final_counts, tasks, samples, max_keep):
    """(rows, sizes): the rows of the padded [S, max_keep] outputs in output order - sample by sample, inside a sample task by task,
    inside a task in keep order - and the number of rows of every sample"""
    rows, sizes = [], []
    for b in range(samples):
        n = 0
        for t in range(tasks):
            s = t * samples + b
            rows.extend(range(s * max_keep, s * max_keep + int(final_counts[s])))
            n += int(final_counts[s])
        sizes.append(n)
    return rows, sizes


def _task_table(preds_dicts, anchors, label_bases, use_direction):
    """(ctypes array of s2d_anchor_predict_task, tensors kept alive, samples, max_anchors): fp32 contiguous predictions are read in place,
    anything else is widened / made contiguous first, as anchors.decode_anchors does"""
    table = (_lib.AnchorPredictTask * len(preds_dicts))()
    alive = []
    samples = int(preds_dicts[0]["box_preds"].shape[0])
    max_anchors = 0
    for i, (rec, preds, table_t, base) in enumerate(zip(table, preds_dicts, anchors, label_bases)):
        box, cls = preds["box_preds"], preds["cls_preds"]
        dirs = preds.get("dir_cls_preds") if use_direction else None
        a = int(table_t.shape[0])
        if box.shape[0] != samples or box.numel() != samples * a * 7 or (samples * a and cls.numel() % (samples * a)) \
                or cls.shape[0] != samples or (dirs is not None and dirs.numel() != samples * a * 2) or tuple(table_t.shape) != (a, 7):
            raise _lib.S2DError(f"decode_anchor_candidates: task {i}: shapes disagree (box_preds {tuple(box.shape)}, cls_preds "
                                f"{tuple(cls.shape)}, anchors {tuple(table_t.shape)})")
        ptrs = []
        for t in (box, cls, dirs, table_t):
            if t is not None:
                t = t.float().contiguous()   # (no copy for fp32 contiguous tensors)
                alive.append(t)
            ptrs.append(None if t is None else t.data_ptr())
        rec.box_preds, rec.cls_preds, rec.dir_cls_preds, rec.anchors = ptrs
        rec.num_anchors = a
        rec.classes = cls.numel() // (samples * a) if samples * a else 1
        rec.label_base = int(base)
        max_anchors = max(max_anchors, a)
    return table, alive, samples, max_anchors


def decode_anchor_candidates(preds_dicts, anchors, test_cfg, use_direction=True, label_bases=None):
    """Candidates of every (task, sample) segment of a MultiGroupHead from its raw predictions.

    preds_dicts: one dict per task (at most 8) of CUDA tensors box_preds [B, ..., 7 per anchor], cls_preds, dir_cls_preds (read when
    use_direction); anchors: one [A_t, 7] CUDA table per task.  test_cfg supplies score_threshold (rounded to fp32, `>=`),
    post_center_limit_range (empty: every row is in range) and nms.nms_pre_max_size (None: no cut).
    Runs on the current stream; ONE host read (the per-segment pass counts).  Returns `Candidates`."""
    tensors = [v for p in preds_dicts for k, v in p.items() if k in ("box_preds", "cls_preds", "dir_cls_preds")] + list(anchors)
    if not all(torch.is_tensor(v) and v.is_cuda for v in tensors):
        raise _lib.S2DError("decode_anchor_candidates: CUDA tensors expected (no CPU fallback)")
    if not 1 <= len(preds_dicts) <= MAX_TASKS:
        raise _lib.S2DError(f"decode_anchor_candidates: {len(preds_dicts)} tasks (1..{MAX_TASKS} supported)")
    lib = _lib.load()
    get = _cfg_get(test_cfg)
    nms_cfg = get("nms")
    pre_max = nms_cfg.get("nms_pre_max_size") if isinstance(nms_cfg, dict) else getattr(nms_cfg, "nms_pre_max_size", None)
    tasks = len(preds_dicts)
    table, alive, samples, max_anchors = _task_table(preds_dicts, anchors, label_bases or [0] * tasks, use_direction)
    dev = preds_dicts[0]["box_preds"].device
    segs = tasks * samples
    rng = get("post_center_limit_range")
    rng = (ctypes.c_float * 6)(*[float(v) for v in rng]) if rng is not None and len(rng) > 0 else None
    st = _stream(dev)
    score = torch.empty((segs, max_anchors), dtype=torch.float32, device=dev)
    label = torch.empty((segs, max_anchors), dtype=torch.int32, device=dev)
    count = torch.empty((segs,), dtype=torch.int32, device=dev)
    _lib.check(lib.s2d_anchor_predict_score(table, tasks, samples, max_anchors, float(np.float32(get("score_threshold"))), score.data_ptr(),
                                            label.data_ptr(), count.data_ptr(), st), "s2d_anchor_predict_score")
    # descending score, ties by anchor index: the order the per-segment chain produced (mask compaction, then rotate_nms's stable sort)
    score_sorted, order = torch.sort(score, dim=1, descending=True, stable=True)
    passed = count.tolist()   # host read 1
    counts, offsets, total = segment_layout(passed, pre_max)
    segments = torch.tensor([offsets, counts], dtype=torch.int32).reshape(2, segs).to(dev)
    boxes = torch.empty((total, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((total,), dtype=torch.float32, device=dev)
    labels = torch.empty((total,), dtype=torch.int32, device=dev)
    dirs = torch.empty((total,), dtype=torch.int32, device=dev)
    in_range = torch.empty((total,), dtype=torch.uint8, device=dev)
    if total:
        _lib.check(lib.s2d_anchor_predict_boxes(table, tasks, samples, max_anchors, rng, order.data_ptr(), score_sorted.data_ptr(),
                                                label.data_ptr(), segments[0].data_ptr(), segments[1].data_ptr(), max(counts), total,
                                                boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), dirs.data_ptr(), in_range.data_ptr(), st),
                   "s2d_anchor_predict_boxes")
    del alive
    return Candidates(boxes, scores, labels, dirs, in_range, counts, offsets, segments, passed, samples, tasks, table)


def predict_on_device(preds_dicts, anchors, test_cfg, num_classes, use_direction=True, direction_offset=0.0):
    """decode + batched rotated NMS + finish + per-sample assembly: a list of (boxes [n, 7], scores [n], labels [n] int64) per sample, tasks
    concatenated in task order and labels offset by the class counts of the earlier tasks - or None when a segment exceeds the NMS
    kernels' limit or the batched NMS workspace would exceed NMS_MAX_WORKSPACE_BYTES (the caller then takes the per-segment chain).
    Two host reads per call: the pass counts and the final counts."""
    from .nms import rotate_nms_batched
    get = _cfg_get(test_cfg)
    nms_cfg = get("nms")
    nget = (lambda k: nms_cfg[k]) if isinstance(nms_cfg, dict) else (lambda k: getattr(nms_cfg, k))
    bases = [sum(num_classes[:t]) for t in range(len(preds_dicts))]
    cand = decode_anchor_candidates(preds_dicts, anchors, test_cfg, use_direction, bases)
    dev = cand.boxes.device
    if sum(cand.counts) == 0:   # no anchor passed anywhere: neither the NMS nor the finish is launched
        empty = (cand.boxes, cand.scores, torch.empty((0,), dtype=torch.int64, device=dev))
        return [empty for _ in range(cand.samples)]
    if max(cand.counts) > NMS_MAX_BOXES:
        return None
    lib = _lib.load()
    if lib.s2d_nms_batched_workspace_bytes(sum(cand.counts), max(cand.counts)) > NMS_MAX_WORKSPACE_BYTES:
        return None
    keep, n_keep = rotate_nms_batched(cand.boxes, cand.segments, cand.counts, nget("nms_iou_threshold"), nget("nms_post_max_size"),
                                      n_keep_on_device=True)
    segs, max_keep = keep.shape
    out_boxes = torch.empty((segs * max_keep, 7), dtype=torch.float32, device=dev)
    out_scores = torch.empty((segs * max_keep,), dtype=torch.float32, device=dev)
    out_labels = torch.empty((segs * max_keep,), dtype=torch.int64, device=dev)
    out_count = torch.empty((segs,), dtype=torch.int32, device=dev)
    _lib.check(lib.s2d_anchor_predict_finish(cand.table, cand.tasks, cand.samples, cand.boxes.data_ptr(), cand.scores.data_ptr(),
                                             cand.labels.data_ptr(), cand.dirs.data_ptr(), cand.in_range.data_ptr(), cand.segments[0].data_ptr(),
                                             cand.segments[1].data_ptr(), int(cand.boxes.shape[0]), keep.data_ptr(), n_keep.data_ptr(), max_keep,
                                             int(bool(use_direction)), float(direction_offset), out_boxes.data_ptr(), out_scores.data_ptr(),
                                             out_labels.data_ptr(), out_count.data_ptr(), _stream(dev)), "s2d_anchor_predict_finish")
    rows, sizes = assembly_rows(out_count.tolist(), cand.tasks, cand.samples, max_keep)   # host read 2
    rows = torch.tensor(rows, dtype=torch.int64).to(dev)
    return list(zip(out_boxes[rows].split(sizes), out_scores[rows].split(sizes), out_labels[rows].split(sizes)))
