"""MultiGroupHead.predict on the device (csrc/anchor_predict.hip): the score of every anchor of every task and sample in one launch, one
sort, the decode of the candidates only, the batched rotated NMS (nms.rotate_nms_batched) and one finishing launch (range cut, direction
flip, label bases) - instead of the dense decode of anchors.decode_anchors and the per-(task, sample) torch chain of
MultiGroupHead.predict_torch (det3d/models/bbox_heads/mg_head.py:697-1086, single-class rotated-NMS branch).
A SEGMENT is one (task, sample) pair, segment = task * samples + sample.
`StaticAnchorPlan` (below) is the same predict without the host: the device top-K select (csrc/segment_topk.hip) in place of the sort,
fixed-capacity buffers allocated once, launches only - the form a HIP graph can hold."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .center_predict import MAX_TASKS, NMS_MAX_BOXES, NMS_MAX_WORKSPACE_BYTES, TOPK_MAX, StaticDetections, _cfg_get, _stream  # noqa: F401  (the same bounds)

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


# ---- predict without the host: fixed-capacity buffers, launches only, capturable into one HIP graph --------------------------------------
def _nms_get(test_cfg):
    get = _cfg_get(test_cfg)
    nms_cfg = get("nms")
    return get, ((lambda k: nms_cfg[k]) if isinstance(nms_cfg, dict) else (lambda k: getattr(nms_cfg, k)))


def _static_inputs(preds_dicts, anchors, use_direction):
    """the refusals of the static path that concern the predictions and the anchor tables, before any HIP call: it reads them in place, so
    it can neither widen nor copy.  Returns (samples, device)."""
    if not 1 <= len(preds_dicts) <= MAX_TASKS:
        raise _lib.S2DError(f"predict_static: {len(preds_dicts)} tasks (1..{MAX_TASKS} supported)")
    if len(anchors) != len(preds_dicts):
        raise _lib.S2DError(f"predict_static: {len(anchors)} anchor tables for {len(preds_dicts)} tasks")
    for i, (preds, table) in enumerate(zip(preds_dicts, anchors)):
        if use_direction and preds.get("dir_cls_preds") is None:
            raise _lib.S2DError(f"predict_static: task {i} has no dir_cls_preds (the head uses the direction classifier)")
        named = [("box_preds", preds["box_preds"]), ("cls_preds", preds["cls_preds"]), ("anchors", table)]
        if use_direction:
            named.append(("dir_cls_preds", preds["dir_cls_preds"]))
        for name, t in named:
            if not torch.is_tensor(t) or not t.is_cuda:
                raise _lib.S2DError(f"predict_static: task {i}: CUDA tensors expected (no CPU fallback), '{name}' is not one")
            if t.dtype != torch.float32:
                raise _lib.S2DError(f"predict_static: task {i}: '{name}' is {t.dtype}: fp32 only (the static path does not widen)")
            if not t.is_contiguous():
                raise _lib.S2DError(f"predict_static: task {i}: '{name}' is not contiguous (the static path does not copy)")
    box0 = preds_dicts[0]["box_preds"]
    return int(box0.shape[0]), box0.device


class StaticAnchorPlan:
    """MultiGroupHead.predict for one (test_cfg, class counts, anchor tables, samples, direction settings, device) with every buffer
    allocated at build time.  `run` only launches on the current stream - score (with the zero-fill of its counts), top-K, boxes, the two
    kernels of the batched rotated NMS, finish: seven kernels - with no host read, no host-to-device copy, no allocation and no torch
    operator, so it can be captured into a HIP graph (one stream, a linear chain).  A captured graph holds the addresses of the
    prediction tensors and of the anchor tables: new predictions are written into the same tensors, and the graph is captured again if
    they move.
    k = nms_pre_max_size candidates per segment - the cut `predict` makes, so the results are equal whatever passes:
    overflow[s] = passed[s] > k only says that the cut was taken and marks no deviation from `predict`."""

    def __init__(self, test_cfg, num_classes, anchors, samples, use_direction, direction_offset, device):
        get, nget = _nms_get(test_cfg)
        device = torch.device(device)
        pre_max = nget("nms_pre_max_size")
        if pre_max is None or not 1 <= int(pre_max) <= TOPK_MAX:
            raise _lib.S2DError(f"StaticAnchorPlan: nms_pre_max_size {pre_max} (1..{TOPK_MAX} supported: the candidates per segment)")
        self.tasks, self.samples, self.k = len(num_classes), int(samples), int(pre_max)
        if not 1 <= self.tasks <= MAX_TASKS:
            raise _lib.S2DError(f"StaticAnchorPlan: {self.tasks} tasks (1..{MAX_TASKS} supported)")
        if len(anchors) != self.tasks:
            raise _lib.S2DError(f"StaticAnchorPlan: {len(anchors)} anchor tables for {self.tasks} tasks")
        if device.type != "cuda":
            raise _lib.S2DError("StaticAnchorPlan: a CUDA device expected (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.samples < 1:
            raise _lib.S2DError(f"StaticAnchorPlan: {samples} samples")
        for i, t in enumerate(anchors):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != 7 or t.shape[0] < 1:
                raise _lib.S2DError(f"StaticAnchorPlan: anchor table {i}: a contiguous fp32 [A, 7] tensor expected (the static path neither "
                                    "widens nor copies)")
            if t.device != device:
                raise _lib.S2DError(f"StaticAnchorPlan: anchor table {i} is on {t.device}, the plan is built for {device}")
        post_max = nget("nms_post_max_size")
        self.max_keep = self.k if post_max is None else min(self.k, int(post_max))
        if self.max_keep < 1:
            raise _lib.S2DError(f"StaticAnchorPlan: nms_post_max_size {post_max}")
        self.device, self.use_direction, self.direction_offset = device, bool(use_direction), float(direction_offset)
        self.classes = [int(c) for c in num_classes]
        self.label_bases = [sum(self.classes[:t]) for t in range(self.tasks)]
        self.anchors = list(anchors)   # kept alive: the kernels read them in place
        self.num_anchors = [int(t.shape[0]) for t in anchors]
        rng = get("post_center_limit_range")
        self.range6 = (ctypes.c_float * 6)(*[float(v) for v in rng]) if rng is not None and len(rng) > 0 else None
        self.threshold = float(np.float32(get("score_threshold")))
        self.iou_threshold = float(nget("nms_iou_threshold"))
        segs, a_max, k = self.tasks * self.samples, max(self.num_anchors), self.k
        self.segs, self.max_anchors, self.total, self.cap = segs, a_max, segs * k, self.tasks * self.max_keep
        if a_max > 1 << 20 or segs > 65535:
            raise _lib.S2DError(f"StaticAnchorPlan: {a_max} anchors per task, {segs} segments (s2d_segment_topk takes rows up to 2^20, the "
                                "kernels 65535 segments)")
        lib = _lib.load()
        from .nms import _ws
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
        self.score, self.label, self.passed = new((segs, a_max), torch.float32), new((segs, a_max), torch.int32), new((segs,), torch.int32)
        # row stride max_anchors, the first k columns filled: s2d_anchor_predict_boxes reads them as it reads a full sort
        self.order, self.score_sorted = new((segs, a_max), torch.int64), new((segs, a_max), torch.float32)
        self.table = new((3, segs), torch.int32)   # offsets, counts, overflow
        self.cand_boxes, self.cand_scores = new((self.total, 7), torch.float32), new((self.total,), torch.float32)
        self.cand_labels, self.cand_dirs, self.cand_in_range = new((self.total,), torch.int32), new((self.total,), torch.int32), new((self.total,), torch.uint8)
        self.keep, self.n_keep = new((segs, self.max_keep), torch.int64), new((segs,), torch.int32)
        self.nms_ws = _ws(lib.s2d_nms_batched_workspace_bytes(self.total, k), device)
        self.boxes, self.scores = new((self.samples, self.cap, 7), torch.float32), new((self.samples, self.cap), torch.float32)
        self.labels, self.counts = new((self.samples, self.cap), torch.int64), new((self.samples,), torch.int32)
        self.out = StaticDetections(self.boxes, self.scores, self.labels, self.counts, self.table[2])

    def buffers(self):
        """every device buffer of the plan by name (none is ever reallocated); the anchor tables as anchors_0 .."""
        names = ("score", "label", "passed", "order", "score_sorted", "table", "cand_boxes", "cand_scores", "cand_labels", "cand_dirs", "cand_in_range",
                 "keep", "n_keep", "nms_ws", "boxes", "scores", "labels", "counts")
        return dict({n: getattr(self, n) for n in names}, **{f"anchors_{i}": t for i, t in enumerate(self.anchors)})

    def _task_table(self, preds_dicts):
        if len(preds_dicts) != self.tasks:
            raise _lib.S2DError(f"StaticAnchorPlan.run: {len(preds_dicts)} tasks, the plan was built for {self.tasks}")
        _static_inputs(preds_dicts, self.anchors, self.use_direction)
        table = (_lib.AnchorPredictTask * self.tasks)()
        for i, (rec, preds, anchors, a, classes, base) in enumerate(zip(table, preds_dicts, self.anchors, self.num_anchors, self.classes,
                                                                       self.label_bases)):
            box, cls = preds["box_preds"], preds["cls_preds"]
            dirs = preds["dir_cls_preds"] if self.use_direction else None
            b = self.samples
            if box.shape[0] != b or cls.shape[0] != b or box.numel() != b * a * 7 or cls.numel() != b * a * classes \
                    or (dirs is not None and (dirs.shape[0] != b or dirs.numel() != b * a * 2)) \
                    or any(t.device != self.device for t in (box, cls, dirs) if t is not None):
                raise _lib.S2DError(f"StaticAnchorPlan.run: task {i}: box_preds {tuple(box.shape)}, cls_preds {tuple(cls.shape)} on {box.device}; "
                                    f"the plan was built for {b} samples, {a} anchors, {classes} classes on {self.device}")
            rec.box_preds, rec.cls_preds, rec.anchors = box.data_ptr(), cls.data_ptr(), anchors.data_ptr()
            rec.dir_cls_preds = None if dirs is None else dirs.data_ptr()
            rec.num_anchors, rec.classes, rec.label_base = a, classes, base
        return table

    def run(self, preds_dicts):
        """launches only, on the current stream; returns the plan's `StaticDetections` (the same tensors at every call)"""
        table = self._task_table(preds_dicts)   # host only: the pointers of the predictions, read in place
        lib, st, ptr = _lib.load(), _stream(self.device), lambda t: t.data_ptr()
        offsets, counts, overflow = (self.table[i].data_ptr() for i in range(3))
        a_max = self.max_anchors
        _lib.check(lib.s2d_anchor_predict_score(table, self.tasks, self.samples, a_max, self.threshold, ptr(self.score), ptr(self.label),
                                                ptr(self.passed), st), "s2d_anchor_predict_score")
        _lib.check(lib.s2d_segment_topk(ptr(self.score), self.segs, a_max, a_max, self.k, ptr(self.passed), ptr(self.order), ptr(self.score_sorted),
                                        a_max, offsets, counts, overflow, st), "s2d_segment_topk")
        _lib.check(lib.s2d_anchor_predict_boxes(table, self.tasks, self.samples, a_max, self.range6, ptr(self.order), ptr(self.score_sorted),
                                                ptr(self.label), offsets, counts, self.k, self.total, ptr(self.cand_boxes), ptr(self.cand_scores),
                                                ptr(self.cand_labels), ptr(self.cand_dirs), ptr(self.cand_in_range), st), "s2d_anchor_predict_boxes")
        _lib.check(lib.s2d_nms_rotated_bev_batched(ptr(self.cand_boxes), 7, offsets, counts, self.segs, self.k, self.total, self.iou_threshold,
                                                   self.max_keep, ptr(self.keep), ptr(self.n_keep), ptr(self.nms_ws), self.nms_ws.numel(), st),
                   "s2d_nms_rotated_bev_batched")
        _lib.check(lib.s2d_anchor_predict_finish_static(table, self.tasks, self.samples, ptr(self.cand_boxes), ptr(self.cand_scores),
                                                        ptr(self.cand_labels), ptr(self.cand_dirs), ptr(self.cand_in_range), offsets, counts,
                                                        self.total, ptr(self.keep), ptr(self.n_keep), self.max_keep, int(self.use_direction),
                                                        self.direction_offset, ptr(self.boxes), ptr(self.scores), ptr(self.labels),
                                                        ptr(self.counts), st), "s2d_anchor_predict_finish_static")
        return self.out


def static_plan_key(test_cfg, num_classes, anchors, samples, use_direction, direction_offset, device):
    """what a StaticAnchorPlan depends on, as a hashable key (MultiGroupHead.predict_static caches plans by it)"""
    get, nget = _nms_get(test_cfg)
    flat = lambda v: None if v is None else tuple(float(x) for x in v)
    return (float(get("score_threshold")), flat(get("post_center_limit_range")), nget("nms_pre_max_size"), nget("nms_post_max_size"),
            float(nget("nms_iou_threshold")), tuple(int(c) for c in num_classes), tuple((int(t.data_ptr()), tuple(t.shape)) for t in anchors),
            int(samples), bool(use_direction), float(direction_offset), str(device))
