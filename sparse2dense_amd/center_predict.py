"""CenterHead.predict on the device (csrc/center_predict.hip): the decode of every task and sample of a head in two launches around one
sort, and the assembly of the per-sample results from the batched NMS (nms.rotate_nms_batched / nms.circle_nms_batched).
Replaces the per-task torch chain of /root/reference/det3d/models/bbox_heads/center_head.py:311-419 and the per-(task, sample) chain
of :452-495.  A SEGMENT is one (task, sample) pair, segment = task * samples + sample.
`StaticPredictPlan` (below) is the same predict without the host: a device top-K select (csrc/segment_topk.hip) in place of the sort,
fixed-capacity buffers allocated once, launches only - the form a HIP graph can hold."""
import ctypes
from collections import namedtuple

import torch

from . import _lib

MAX_TASKS = 8
NMS_MAX_BOXES = 65536   # limit of the NMS kernels (one suppression row is walked by one workgroup)
# The batched NMS holds the suppression bits of ALL segments at once, every row as long as the largest segment's: total * ceil(max n / 64)
# words.  A few MB for trained heat maps; an untrained one under the circle NMS (no pre_max cut) can pass every pixel - 6 tasks x 4
# samples x 180 x 180 rows would ask for ~3 GB where the per-segment chain holds one segment's 130 MB.  Above this bound the call takes
# the chain.
NMS_MAX_WORKSPACE_BYTES = 256 << 20
_MAPS = ("hm", "reg", "height", "dim", "vel", "rot")
_CHANNELS = dict(reg=2, height=1, dim=3, vel=2, rot=2)

# boxes [N, 7 | 9] fp32, scores [N] fp32, labels [N] int64: the candidates of all segments, each segment's sorted by descending score
# (ties by pixel index); counts / offsets: per segment, python lists; segments: int32 [2, S] on the device (offsets, counts);
# passed: the number of pixels of each segment that passed the score / range test (>= counts when pre_max_size cuts)
Candidates = namedtuple("Candidates", "boxes scores labels counts offsets segments passed samples tasks")


def _stream(dev):
    return torch._C._cuda_getCurrentRawStream(dev.index)


def _cfg_get(test_cfg):
    return (lambda k, d=None: test_cfg.get(k, d)) if hasattr(test_cfg, "get") else (lambda k, d=None: getattr(test_cfg, k, d))


def _task_table(preds_dicts, label_bases):
    """(ctypes array of s2d_center_predict_task, tensors kept alive): fp32 maps read in place when NCHW-contiguous or channels_last"""
    table = (_lib.CenterPredictTask * len(preds_dicts))()
    alive = []
    has_vel = "vel" in preds_dicts[0]
    images, _, h, w = preds_dicts[0]["hm"].shape
    for rec, preds, base in zip(table, preds_dicts, label_bases):
        if ("vel" in preds) != has_vel:
            raise _lib.S2DError("decode_center_maps: a velocity branch on some tasks only")
        for m, key in enumerate(_MAPS):
            if key == "vel" and not has_vel:
                continue
            t = preds[key]
            want = (images, preds["hm"].shape[1] if key == "hm" else _CHANNELS[key], h, w)
            if tuple(t.shape) != want:   # the kernels index every map of every task with the same sizes
                raise _lib.S2DError(f"decode_center_maps: map '{key}' has shape {tuple(t.shape)}, expected {want}")
            if t.dtype != torch.float32:   # bf16 maps are widened first, as the torch chain does
                t = t.float()
            nchw = t.is_contiguous()
            if not nchw and not t.is_contiguous(memory_format=torch.channels_last):
                t, nchw = t.contiguous(), True
            alive.append(t)
            c, hw = t.shape[1], t.shape[2] * t.shape[3]
            rec.map[m] = t.data_ptr()
            rec.channel_stride[m], rec.pixel_stride[m] = (hw, 1) if nchw else (1, c)
        rec.classes = preds["hm"].shape[1]
        rec.label_base = int(base)
    return table, alive


def decode_center_maps(preds_dicts, test_cfg, double_flip=False, pre_max_size=None, label_bases=None):
    """Candidates of every (task, sample) segment of a CenterHead from its raw prediction maps.

    preds_dicts: one dict per task (at most 8) of CUDA maps [images, C, H, W] (hm, reg, height, dim, rot and optionally vel; fp32 maps
    are read in place in NCHW or channels_last layout, other dtypes are widened); with double_flip the images are 4 per sample
    (original, H-mirrored, W-mirrored, both) and are mirrored back and averaged.  test_cfg supplies score_threshold,
    post_center_limit_range (empty: no range test), out_size_factor, voxel_size, pc_range.  A pixel is a candidate when its class-maximum
    score exceeds the threshold and its centre lies inside the range; each segment keeps its pre_max_size best (None: all).
    label_bases: added to the labels of each task (default 0: task-local classes).
    Runs on the current stream; ONE host read (the per-segment pass counts).  Returns `Candidates`."""
    hm0 = preds_dicts[0]["hm"]
    if not all(v.is_cuda for p in preds_dicts for v in p.values()):
        raise _lib.S2DError("decode_center_maps: CUDA tensors expected (no CPU fallback)")
    if not 1 <= len(preds_dicts) <= MAX_TASKS:
        raise _lib.S2DError(f"decode_center_maps: {len(preds_dicts)} tasks (1..{MAX_TASKS} supported)")
    lib = _lib.load()
    get = _cfg_get(test_cfg)
    dev = hm0.device
    images, _, h, w = hm0.shape
    if double_flip:
        assert images % 4 == 0, images
    samples = images // 4 if double_flip else images
    tasks = len(preds_dicts)
    segs, hw = tasks * samples, h * w
    nd = 9 if "vel" in preds_dicts[0] else 7
    table, alive = _task_table(preds_dicts, label_bases or [0] * tasks)
    rng = get("post_center_limit_range")
    rng = (ctypes.c_float * 6)(*[float(v) for v in rng]) if rng is not None and len(rng) > 0 else None
    vs, pc0 = get("voxel_size"), get("pc_range")
    geo = (float(get("out_size_factor")), float(vs[0]), float(vs[1]), float(pc0[0]), float(pc0[1]))
    st = _stream(dev)
    score = torch.empty((segs, hw), dtype=torch.float32, device=dev)
    label = torch.empty((segs, hw), dtype=torch.int32, device=dev)
    count = torch.empty((segs,), dtype=torch.int32, device=dev)
    _lib.check(lib.s2d_center_predict_score(table, tasks, samples, h, w, int(double_flip), float(get("score_threshold")), rng, *geo,
                                            score.data_ptr(), label.data_ptr(), count.data_ptr(), st), "s2d_center_predict_score")
    # descending score, ties by pixel index: the order the per-segment chain produced (mask compaction, then a stable sort)
    score_sorted, order = torch.sort(score, dim=1, descending=True, stable=True)
    passed = count.tolist()   # host read 1
    counts = [c if pre_max_size is None else min(c, int(pre_max_size)) for c in passed]
    offsets, total = [], 0
    for c in counts:
        offsets.append(total)
        total += c
    segments = torch.tensor([offsets, counts], dtype=torch.int32).reshape(2, segs).to(dev)
    boxes = torch.empty((total, nd), dtype=torch.float32, device=dev)
    scores = torch.empty((total,), dtype=torch.float32, device=dev)
    labels = torch.empty((total,), dtype=torch.int64, device=dev)
    if total:
        _lib.check(lib.s2d_center_predict_boxes(table, tasks, samples, h, w, int(double_flip), *geo, order.data_ptr(), score_sorted.data_ptr(),
                                                label.data_ptr(), segments[0].data_ptr(), segments[1].data_ptr(), max(counts), total,
                                                boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), st), "s2d_center_predict_boxes")
    del alive
    return Candidates(boxes, scores, labels, counts, offsets, segments, passed, samples, tasks)


def predict_on_device(preds_dicts, test_cfg, num_classes):
    """decode + batched NMS + per-sample assembly: a list of (boxes, scores, labels) per sample, tasks concatenated in task order and
    labels offset by the class counts of the earlier tasks - or None when a segment exceeds the NMS kernels' limit or the batched NMS
    workspace would exceed NMS_MAX_WORKSPACE_BYTES (the caller then takes the per-segment chain).  Two host reads per call: the pass counts and the kept counts."""
    from .nms import circle_nms_batched, rotate_nms_batched
    get = _cfg_get(test_cfg)
    nms_cfg = get("nms")
    nget = (lambda k: nms_cfg[k]) if isinstance(nms_cfg, dict) else (lambda k: getattr(nms_cfg, k))
    circular = bool(get("circular_nms", False))
    bases = [sum(num_classes[:t]) for t in range(len(preds_dicts))]
    # the circle NMS takes every passing pixel (center_head.py:473-476), the rotated NMS the pre_max_size best (:478-481)
    cand = decode_center_maps(preds_dicts, test_cfg, bool(get("double_flip", False)), None if circular else nget("nms_pre_max_size"), bases)
    if cand.counts and max(cand.counts) > NMS_MAX_BOXES:
        return None
    if cand.counts and _lib.load().s2d_nms_batched_workspace_bytes(sum(cand.counts), max(cand.counts)) > NMS_MAX_WORKSPACE_BYTES:
        return None
    post_max = nget("nms_post_max_size")
    if circular:
        radius = [float(get("min_radius")[t]) for t in range(cand.tasks) for _ in range(cand.samples)]
        keep, n_keep = circle_nms_batched(cand.boxes, cand.segments, cand.counts, radius, post_max)
    else:
        keep, n_keep = rotate_nms_batched(cand.boxes, cand.segments, cand.counts, nget("nms_iou_threshold"), post_max)
    # rows of the packed lists in output order: sample by sample, inside a sample task by task, inside a task in keep order
    max_keep = keep.shape[1] if keep.dim() == 2 else 0
    pos, sizes = [], []
    for b in range(cand.samples):
        n = 0
        for t in range(cand.tasks):
            s = t * cand.samples + b
            pos.extend(range(s * max_keep, s * max_keep + n_keep[s]))
            n += n_keep[s]
        sizes.append(n)
    if not sizes:
        return []
    if pos:
        rows = (keep + cand.segments[0].long()[:, None]).reshape(-1)[torch.tensor(pos, dtype=torch.int64).to(keep.device)]
        boxes, scores, labels = cand.boxes[rows], cand.scores[rows], cand.labels[rows]
    else:
        boxes, scores, labels = cand.boxes[:0], cand.scores[:0], cand.labels[:0]
    return list(zip(boxes.split(sizes), scores.split(sizes), labels.split(sizes)))


# ---- predict without the host: fixed-capacity buffers, launches only, capturable into one HIP graph --------------------------------------
TOPK_MAX = 4096   # s2d_segment_topk's limit on k


class StaticDetections:
    """Padded results of `StaticPredictPlan.run`, all on the device and owned by the plan (the next run overwrites them):
    boxes [B, cap, 7 | 9] fp32, scores [B, cap] fp32, labels [B, cap] int64 - the first counts[b] (int32 [B]) rows of sample b are its
    detections in `predict`'s order, the rows behind them are zero with label -1; overflow int32 [tasks * B]: 1 where a (task, sample)
    segment had more passing pixels than the plan's k (its result is then the NMS of its k best)."""
    __slots__ = ("boxes", "scores", "labels", "counts", "overflow")

    def __init__(self, boxes, scores, labels, counts, overflow):
        self.boxes, self.scores, self.labels, self.counts, self.overflow = boxes, scores, labels, counts, overflow

    def __iter__(self):
        return iter((self.boxes, self.scores, self.labels, self.counts, self.overflow))

    def as_list(self, metadata=None):
        """what `CenterHead.predict` returns: one dict per sample (box3d_lidar, scores, label_preds, metadata), views into the padded
        buffers.  The ONE host read of the static path: the counts."""
        counts = self.counts.tolist()
        return [dict(box3d_lidar=self.boxes[b, :n], scores=self.scores[b, :n], label_preds=self.labels[b, :n],
                     metadata=metadata[b] if metadata else None) for b, n in enumerate(counts)]


def _static_maps(preds_dicts):
    """the refusals of the static path that concern the maps, before any HIP call: it reads the maps in place, so it cannot widen or copy"""
    if not 1 <= len(preds_dicts) <= MAX_TASKS:
        raise _lib.S2DError(f"predict_static: {len(preds_dicts)} tasks (1..{MAX_TASKS} supported)")
    has_vel = "vel" in preds_dicts[0]
    for preds in preds_dicts:
        if ("vel" in preds) != has_vel:
            raise _lib.S2DError("predict_static: a velocity branch on some tasks only")
        for key in _MAPS:
            if key == "vel" and not has_vel:
                continue
            t = preds[key]
            if t.dtype != torch.float32:
                raise _lib.S2DError(f"predict_static: map '{key}' is {t.dtype}: fp32 maps only (the static path does not widen)")
            if t.dim() != 4 or not (t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)):
                raise _lib.S2DError(f"predict_static: map '{key}' is neither NCHW-contiguous nor channels_last (the static path does not copy)")
    if not all(v.is_cuda for p in preds_dicts for v in p.values()):
        raise _lib.S2DError("predict_static: CUDA tensors expected (no CPU fallback)")
    return has_vel


class StaticPredictPlan:
    """CenterHead.predict for one (test_cfg, class counts, samples, h, w, velocity branch, device) with every buffer allocated at build
    time.  `run` only launches on the current stream - score, top-K, boxes, batched NMS, gather: seven kernels - with no host read, no
    host-to-device copy, no allocation and no torch operator, so it can be captured into a HIP graph (one stream, a linear chain).
    k candidates per segment: nms_pre_max_size under the rotated NMS (the cut `predict` makes: equal results whatever passes);
    `max_candidates` under the circle NMS, where `predict` takes every passing pixel - a segment with more gets overflow = 1 and the NMS of
    its k best."""

    def __init__(self, test_cfg, num_classes, samples, h, w, has_vel, device, max_candidates=4096):
        get = _cfg_get(test_cfg)
        nms_cfg = get("nms")
        nget = (lambda k: nms_cfg[k]) if isinstance(nms_cfg, dict) else (lambda k: getattr(nms_cfg, k))
        device = torch.device(device)
        self.circular = bool(get("circular_nms", False))
        self.double_flip = bool(get("double_flip", False))
        self.tasks, self.samples, self.h, self.w = len(num_classes), int(samples), int(h), int(w)
        self.k = int(max_candidates if self.circular else nget("nms_pre_max_size"))
        if not 1 <= self.k <= TOPK_MAX:
            raise _lib.S2DError(f"StaticPredictPlan: {self.k} candidates per segment (1..{TOPK_MAX} supported)")
        if not 1 <= self.tasks <= MAX_TASKS:
            raise _lib.S2DError(f"StaticPredictPlan: {self.tasks} tasks (1..{MAX_TASKS} supported)")
        if device.type != "cuda":
            raise _lib.S2DError("StaticPredictPlan: a CUDA device expected (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.samples < 1 or self.h < 1 or self.w < 1:
            raise _lib.S2DError(f"StaticPredictPlan: empty maps (samples {samples}, h {h}, w {w})")
        if get("per_class_nms", False):
            raise NotImplementedError("StaticPredictPlan: per_class_nms produces no result in the reference either (center_head.py:417-418)")
        if self.circular and len(get("min_radius")) < self.tasks:
            raise _lib.S2DError(f"StaticPredictPlan: {len(get('min_radius'))} circle radii for {self.tasks} tasks")
        lib = _lib.load()
        from .nms import _ws
        self.device, self.has_vel = device, bool(has_vel)
        self.classes = [int(c) for c in num_classes]
        self.label_bases = [sum(self.classes[:t]) for t in range(self.tasks)]
        rng = get("post_center_limit_range")
        self.range6 = (ctypes.c_float * 6)(*[float(v) for v in rng]) if rng is not None and len(rng) > 0 else None
        vs, pc0 = get("voxel_size"), get("pc_range")
        self.geo = (float(get("out_size_factor")), float(vs[0]), float(vs[1]), float(pc0[0]), float(pc0[1]))
        self.threshold = float(get("score_threshold"))
        self.iou_threshold = float(nget("nms_iou_threshold"))
        post_max = nget("nms_post_max_size")
        self.max_keep = self.k if post_max is None else min(self.k, int(post_max))
        segs, hw, k, nd = self.tasks * self.samples, self.h * self.w, self.k, 9 if has_vel else 7
        self.segs, self.hw, self.box_dim, self.total, self.cap = segs, hw, nd, segs * k, self.tasks * self.max_keep
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
        self.score, self.label, self.passed = new((segs, hw), torch.float32), new((segs, hw), torch.int32), new((segs,), torch.int32)
        # row stride h * w, the first k columns filled: s2d_center_predict_boxes reads them as it reads a full sort
        self.order, self.score_sorted = new((segs, hw), torch.int64), new((segs, hw), torch.float32)
        self.table = new((3, segs), torch.int32)   # offsets, counts, overflow
        self.cand_boxes, self.cand_scores, self.cand_labels = new((self.total, nd), torch.float32), new((self.total,), torch.float32), new((self.total,), torch.int64)
        self.keep, self.n_keep = new((segs, self.max_keep), torch.int64), new((segs,), torch.int32)
        self.nms_ws = _ws(lib.s2d_nms_batched_workspace_bytes(self.total, k), device)
        self.radius = None
        if self.circular:
            radius = [float(get("min_radius")[t]) for t in range(self.tasks) for _ in range(self.samples)]
            self.radius = torch.tensor(radius, dtype=torch.float32).to(device)
        self.boxes, self.scores = new((self.samples, self.cap, nd), torch.float32), new((self.samples, self.cap), torch.float32)
        self.labels, self.counts = new((self.samples, self.cap), torch.int64), new((self.samples,), torch.int32)
        self.out = StaticDetections(self.boxes, self.scores, self.labels, self.counts, self.table[2])

    def buffers(self):
        """every device buffer of the plan by name (none is ever reallocated)"""
        names = ("score", "label", "passed", "order", "score_sorted", "table", "cand_boxes", "cand_scores", "cand_labels", "keep", "n_keep", "nms_ws",
                 "radius", "boxes", "scores", "labels", "counts")
        return {n: getattr(self, n) for n in names if getattr(self, n) is not None}

    def _task_table(self, preds_dicts):
        if _static_maps(preds_dicts) != self.has_vel or len(preds_dicts) != self.tasks:
            raise _lib.S2DError("StaticPredictPlan.run: the tasks or the velocity branch differ from the plan's")
        images = self.samples * (4 if self.double_flip else 1)
        table = (_lib.CenterPredictTask * self.tasks)()
        for rec, preds, classes, base in zip(table, preds_dicts, self.classes, self.label_bases):
            for m, key in enumerate(_MAPS):
                if key == "vel" and not self.has_vel:
                    continue
                t = preds[key]
                c = classes if key == "hm" else _CHANNELS[key]
                if tuple(t.shape) != (images, c, self.h, self.w) or t.device != self.device:
                    raise _lib.S2DError(f"StaticPredictPlan.run: map '{key}' has shape {tuple(t.shape)} on {t.device}, the plan was built for "
                                        f"{(images, c, self.h, self.w)} on {self.device}")
                rec.map[m] = t.data_ptr()
                rec.channel_stride[m], rec.pixel_stride[m] = (self.hw, 1) if t.is_contiguous() else (1, c)
            rec.classes, rec.label_base = classes, base
        return table

    def run(self, preds_dicts):
        """launches only, on the current stream; returns the plan's `StaticDetections` (the same tensors at every call)"""
        table = self._task_table(preds_dicts)   # host only: pointers and strides of the maps, read in place
        lib, st, flip, ptr = _lib.load(), _stream(self.device), int(self.double_flip), lambda t: t.data_ptr()
        offsets, counts, overflow = (self.table[i].data_ptr() for i in range(3))
        _lib.check(lib.s2d_center_predict_score(table, self.tasks, self.samples, self.h, self.w, flip, self.threshold, self.range6, *self.geo,
                                                ptr(self.score), ptr(self.label), ptr(self.passed), st), "s2d_center_predict_score")
        _lib.check(lib.s2d_segment_topk(ptr(self.score), self.segs, self.hw, self.hw, self.k, ptr(self.passed), ptr(self.order), ptr(self.score_sorted),
                                        self.hw, offsets, counts, overflow, st), "s2d_segment_topk")
        _lib.check(lib.s2d_center_predict_boxes(table, self.tasks, self.samples, self.h, self.w, flip, *self.geo, ptr(self.order), ptr(self.score_sorted),
                                                ptr(self.label), offsets, counts, self.k, self.total, ptr(self.cand_boxes), ptr(self.cand_scores),
                                                ptr(self.cand_labels), st), "s2d_center_predict_boxes")
        if self.circular:
            rc = lib.s2d_nms_circle_batched(ptr(self.cand_boxes), self.box_dim, offsets, counts, self.segs, self.k, self.total, ptr(self.radius),
                                            self.max_keep, ptr(self.keep), ptr(self.n_keep), ptr(self.nms_ws), self.nms_ws.numel(), st)
        else:
            rc = lib.s2d_nms_rotated_bev_batched(ptr(self.cand_boxes), self.box_dim, offsets, counts, self.segs, self.k, self.total, self.iou_threshold,
                                                 self.max_keep, ptr(self.keep), ptr(self.n_keep), ptr(self.nms_ws), self.nms_ws.numel(), st)
        _lib.check(rc, "s2d_nms_circle_batched" if self.circular else "s2d_nms_rotated_bev_batched")
        _lib.check(lib.s2d_predict_static_gather(ptr(self.cand_boxes), ptr(self.cand_scores), ptr(self.cand_labels), offsets, ptr(self.keep),
                                                 ptr(self.n_keep), self.tasks, self.samples, self.max_keep, self.box_dim, self.total, ptr(self.boxes),
                                                 ptr(self.scores), ptr(self.labels), ptr(self.counts), st), "s2d_predict_static_gather")
        return self.out


def static_plan_key(test_cfg, num_classes, images, h, w, has_vel, device, max_candidates):
    """what a StaticPredictPlan depends on, as a hashable key (CenterHead.predict_static caches plans by it)"""
    get = _cfg_get(test_cfg)
    nms_cfg = get("nms")
    nget = (lambda k: nms_cfg[k]) if isinstance(nms_cfg, dict) else (lambda k: getattr(nms_cfg, k))
    flat = lambda v: None if v is None else tuple(float(x) for x in v)
    circular = bool(get("circular_nms", False))
    return (float(get("score_threshold")), flat(get("post_center_limit_range")), float(get("out_size_factor")), flat(get("voxel_size")),
            flat(get("pc_range")), bool(get("double_flip", False)), circular, flat(get("min_radius")) if circular else None,
            nget("nms_pre_max_size"), nget("nms_post_max_size"), float(nget("nms_iou_threshold")), bool(get("per_class_nms", False)),
            tuple(num_classes), int(images), int(h), int(w), bool(has_vel), str(device), int(max_candidates))
