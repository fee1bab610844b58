"""CenterHead.predict on the device (csrc/center_predict.hip): the decode of every task and sample of a head in two launches around one
sort, and the assembly of the per-sample results from the batched NMS (nms.rotate_nms_batched / nms.circle_nms_batched).
Replaces the per-task torch chain of /root/reference/det3d/models/bbox_heads/center_head.py:311-419 and the per-(task, sample) chain
of :452-495.  A SEGMENT is one (task, sample) pair, segment = task * samples + sample."""
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
