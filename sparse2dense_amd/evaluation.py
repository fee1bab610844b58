"""Detection AP evaluation: the reference's KITTI-protocol evaluator (det3d/datasets/kitti/eval.py, det3d/datasets/utils/eval.py over
`rotate_iou_gpu_eval` of det3d/ops/nms/nms_gpu.py:580-672), restated in numpy as the float64 definition and run on the device by
csrc/eval_ap.hip.

    get_official_eval_result / get_coco_eval_result / do_eval_v3 / do_coco_style_eval / eval_class_v3 / get_mAP / get_thresholds /
    clean_data, prepare_data, calculate_iou_partly, compute_statistics_jit, image_box_overlap, bev_box_overlap, box3d_overlap,
    box3d_overlap_kernel, rotate_iou_gpu_eval       the reference's names, signatures, dictionaries and result strings
    Evaluator                                       the tensor-native front: what `predict` returns plus the frame's boxes, kept on the device
    device_reason, eval_paths, device_stats         which route a call takes and why; how many calls took each; launches and host reads
    decisions_clear                                 no decision can flip when every overlap moves by up to a margin

Geometry.  A BEV row is (x, y, dx, dy, r) and a corner (cx, cy) of the axis-aligned rectangle maps to (cos r cx + sin r cy + x,
-sin r cx + cos r cy + y), the reference's `rbbox_to_corners`.  Rows are rounded to float32 as the reference's launcher does; the host
definition then clips the two rectangles in float64 (Sutherland-Hodgman, area by the shoelace sum) where the reference fans triangles over
fp32 intersection points, and rounds the result to float32 as the reference's output array does.  The 3-D height term is the reference's,
in double, on the fp32 intersection area, stored to fp32.

The matching.  The detection scan of `compute_statistics_jit` is one reduction per ground truth; with min_overlap >= 0 the reference's
branches select
    compute_fp=False   the highest score among candidates with overlap > min_overlap, the lowest index on equal scores (its `>`);
    compute_fp=True    the largest overlap among non-ignored candidates, the lowest index on equal overlaps; else the first ignored one
(the first non-ignored candidate is always taken, whether an ignored one was taken before or not, later ones only with a strictly larger
overlap, and an ignored one only while nothing is chosen).  The ground-truth walk stays sequential: a taken detection is gone.

Routes.  Annotations whose arrays are CUDA tensors go to the device unless compute_aos is set (a detection alpha != -10), a frame has more
than 1024 detections or more than 1024 ground-truth rows (DontCare included), a min_overlap is negative, or S2D_EVAL_DEVICE=0; everything
else, numpy annotations among it, runs the host definition.  Nothing raises for being unsupported.  On the device `eval_class_v3` is three
launches (overlaps, first-pass matching, the sweep over up to 41 score thresholds) and two host reads (the true-positive scores, the
counts) per metric, whatever the number of frames; `get_thresholds`, the running-max precision and `get_mAP` stay on the host.

Out of scope: AOS on the device, the Waymo / nuScenes metric programs and their file writers, HIP-graph capture."""
import ctypes
import io as sysio
import os

import numpy as np

try:
    import torch
except ImportError:   # the host definition needs numpy alone
    torch = None

MAX_DETS = MAX_GTS = 1024   # per frame on the device route (S2D_EVAL_MAX_ROWS)
N_SAMPLE_PTS = 41
EVAL_CLASS_LAUNCHES, EVAL_CLASS_HOST_READS = 3, 2

CLASS_NAMES = ["car", "pedestrian", "bicycle", "truck", "bus", "trailer", "construction_vehicle", "motorcycle", "barrier", "traffic_cone",
               "cyclist"]
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]
NAME_VAN, NAME_SITTING, NAME_OTHER, NAME_DONTCARE_BIT = 11, 12, 15, 256   # row name codes of the kernels, after CLASS_NAMES' indices

eval_paths = {"device": 0, "host": 0}   # eval_class_v3 calls per route
device_stats = {"launches": 0, "host_reads": 0}   # kernel launches and device-to-host reads of the device route, summed over the calls


# ---- rotated rectangles --------------------------------------------------------------------------------------------------------------
def _corners(rows):
    """[N, 4, 2] float64 corners of (x, y, dx, dy, r) rows in the order of the reference's rbbox_to_corners"""
    rows = np.asarray(rows, np.float64).reshape(-1, 5)
    c, s = np.cos(rows[:, 4]), np.sin(rows[:, 4])
    cx = np.stack([-rows[:, 2], -rows[:, 2], rows[:, 2], rows[:, 2]], 1) / 2
    cy = np.stack([-rows[:, 3], rows[:, 3], rows[:, 3], -rows[:, 3]], 1) / 2
    return np.stack([c[:, None] * cx + s[:, None] * cy + rows[:, 0:1], -s[:, None] * cx + c[:, None] * cy + rows[:, 1:2]], 2)


def _clip_area(subject, clip):
    """area of the intersection of convex quadrilaterals, pairwise: subject, clip [P, 4, 2] float64 -> [P] float64.  Sutherland-Hodgman
    against the four edges of `clip`, at most 8 vertices, then the shoelace sum."""
    p = subject.shape[0]
    poly = np.zeros((p, 8, 2))
    poly[:, :4] = subject
    cnt = np.full(p, 4, np.int64)
    centre = clip.mean(1)
    k8 = np.arange(8)[None, :]
    for e in range(4):
        a, b = clip[:, e], clip[:, (e + 1) % 4]
        ab = b - a
        sign = np.sign(ab[:, 0] * (centre[:, 1] - a[:, 1]) - ab[:, 1] * (centre[:, 0] - a[:, 0]))   # the side the rectangle lies on
        d = (ab[:, None, 0] * (poly[:, :, 1] - a[:, None, 1]) - ab[:, None, 1] * (poly[:, :, 0] - a[:, None, 0])) * sign[:, None]
        nxt = np.where(k8 + 1 < cnt[:, None], k8 + 1, 0)
        dn = np.take_along_axis(d, nxt, 1)
        pn = np.take_along_axis(poly, nxt[:, :, None], 1)
        live = k8 < cnt[:, None]
        keep = live & (d >= 0)
        cross = live & ((d >= 0) != (dn >= 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(cross, d / (d - dn), 0.0)
        inter = poly + (pn - poly) * t[:, :, None]
        out = np.stack([poly, inter], 2).reshape(p, 16, 2)          # per vertex: itself if kept, then the crossing of its edge
        emit = np.stack([keep, cross], 2).reshape(p, 16)
        order = np.argsort(~emit, 1, kind="stable")[:, :8]
        poly = np.take_along_axis(out, order[:, :, None], 1)
        cnt = emit.sum(1)
        assert cnt.max(initial=0) <= 8
        poly[k8 >= cnt[:, None]] = 0.0
    nxt = np.where(k8 + 1 < cnt[:, None], k8 + 1, 0)
    pn = np.take_along_axis(poly, nxt[:, :, None], 1)
    terms = np.where(k8 < cnt[:, None], poly[:, :, 0] * pn[:, :, 1] - pn[:, :, 0] * poly[:, :, 1], 0.0)
    return np.abs(terms.sum(1)) / 2


def rotate_overlap64(boxes, query_boxes, criterion=-1):
    """float64 [N, K]: devRotateIoUEval of the reference on the float32-rounded rows with an area-exact intersection.  criterion -1 IoU,
    0 / 1 intersection over the area of the second / first argument of the reference's kernel call (query row / box row), 2 the area."""
    boxes = np.asarray(boxes).astype(np.float32).astype(np.float64).reshape(-1, 5)
    query = np.asarray(query_boxes).astype(np.float32).astype(np.float64).reshape(-1, 5)
    n, k = boxes.shape[0], query.shape[0]
    out = np.zeros((n, k))
    if n == 0 or k == 0:
        return out
    reach_b, reach_q = np.hypot(boxes[:, 2], boxes[:, 3]) / 2, np.hypot(query[:, 2], query[:, 3]) / 2
    near = np.hypot(boxes[:, None, 0] - query[None, :, 0], boxes[:, None, 1] - query[None, :, 1]) <= reach_b[:, None] + reach_q[None, :]
    bi, qi = np.nonzero(near)
    inter = np.zeros((n, k))
    if len(bi):
        cb, cq = _corners(boxes), _corners(query)
        inter[bi, qi] = _clip_area(cq[qi], cb[bi])
    area_b, area_q = (boxes[:, 2] * boxes[:, 3])[:, None], (query[:, 2] * query[:, 3])[None, :]   # the kernel's rbox2, rbox1
    with np.errstate(divide="ignore", invalid="ignore"):
        if criterion == -1:
            return inter / (area_q + area_b - inter)
        if criterion == 0:
            return inter / np.broadcast_to(area_q, inter.shape)
        if criterion == 1:
            return inter / np.broadcast_to(area_b, inter.shape)
    return inter


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """the reference's launcher: float32 [N, K]"""
    return rotate_overlap64(boxes, query_boxes, criterion).astype(np.float32)


def image_box_overlap(boxes, query_boxes, criterion=-1):
    boxes, query_boxes = np.asarray(boxes), np.asarray(query_boxes)
    n, k = boxes.shape[0], query_boxes.shape[0]
    overlaps = np.zeros((n, k), dtype=boxes.dtype)
    if n == 0 or k == 0:
        return overlaps
    b, q = boxes[:, None, :], query_boxes[None, :, :]
    qarea = (q[..., 2] - q[..., 0]) * (q[..., 3] - q[..., 1])
    barea = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0])
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1])
    hit = (iw > 0) & (ih > 0)
    if criterion == -1:
        ua = barea + qarea - iw * ih
    elif criterion == 0:
        ua = np.broadcast_to(barea, hit.shape)
    elif criterion == 1:
        ua = np.broadcast_to(qarea, hit.shape)
    else:
        ua = np.ones(hit.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        overlaps[hit] = (iw * ih / ua)[hit]
    return overlaps


def bev_box_overlap(boxes, qboxes, criterion=-1, stable=False):
    return rotate_iou_gpu_eval(boxes, qboxes, criterion)


def box3d_overlap_kernel(boxes, qboxes, rinc, criterion=-1, z_axis=1, z_center=1.0):
    """in place on rinc [N, K] (the BEV intersection areas), as the reference: the height overlap from z_axis / z_center in double"""
    boxes, qboxes = np.asarray(boxes), np.asarray(qboxes)
    if rinc.size == 0:
        return
    bz, bh = boxes[:, z_axis].astype(np.float64)[:, None], boxes[:, z_axis + 3].astype(np.float64)[:, None]
    qz, qh = qboxes[:, z_axis].astype(np.float64)[None, :], qboxes[:, z_axis + 3].astype(np.float64)[None, :]
    min_z = np.minimum(bz + bh * (1 - z_center), qz + qh * (1 - z_center))
    max_z = np.maximum(bz - bh * z_center, qz - qh * z_center)
    iw = min_z - max_z
    area1 = (boxes[:, 3] * boxes[:, 4] * boxes[:, 5]).astype(np.float64)[:, None]
    area2 = (qboxes[:, 3] * qboxes[:, 4] * qboxes[:, 5]).astype(np.float64)[None, :]
    inc = iw * rinc.astype(np.float64)
    if criterion == -1:
        ua = area1 + area2 - inc
    elif criterion == 0:
        ua = np.broadcast_to(area1, inc.shape)
    elif criterion == 1:
        ua = np.broadcast_to(area2, inc.shape)
    else:
        ua = np.ones(inc.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = np.where(iw > 0, inc / ua, 0.0)
    pos = rinc > 0
    rinc[pos] = val[pos].astype(rinc.dtype)


def box3d_overlap(boxes, qboxes, criterion=-1, z_axis=1, z_center=1.0):
    bev_axes = list(range(7))
    bev_axes.pop(z_axis + 3)
    bev_axes.pop(z_axis)
    boxes, qboxes = np.asarray(boxes), np.asarray(qboxes)
    rinc = rotate_iou_gpu_eval(boxes[:, bev_axes], qboxes[:, bev_axes], 2)
    box3d_overlap_kernel(boxes, qboxes, rinc, criterion, z_axis, z_center)
    return rinc


# ---- annotations ---------------------------------------------------------------------------------------------------------------------
def _host(v):
    if torch is not None and torch.is_tensor(v):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def _host_anno(anno):
    out = {k: _host(v) for k, v in anno.items() if k != "name_code"}
    if "name" not in out:
        out["name"] = names_of_codes(_host(anno["name_code"]))
    return out


def name_codes(names):
    """int32 row codes of the kernels: the index in CLASS_NAMES of the lower-cased name, NAME_VAN, NAME_SITTING or NAME_OTHER, plus
    NAME_DONTCARE_BIT for the exact names "DontCare" and "ignore" (the reference compares those without lower-casing)"""
    out = np.empty(len(names), np.int32)
    for i, n in enumerate(names):
        low = str(n).lower()
        code = CLASS_NAMES.index(low) if low in CLASS_NAMES else NAME_VAN if low == "van" else NAME_SITTING if low == "person_sitting" \
            else NAME_OTHER
        out[i] = code | (NAME_DONTCARE_BIT if str(n) in ("DontCare", "ignore") else 0)
    return out


def names_of_codes(codes):
    table = CLASS_NAMES + ["Van", "Person_sitting", "other", "other", "other"]
    return np.array(["DontCare" if c & NAME_DONTCARE_BIT else table[c & 15] for c in np.asarray(codes).tolist()], dtype=object)


def clean_data(gt_anno, dt_anno, current_class, difficulty):
    dc_bboxes, ignored_gt, ignored_dt = [], [], []
    current_cls_name = CLASS_NAMES[current_class].lower()
    num_gt = len(gt_anno["name"])
    num_dt = len(dt_anno["name"])
    num_valid_gt = 0
    for i in range(num_gt):
        bbox = gt_anno["bbox"][i]
        gt_name = gt_anno["name"][i].lower()
        height = bbox[3] - bbox[1]
        valid_class = -1
        if gt_name == current_cls_name:
            valid_class = 1
        elif current_cls_name == "Pedestrian".lower() and "Person_sitting".lower() == gt_name:
            valid_class = 0
        elif current_cls_name == "Car".lower() and "Van".lower() == gt_name:
            valid_class = 0
        else:
            valid_class = -1
        ignore = False
        if (gt_anno["occluded"][i] > MAX_OCCLUSION[difficulty]) or (gt_anno["truncated"][i] > MAX_TRUNCATION[difficulty]) or (
                height <= MIN_HEIGHT[difficulty]):
            ignore = True
        if valid_class == 1 and not ignore:
            ignored_gt.append(0)
            num_valid_gt += 1
        elif valid_class == 0 or (ignore and (valid_class == 1)):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
        if (gt_anno["name"][i] == "DontCare") or (gt_anno["name"][i] == "ignore"):
            dc_bboxes.append(gt_anno["bbox"][i])
    for i in range(num_dt):
        if dt_anno["name"][i].lower() == current_cls_name:
            valid_class = 1
        else:
            valid_class = -1
        height = abs(dt_anno["bbox"][i, 3] - dt_anno["bbox"][i, 1])
        if height < MIN_HEIGHT[difficulty]:
            ignored_dt.append(1)
        elif valid_class == 1:
            ignored_dt.append(0)
        else:
            ignored_dt.append(-1)
    return num_valid_gt, ignored_gt, ignored_dt, dc_bboxes


def prepare_data(gt_annos, dt_annos, current_class, difficulty=None, clean_data=clean_data):
    gt_datas_list, dt_datas_list, total_dc_num = [], [], []
    ignored_gts, ignored_dets, dontcares = [], [], []
    total_num_valid_gt = 0
    for i in range(len(gt_annos)):
        num_valid_gt, ignored_gt, ignored_det, dc_bboxes = clean_data(gt_annos[i], dt_annos[i], current_class, difficulty)
        ignored_gts.append(np.array(ignored_gt, dtype=np.int64))
        ignored_dets.append(np.array(ignored_det, dtype=np.int64))
        if len(dc_bboxes) == 0:
            dc_bboxes = np.zeros((0, 4)).astype(np.float64)
        else:
            dc_bboxes = np.stack(dc_bboxes, 0).astype(np.float64)
        total_dc_num.append(dc_bboxes.shape[0])
        dontcares.append(dc_bboxes)
        total_num_valid_gt += num_valid_gt
        gt_datas_list.append(np.concatenate([gt_annos[i]["bbox"], gt_annos[i]["alpha"][..., np.newaxis]], 1))
        dt_datas_list.append(np.concatenate([dt_annos[i]["bbox"], dt_annos[i]["alpha"][..., np.newaxis],
                                             dt_annos[i]["score"][..., np.newaxis]], 1))
    total_dc_num = np.stack(total_dc_num, axis=0) if total_dc_num else np.zeros(0, np.int64)
    return gt_datas_list, dt_datas_list, ignored_gts, ignored_dets, dontcares, total_dc_num, total_num_valid_gt


def _frame_boxes(anno, metric, z_axis):
    """the rows `calculate_iou_partly` hands to the overlap of `metric`"""
    if metric == 0:
        return anno["bbox"]
    rows = np.concatenate([anno["location"], anno["dimensions"], anno["rotation_y"][..., np.newaxis]], axis=1)
    if metric == 1:
        bev_axes = list(range(3))
        bev_axes.pop(z_axis)
        return rows[:, bev_axes + [3 + a for a in bev_axes] + [6]]
    return rows


def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50, z_axis=1, z_center=1.0):
    """per frame overlaps [len(gt_annos[i]), len(dt_annos[i])] (`eval_class_v3` passes the detections first).  Every frame is its own
    part: the reference's split into `num_parts` changes no result."""
    assert len(gt_annos) == len(dt_annos)
    if metric not in (0, 1, 2):
        raise ValueError("unknown metric")
    total_dt_num = np.array([len(a["name"]) for a in dt_annos], np.int64)
    total_gt_num = np.array([len(a["name"]) for a in gt_annos], np.int64)
    overlaps = []
    for g, d in zip(gt_annos, dt_annos):
        gt_boxes, dt_boxes = _frame_boxes(g, metric, z_axis), _frame_boxes(d, metric, z_axis)
        if metric == 0:
            overlaps.append(image_box_overlap(gt_boxes, dt_boxes))
        elif metric == 1:
            overlaps.append(bev_box_overlap(gt_boxes, dt_boxes).astype(np.float64))
        else:
            overlaps.append(box3d_overlap(gt_boxes, dt_boxes, z_axis=z_axis, z_center=z_center).astype(np.float64))
    return overlaps, overlaps, total_gt_num, total_dt_num


NO_DETECTION = -10000000


def compute_statistics_jit(overlaps, gt_datas, dt_datas, ignored_gt, ignored_det, dc_bboxes, metric, min_overlap, thresh=0,
                           compute_fp=False, compute_aos=False):
    """the reference's function with the detection scan as one reduction per ground truth (see the module text)"""
    det_size, gt_size = dt_datas.shape[0], gt_datas.shape[0]
    dt_scores, dt_alphas, gt_alphas, dt_bboxes = dt_datas[:, -1], dt_datas[:, 4], gt_datas[:, 4], dt_datas[:, :4]
    ignored_det, ignored_gt = np.asarray(ignored_det), np.asarray(ignored_gt)
    assigned_detection = np.zeros(det_size, np.bool_)
    ignored_threshold = dt_scores < thresh if compute_fp else np.zeros(det_size, np.bool_)
    open_static = (ignored_det != -1) & ~ignored_threshold
    tp, fp, fn, similarity = 0, 0, 0, 0
    thresholds, delta = [], []
    for i in range(gt_size):
        if ignored_gt[i] == -1:
            continue
        cand = open_static & ~assigned_detection & (overlaps[:, i] > min_overlap)
        det_idx = -1
        if not compute_fp:
            cand &= dt_scores > NO_DETECTION
            if cand.any():
                det_idx = int(np.argmax(np.where(cand, dt_scores, -np.inf)))
        else:
            real = cand & (ignored_det == 0)
            if min_overlap < 0:   # the first real candidate is taken whatever its overlap once an ignored one was; a later one needs > 0
                det_idx = _scan_fp(overlaps[:, i], cand, ignored_det)
            elif real.any():
                det_idx = int(np.argmax(np.where(real, overlaps[:, i], -np.inf)))
            elif cand.any():
                det_idx = int(np.argmax(cand))
        if det_idx < 0:
            if ignored_gt[i] == 0:
                fn += 1
        elif ignored_gt[i] == 1 or ignored_det[det_idx] == 1:
            assigned_detection[det_idx] = True
        else:
            tp += 1
            thresholds.append(dt_scores[det_idx])
            if compute_aos:
                delta.append(gt_alphas[i] - dt_alphas[det_idx])
            assigned_detection[det_idx] = True
    if compute_fp:
        rest = ~(assigned_detection | (ignored_det == -1) | (ignored_det == 1) | ignored_threshold)
        fp = int(rest.sum())
        nstuff = 0
        if metric == 0 and len(dc_bboxes):
            overlaps_dt_dc = image_box_overlap(dt_bboxes, np.asarray(dc_bboxes), 0)
            nstuff = int((rest & (overlaps_dt_dc > min_overlap).any(1)).sum())
        fp -= nstuff
        if compute_aos:
            tmp = np.zeros((fp + len(delta),))
            for i in range(len(delta)):
                tmp[i + fp] = (1.0 + np.cos(delta[i])) / 2.0
            similarity = np.sum(tmp) if tp > 0 or fp > 0 else -1
    return tp, fp, fn, similarity, np.array(thresholds, np.float64)


def _scan_fp(column, cand, ignored_det):
    """the reference's compute_fp=True scan, literally (only reached with a negative min_overlap)"""
    det_idx, max_overlap, assigned_ignored_det, chosen = -1, 0, False, False
    for j in np.nonzero(cand)[0]:
        if (column[j] > max_overlap or assigned_ignored_det) and ignored_det[j] == 0:
            max_overlap, det_idx, chosen, assigned_ignored_det = column[j], int(j), True, False
        elif not chosen and ignored_det[j] == 1:
            det_idx, chosen, assigned_ignored_det = int(j), True, True
    return det_idx


def get_thresholds(scores, num_gt, num_sample_pts=41):
    scores.sort()
    scores = scores[::-1]
    current_recall = 0
    thresholds = []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        if i < (len(scores) - 1):
            r_recall = (i + 2) / num_gt
        else:
            r_recall = l_recall
        if ((r_recall - current_recall) < (current_recall - l_recall)) and (i < (len(scores) - 1)):
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


# ---- routing -------------------------------------------------------------------------------------------------------------------------
def _is_cuda(anno):
    return torch is not None and torch.is_tensor(anno.get("bbox")) and anno["bbox"].is_cuda


def _rows(anno):
    return int(anno["bbox"].shape[0])


def compute_aos_of(dt_annos):
    """the reference's test: the first detection of the first frame that has one carries an alpha other than -10"""
    for anno in dt_annos:
        if anno["alpha"].shape[0] != 0:
            return bool(_host(anno["alpha"][:1])[0] != -10)
    return False


def device_reason(gt_annos, dt_annos, compute_aos=False, min_overlaps=None):
    """None when `eval_class_v3` takes the device for these annotations, else why it runs the host definition"""
    if os.environ.get("S2D_EVAL_DEVICE") == "0":
        return "S2D_EVAL_DEVICE=0"
    if not len(gt_annos) or not all(_is_cuda(a) for a in gt_annos) or not all(_is_cuda(a) for a in dt_annos):
        return "annotations on the host"
    if compute_aos:
        return "compute_aos: orientation similarity is computed on the host"
    nd, ng = max(_rows(a) for a in dt_annos), max(_rows(a) for a in gt_annos)
    if nd > MAX_DETS:
        return f"a frame with {nd} detections: at most {MAX_DETS} on the device"
    if ng > MAX_GTS:
        return f"a frame with {ng} ground-truth rows: at most {MAX_GTS} on the device"
    if min_overlaps is not None and np.min(min_overlaps) < 0:
        return "a negative min_overlap"
    return None


# ---- the device route ----------------------------------------------------------------------------------------------------------------
def _codes_of(anno, dev):
    if "name_code" in anno:
        return anno["name_code"].to(dev, torch.int32)
    return torch.from_numpy(name_codes(anno["name"])).to(dev)


class _Packed:
    """every frame's rows concatenated on the device, with the frames' row offsets; built once per result call"""

    def __init__(self, gt_annos, dt_annos):
        dev = dt_annos[0]["bbox"].device
        f64 = lambda v: v.to(dev, torch.float64)
        cat = lambda parts, width: torch.cat([p.reshape(-1, width) for p in parts], 0).contiguous()
        box = lambda a: torch.cat([f64(a["location"]).reshape(-1, 3), f64(a["dimensions"]).reshape(-1, 3), f64(a["rotation_y"]).reshape(-1, 1)], 1)
        self.device, self.frames = dev, len(gt_annos)
        self.det_box, self.gt_box = cat([box(a) for a in dt_annos], 7), cat([box(a) for a in gt_annos], 7)
        self.det_img, self.gt_img = cat([f64(a["bbox"]) for a in dt_annos], 4), cat([f64(a["bbox"]) for a in gt_annos], 4)
        self.det_score = cat([f64(a["score"]) for a in dt_annos], 1).reshape(-1)
        self.gt_occ = cat([torch.stack([f64(a["occluded"]).reshape(-1), f64(a["truncated"]).reshape(-1)], 1) for a in gt_annos], 2)
        self.det_name = torch.cat([_codes_of(a, dev) for a in dt_annos]).contiguous()
        self.gt_name = torch.cat([_codes_of(a, dev) for a in gt_annos]).contiguous()
        nd, ng = np.array([_rows(a) for a in dt_annos], np.int64), np.array([_rows(a) for a in gt_annos], np.int64)
        self.nd, self.ng = nd, ng
        self.det_off_h, self.gt_off_h = np.concatenate([[0], np.cumsum(nd)]), np.concatenate([[0], np.cumsum(ng)])
        self.ov_off_h = np.concatenate([[0], np.cumsum(nd * ng)])
        self.det_off = torch.from_numpy(self.det_off_h.astype(np.int32)).to(dev)
        self.gt_off = torch.from_numpy(self.gt_off_h.astype(np.int32)).to(dev)
        self.ov_off = torch.from_numpy(self.ov_off_h.astype(np.int64)).to(dev)
        self.launches = self.host_reads = 0


def _stream(dev):
    return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def device_overlaps(packed, metric, z_axis=1, z_center=1.0):
    """the ragged fp32 overlaps of every frame in one launch: frame f holds [ng_f, nd_f] (ground truth major) at ov_off[f]"""
    from . import _lib
    pairs = int(packed.ov_off_h[-1])
    out = torch.empty(pairs, dtype=torch.float32, device=packed.device)
    _lib.check(_lib.load().s2d_eval_overlaps(metric, _ptr(packed.det_box), _ptr(packed.det_img), _ptr(packed.gt_box), _ptr(packed.gt_img),
                                             packed.det_off.data_ptr(), packed.gt_off.data_ptr(), packed.ov_off.data_ptr(), packed.frames,
                                             pairs, z_axis, float(z_center), _ptr(out), _stream(packed.device)), "s2d_eval_overlaps")
    packed.launches += 1
    device_stats["launches"] += 1
    return out


def frame_overlaps(packed, flat):
    """the per frame [nd, ng] float32 matrices of `device_overlaps` on the host (for tests and analysis)"""
    flat = flat.cpu().numpy()
    return [flat[packed.ov_off_h[f]:packed.ov_off_h[f + 1]].reshape(int(packed.ng[f]), int(packed.nd[f])).T for f in range(packed.frames)]


def device_counts(packed, overlaps, current_classes, difficultys, metric, min_overlaps):
    """the two matching passes.  min_overlaps [K, 3, M].  Returns (thresholds [M, L, K, 41] with their counts [M, L, K], pr int64
    [M, L, K, 41, 3] = tp, fp, fn summed over the frames)."""
    from . import _lib
    lib, dev, frames = _lib.load(), packed.device, packed.frames
    m, l, k = len(current_classes), len(difficultys), min_overlaps.shape[0]
    combos, total_gt = m * l * k, int(packed.gt_off_h[-1])
    classes, diffs = (ctypes.c_int32 * m)(*[int(c) for c in current_classes]), (ctypes.c_int32 * l)(*[int(d) for d in difficultys])
    mins = torch.from_numpy(np.ascontiguousarray(min_overlaps[:, metric, :].T, dtype=np.float64)).to(dev)   # [M, K]
    # one buffer, one read: the true-positive scores [combos, total_gt] double, then (true positives, valid ground truths) int32 per
    # (frame, combo)
    score_bytes = combos * total_gt * 8
    first = torch.empty(score_bytes + frames * combos * 8, dtype=torch.uint8, device=dev)
    tp_scores, counts = first[:score_bytes].view(torch.float64), first[score_bytes:].view(torch.int32)
    pr = torch.empty(combos * N_SAMPLE_PTS * 3, dtype=torch.int64, device=dev)   # zeroed by the first pass
    rows = (_ptr(overlaps), _ptr(packed.det_img), _ptr(packed.det_score), _ptr(packed.det_name), _ptr(packed.gt_img), _ptr(packed.gt_occ),
            _ptr(packed.gt_name), packed.det_off.data_ptr(), packed.gt_off.data_ptr(), packed.ov_off.data_ptr(), frames)
    table = (classes, m, diffs, l, mins.data_ptr(), k)
    _lib.check(lib.s2d_eval_match(*rows, *table, total_gt, _ptr(tp_scores), counts.data_ptr(), pr.data_ptr(), _stream(dev)), "s2d_eval_match")
    packed.launches += 1
    device_stats["launches"] += 1
    first_h = first.cpu().numpy()
    packed.host_reads += 1
    device_stats["host_reads"] += 1
    tp_scores_h = first_h[:score_bytes].view(np.float64).reshape(combos, total_gt)
    counts_h = first_h[score_bytes:].view(np.int32).reshape(frames, combos, 2)
    thresholds = np.zeros((combos, N_SAMPLE_PTS))
    num_thresholds = np.zeros(combos, np.int32)
    slot = packed.gt_off_h[:-1, None] + np.arange(int(packed.ng.max(initial=0)))[None, :]   # [frames, max ng]
    for c in range(combos):
        taken = np.arange(slot.shape[1])[None, :] < counts_h[:, c, 0:1]
        scores = tp_scores_h[c, slot[taken]]   # frame order, then ground-truth order: the order of the reference's list
        picked = get_thresholds(scores, int(counts_h[:, c, 1].sum()))
        num_thresholds[c] = len(picked)
        thresholds[c, :len(picked)] = picked
    thr_d = torch.from_numpy(thresholds).to(dev)
    nthr_d = torch.from_numpy(num_thresholds).to(dev)
    _lib.check(lib.s2d_eval_pr(*rows, metric, *table, thr_d.data_ptr(), nthr_d.data_ptr(), pr.data_ptr(), _stream(dev)), "s2d_eval_pr")
    packed.launches += 1
    device_stats["launches"] += 1
    pr_h = pr.cpu().numpy().reshape(m, l, k, N_SAMPLE_PTS, 3)
    packed.host_reads += 1
    device_stats["host_reads"] += 1
    return thresholds.reshape(m, l, k, N_SAMPLE_PTS), num_thresholds.reshape(m, l, k), pr_h


def _eval_class_device(packed, current_classes, difficultys, metric, min_overlaps, z_axis, z_center):
    overlaps = device_overlaps(packed, metric, z_axis, z_center)
    thresholds, counts, pr = device_counts(packed, overlaps, current_classes, difficultys, metric, min_overlaps)
    precision = np.zeros(thresholds.shape)
    for idx in np.ndindex(counts.shape):
        n = counts[idx]
        with np.errstate(divide="ignore", invalid="ignore"):
            precision[idx][:n] = pr[idx][:n, 0] / (pr[idx][:n, 0] + pr[idx][:n, 1]).astype(np.float64)
        for i in range(n):
            precision[idx][i] = np.max(precision[idx][i:], axis=-1)
    return {"recall": np.zeros(thresholds.shape), "precision": precision, "orientation": np.zeros(thresholds.shape), "thresholds": thresholds,
            "min_overlaps": min_overlaps, "counts": pr}


# ---- the reference's drivers ---------------------------------------------------------------------------------------------------------
def eval_class_v3(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, z_axis=1, z_center=1.0,
                  num_parts=50, _packed=None):
    """Kitti eval of one metric (0 bbox, 1 bev, 2 3d).  min_overlaps [num_minoverlap, metric, num_class].  Returns the reference's
    dictionary of recall (zeros, as in the reference), precision, orientation, thresholds [num_class, num_difficulty, num_minoverlap, 41]
    and min_overlaps, plus "counts": the integer tp / fp / fn behind every precision, [..., 41, 3]."""
    assert len(gt_annos) == len(dt_annos)
    min_overlaps = np.asarray(min_overlaps)
    if device_reason(gt_annos, dt_annos, compute_aos, min_overlaps) is None:
        eval_paths["device"] += 1
        packed = _packed if _packed is not None else _Packed(gt_annos, dt_annos)
        return _eval_class_device(packed, current_classes, difficultys, metric, min_overlaps, z_axis, z_center)
    eval_paths["host"] += 1
    gt_annos, dt_annos = [_host_anno(a) for a in gt_annos], [_host_anno(a) for a in dt_annos]
    overlaps, _, total_dt_num, total_gt_num = calculate_iou_partly(dt_annos, gt_annos, metric, num_parts, z_axis=z_axis, z_center=z_center)
    num_minoverlap, num_class, num_difficulty = len(min_overlaps), len(current_classes), len(difficultys)
    shape = [num_class, num_difficulty, num_minoverlap, N_SAMPLE_PTS]
    precision, recall, aos, all_thresholds = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape)
    counts = np.zeros(shape + [3], np.int64)
    for m, current_class in enumerate(current_classes):
        for l, difficulty in enumerate(difficultys):
            gt_datas_list, dt_datas_list, ignored_gts, ignored_dets, dontcares, total_dc_num, total_num_valid_gt = prepare_data(
                gt_annos, dt_annos, current_class, difficulty=difficulty, clean_data=clean_data)
            for k, min_overlap in enumerate(min_overlaps[:, metric, m]):
                thresholdss = []
                for i in range(len(gt_annos)):
                    rets = compute_statistics_jit(overlaps[i], gt_datas_list[i], dt_datas_list[i], ignored_gts[i], ignored_dets[i], dontcares[i],
                                                  metric, min_overlap=min_overlap, thresh=0.0, compute_fp=False)
                    thresholdss += rets[4].tolist()
                thresholds = np.array(get_thresholds(np.array(thresholdss), total_num_valid_gt))
                all_thresholds[m, l, k, :len(thresholds)] = thresholds
                pr = np.zeros([len(thresholds), 4])
                for i in range(len(gt_annos)):
                    for t, thresh in enumerate(thresholds):
                        tp, fp, fn, similarity, _ = compute_statistics_jit(
                            overlaps[i], gt_datas_list[i], dt_datas_list[i], ignored_gts[i], ignored_dets[i], dontcares[i], metric,
                            min_overlap=min_overlap, thresh=thresh, compute_fp=True, compute_aos=compute_aos)
                        pr[t, 0] += tp
                        pr[t, 1] += fp
                        pr[t, 2] += fn
                        if similarity != -1:
                            pr[t, 3] += similarity
                counts[m, l, k, :len(thresholds)] = pr[:, :3]
                with np.errstate(divide="ignore", invalid="ignore"):
                    for i in range(len(thresholds)):
                        precision[m, l, k, i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
                        if compute_aos:
                            aos[m, l, k, i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
                for i in range(len(thresholds)):
                    precision[m, l, k, i] = np.max(precision[m, l, k, i:], axis=-1)
                    if compute_aos:
                        aos[m, l, k, i] = np.max(aos[m, l, k, i:], axis=-1)
    return {"recall": recall, "precision": precision, "orientation": aos, "thresholds": all_thresholds, "min_overlaps": min_overlaps,
            "counts": counts}


def get_mAP(prec):
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def _shared_pack(gt_annos, dt_annos, compute_aos, min_overlaps):
    return _Packed(gt_annos, dt_annos) if device_reason(gt_annos, dt_annos, compute_aos, min_overlaps) is None else None


def do_eval_v3(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, difficultys=(0, 1, 2), z_axis=1, z_center=1.0):
    # min_overlaps: [num_minoverlap, metric, num_class]
    types = ["bbox", "bev", "3d"]
    packed = _shared_pack(gt_annos, dt_annos, compute_aos, min_overlaps)
    metrics = {}
    for i in range(3):
        metrics[types[i]] = eval_class_v3(gt_annos, dt_annos, current_classes, difficultys, i, min_overlaps, compute_aos, z_axis=z_axis,
                                          z_center=z_center, _packed=packed)
    return metrics


def do_coco_style_eval(gt_annos, dt_annos, current_classes, overlap_ranges, compute_aos, z_axis=1, z_center=1.0):
    # overlap_ranges: [range, metric, num_class]
    min_overlaps = np.zeros([10, *overlap_ranges.shape[1:]])
    for i in range(overlap_ranges.shape[1]):
        for j in range(overlap_ranges.shape[2]):
            start, stop, num = overlap_ranges[:, i, j]
            min_overlaps[:, i, j] = np.linspace(start, stop, int(num))
    packed = _shared_pack(gt_annos, dt_annos, compute_aos, min_overlaps)
    maps, mAP_aos = [], None
    for metric in range(3):   # the reference's do_eval_v2: orientation only with the bbox metric
        ret = eval_class_v3(gt_annos, dt_annos, current_classes, (0, 1, 2), metric, min_overlaps, compute_aos if metric == 0 else False,
                            z_axis=z_axis, z_center=z_center, _packed=packed)
        maps.append(get_mAP(ret["precision"]).mean(-1))
        if metric == 0 and compute_aos:
            mAP_aos = get_mAP(ret["orientation"]).mean(-1)
    return maps[0], maps[1], maps[2], mAP_aos


def print_str(value, *arg, sstream=None):
    if sstream is None:
        sstream = sysio.StringIO()
    sstream.truncate(0)
    sstream.seek(0)
    print(value, *arg, file=sstream)
    return sstream.getvalue()


CLASS_TO_NAME = dict(enumerate(CLASS_NAMES))
CLASS_TO_RANGE = {0: [0.5, 0.95, 10], 1: [0.25, 0.7, 10], 2: [0.25, 0.7, 10], 3: [0.5, 0.95, 10], 4: [0.5, 0.95, 10], 5: [0.5, 0.95, 10],
                  6: [0.5, 0.95, 10], 7: [0.25, 0.7, 10], 8: [0.25, 0.7, 10], 9: [0.25, 0.7, 10], 10: [0.25, 0.7, 10]}
OVERLAP_MOD = np.array([[0.7, 0.5, 0.5, 0.7, 0.7, 0.7, 0.7, 0.5, 0.5, 0.5, 0.5]] * 3)
OVERLAP_EASY = np.array([[0.7, 0.5, 0.5, 0.7, 0.7, 0.7, 0.7, 0.5, 0.25, 0.25, 0.5],
                         [0.5, 0.25, 0.25, 0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, 0.25],
                         [0.5, 0.25, 0.25, 0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25, 0.25]])


def _class_ints(current_classes):
    name_to_class = {v: n for n, v in CLASS_TO_NAME.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    return [name_to_class[c.lower()] if isinstance(c, str) else c for c in current_classes]


def official_min_overlaps(current_classes):
    """[2, 3, num_class]: the reference's moderate and easy overlap tables for these classes"""
    return np.stack([OVERLAP_MOD, OVERLAP_EASY], axis=0)[:, :, _class_ints(current_classes)]


def coco_min_overlaps(current_classes):
    """[10, 3, num_class]: the ten overlaps of the reference's class_to_range per class"""
    classes = _class_ints(current_classes)
    out = np.zeros([10, 3, len(classes)])
    for j, c in enumerate(classes):
        out[:, :, j] = np.linspace(CLASS_TO_RANGE[c][0], CLASS_TO_RANGE[c][1], int(CLASS_TO_RANGE[c][2]))[:, None]
    return out


def get_official_eval_result(gt_annos, dt_annos, current_classes, difficultys=[0, 1, 2], z_axis=1, z_center=1.0):
    """gt_annos and dt_annos must contain the keys name, bbox, location, dimensions, rotation_y, alpha, occluded, truncated (score)"""
    current_classes = _class_ints(current_classes)
    min_overlaps = official_min_overlaps(current_classes)
    result = ""
    compute_aos = compute_aos_of(dt_annos)
    metrics = do_eval_v3(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos, difficultys, z_axis=z_axis, z_center=z_center)
    detail = {}
    for j, curcls in enumerate(current_classes):
        class_name = CLASS_TO_NAME[curcls]
        detail[class_name] = {}
        for i in range(min_overlaps.shape[0]):
            mAPbbox = get_mAP(metrics["bbox"]["precision"][j, :, i])
            mAPbev = get_mAP(metrics["bev"]["precision"][j, :, i])
            mAP3d = get_mAP(metrics["3d"]["precision"][j, :, i])
            detail[class_name][f"bbox@{min_overlaps[i, 0, j]:.2f}"] = mAPbbox.tolist()
            detail[class_name][f"bev@{min_overlaps[i, 1, j]:.2f}"] = mAPbev.tolist()
            detail[class_name][f"3d@{min_overlaps[i, 2, j]:.2f}"] = mAP3d.tolist()
            result += print_str((f"{CLASS_TO_NAME[curcls]} " "AP(Average Precision)@{:.2f}, {:.2f}, {:.2f}:".format(*min_overlaps[i, :, j])))
            mAPbbox = ", ".join(f"{v:.2f}" for v in mAPbbox)
            mAPbev = ", ".join(f"{v:.2f}" for v in mAPbev)
            mAP3d = ", ".join(f"{v:.2f}" for v in mAP3d)
            result += print_str(f"bbox AP:{mAPbbox}")
            result += print_str(f"bev  AP:{mAPbev}")
            result += print_str(f"3d   AP:{mAP3d}")
            if compute_aos:
                mAPaos = get_mAP(metrics["bbox"]["orientation"][j, :, i])
                detail[class_name]["aos"] = mAPaos.tolist()
                mAPaos = ", ".join(f"{v:.2f}" for v in mAPaos)
                result += print_str(f"aos  AP:{mAPaos}")
    return {"result": result, "detail": detail}


def get_coco_eval_result(gt_annos, dt_annos, current_classes, z_axis=1, z_center=1.0):
    current_classes = _class_ints(current_classes)
    overlap_ranges = np.zeros([3, 3, len(current_classes)])
    for i, curcls in enumerate(current_classes):
        overlap_ranges[:, :, i] = np.array(CLASS_TO_RANGE[curcls])[:, np.newaxis]
    result = ""
    compute_aos = compute_aos_of(dt_annos)
    mAPbbox, mAPbev, mAP3d, mAPaos = do_coco_style_eval(gt_annos, dt_annos, current_classes, overlap_ranges, compute_aos, z_axis=z_axis,
                                                        z_center=z_center)
    detail = {}
    for j, curcls in enumerate(current_classes):
        class_name = CLASS_TO_NAME[curcls]
        detail[class_name] = {}
        o_range = np.array(CLASS_TO_RANGE[curcls])[[0, 2, 1]]
        o_range[1] = (o_range[2] - o_range[0]) / (o_range[1] - 1)
        result += print_str((f"{CLASS_TO_NAME[curcls]} " "coco AP@{:.2f}:{:.2f}:{:.2f}:".format(*o_range)))
        result += print_str((f"bbox AP:{mAPbbox[j, 0]:.2f}, " f"{mAPbbox[j, 1]:.2f}, " f"{mAPbbox[j, 2]:.2f}"))
        result += print_str((f"bev  AP:{mAPbev[j, 0]:.2f}, " f"{mAPbev[j, 1]:.2f}, " f"{mAPbev[j, 2]:.2f}"))
        result += print_str((f"3d   AP:{mAP3d[j, 0]:.2f}, " f"{mAP3d[j, 1]:.2f}, " f"{mAP3d[j, 2]:.2f}"))
        detail[class_name]["bbox"] = mAPbbox[j].tolist()
        detail[class_name]["bev"] = mAPbev[j].tolist()
        detail[class_name]["3d"] = mAP3d[j].tolist()
        if compute_aos:
            detail[class_name]["aos"] = mAPaos[j].tolist()
            result += print_str((f"aos  AP:{mAPaos[j, 0]:.2f}, " f"{mAPaos[j, 1]:.2f}, " f"{mAPaos[j, 2]:.2f}"))
    return {"result": result, "detail": detail}


# ---- margins -------------------------------------------------------------------------------------------------------------------------
def overlaps64(gt_anno, dt_anno, metric, z_axis=1, z_center=1.0):
    """[nd, ng] float64 overlaps of one frame without the fp32 roundings of the result (the rows are still rounded to float32 for the
    BEV intersection, as everywhere): what the device's and the reference's values are measured against"""
    g, d = _host_anno(gt_anno), _host_anno(dt_anno)
    gb, db = _frame_boxes(g, metric, z_axis), _frame_boxes(d, metric, z_axis)
    if metric == 0:
        return image_box_overlap(db.astype(np.float64), gb.astype(np.float64))
    if metric == 1:
        return rotate_overlap64(db, gb, -1)
    bev_axes = list(range(7))
    bev_axes.pop(z_axis + 3)
    bev_axes.pop(z_axis)
    rinc = rotate_overlap64(db[:, bev_axes], gb[:, bev_axes], 2)
    box3d_overlap_kernel(db, gb, rinc, -1, z_axis, z_center)
    return rinc


def unclear_detections(gt_anno, dt_anno, min_overlaps, z_axis=1, z_center=1.0, margin=1e-3):
    """bool [nd]: detections of one frame behind a decision that an overlap error of up to `margin` could flip, for any metric: an overlap
    within `margin` of a value of min_overlaps[:, metric, :], or two candidates of one ground truth (overlap above the smallest
    min_overlap less margin) closer than `margin` that are not identical rows (identical rows give identical overlaps on any route)"""
    d = _host_anno(dt_anno)
    nd = len(d["bbox"])
    bad = np.zeros(nd, np.bool_)
    if nd == 0 or len(_host(gt_anno["bbox"])) == 0:
        return bad
    rows = np.concatenate([d["bbox"], d["location"], d["dimensions"], d["rotation_y"][:, None]], 1).astype(np.float64)
    same = (rows[:, None, :] == rows[None, :, :]).all(2)
    for metric in range(3):
        ov = overlaps64(gt_anno, dt_anno, metric, z_axis, z_center)
        levels = np.unique(np.asarray(min_overlaps)[:, metric, :])
        bad |= (np.abs(ov[:, :, None] - levels[None, None, :]) < margin).any((1, 2))
        cand = ov > levels.min() - margin
        for i in np.nonzero(cand.sum(0) >= 2)[0]:
            js = np.nonzero(cand[:, i])[0]
            close = (np.abs(ov[js, i][:, None] - ov[js, i][None, :]) < margin) & ~same[np.ix_(js, js)]
            bad[js[close.any(1)]] = True
    return bad


def decisions_clear(gt_annos, dt_annos, min_overlaps, z_axis=1, z_center=1.0, margin=1e-3):
    """True when counts and precisions of these annotations are the same for any overlap values within `margin` of the exact ones"""
    return not any(unclear_detections(g, d, min_overlaps, z_axis, z_center, margin).any() for g, d in zip(gt_annos, dt_annos))


# ---- the tensor-native front ---------------------------------------------------------------------------------------------------------
class Evaluator:
    """Collects frames on the device and scores them.  class_names: the detector's label order (label_preds indexes it; a name outside
    the reference's class table is scored as no class).  add(pred_dicts, gt_boxes, gt_names) takes what `predict` returns per sample
    (box3d_lidar [N, >= 7], scores [N], label_preds [N]) and, per sample, the ground-truth boxes [G, >= 7] (a tensor on the same device)
    with their names (a list of strings) or label indices (a tensor).  It copies nothing to the host.  Columns 0-2 are the location, 3-5
    the dimensions, 6 the rotation; the fields a lidar-frame user of the reference fills in are filled in here: image box (0, 0, 50, 50)
    (height 50: no row is ignored by height), occlusion 0, truncation 0, alpha -10, so one difficulty says everything.
    official() / coco(): the reference's result dictionaries."""

    def __init__(self, class_names, z_axis=2, z_center=0.5):
        self.class_names, self.z_axis, self.z_center = [str(n) for n in class_names], int(z_axis), float(z_center)
        self._codes = name_codes(self.class_names)
        self._code_table = {}
        self.gt_annos, self.dt_annos = [], []

    def _anno(self, boxes, codes, scores=None):
        n, dev = boxes.shape[0], boxes.device
        bbox = torch.tensor([0.0, 0.0, 50.0, 50.0], dtype=torch.float64, device=dev).expand(n, 4)
        zero = torch.zeros(n, dtype=torch.float64, device=dev)
        anno = dict(name_code=codes, bbox=bbox, location=boxes[:, 0:3], dimensions=boxes[:, 3:6], rotation_y=boxes[:, 6], occluded=zero,
                    truncated=zero, alpha=np.full(n, -10.0))
        if scores is not None:
            anno["score"] = scores
        return anno

    def _label_codes(self, labels):
        dev = labels.device
        if dev not in self._code_table:
            self._code_table[dev] = torch.from_numpy(self._codes).to(dev)
        return self._code_table[dev][labels.long()]

    def add(self, pred_dicts, gt_boxes, gt_names):
        if isinstance(pred_dicts, dict):
            pred_dicts, gt_boxes, gt_names = [pred_dicts], [gt_boxes], [gt_names]
        if not len(pred_dicts) == len(gt_boxes) == len(gt_names):
            raise ValueError("one ground-truth box tensor and one name list per predicted sample expected")
        for pred, boxes, names in zip(pred_dicts, gt_boxes, gt_names):
            det = pred["box3d_lidar"]
            boxes = torch.as_tensor(boxes, device=det.device)
            if torch.is_tensor(names):
                codes = self._label_codes(names.to(det.device))
            else:
                codes = torch.from_numpy(name_codes(list(names))).to(det.device)
            self.dt_annos.append(self._anno(det, self._label_codes(pred["label_preds"]), pred["scores"]))
            self.gt_annos.append(self._anno(boxes, codes))

    def reset(self):
        self.gt_annos, self.dt_annos = [], []

    def _scored(self):
        return [n.lower() for n in self.class_names if n.lower() in CLASS_NAMES]

    def official(self, difficultys=(0,)):
        return get_official_eval_result(self.gt_annos, self.dt_annos, self._scored(), list(difficultys), z_axis=self.z_axis,
                                        z_center=self.z_center)

    def coco(self):
        return get_coco_eval_result(self.gt_annos, self.dt_annos, self._scored(), z_axis=self.z_axis, z_center=self.z_center)
