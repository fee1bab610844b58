"""Rotated BEV NMS / IoU on the device (csrc/nms.hip): `box_torch_ops.rotate_nms_pcdet` and `iou3d_nms_cuda.boxes_iou_bev_gpu`
(/root/reference/det3d/core/bbox/box_torch_ops.py:449-464, det3d/ops/iou3d_nms/src/iou3d_nms_api.cpp:11-16)."""
import torch

from . import _lib


def _stream(dev):
    return torch._C._cuda_getCurrentRawStream(dev.index)


def _ws(nbytes, device):
    """caller-owned scratch of one entry: a plain allocation of exactly the queried size (the seam tests/ws_guard.py replaces)"""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def boxes_iou_bev(boxes_a, boxes_b):
    """[N,7] x [M,7] (x,y,z,dx,dy,dz,heading) cuda fp32 -> IoU matrix [N,M]"""
    if not boxes_a.is_cuda:
        raise _lib.S2DError("boxes_iou_bev: CUDA tensors expected (no CPU fallback)")
    lib = _lib.load()
    a, b = boxes_a.float().contiguous(), boxes_b.float().contiguous()
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    _lib.check(lib.s2d_bev_iou_f32(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], out.data_ptr(), _stream(a.device)), "s2d_bev_iou_f32")
    return out


def rotate_nms(boxes, scores, thresh, pre_maxsize=None, post_max_size=None):
    """indices into `boxes` kept by the greedy rotated NMS, in descending-score order (rotate_nms_pcdet).  The only host read is
    the number of kept boxes (the result tensor's size - the reference API exposes it the same way)."""
    if not boxes.is_cuda:
        raise _lib.S2DError("rotate_nms: CUDA tensors expected (no CPU fallback)")
    lib = _lib.load()
    order = torch.sort(scores, dim=0, descending=True, stable=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    n = int(order.shape[0])
    if n == 0:
        return order
    b = boxes[order].float().contiguous()
    keep = torch.empty(n, dtype=torch.int64, device=b.device)
    n_keep = torch.empty(1, dtype=torch.int32, device=b.device)
    ws = _ws(lib.s2d_nms_workspace_bytes(n), b.device)
    max_keep = n if post_max_size is None else min(n, int(post_max_size))
    _lib.check(lib.s2d_nms_rotated_bev(b.data_ptr(), n, float(thresh), max_keep, keep.data_ptr(), n_keep.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream(b.device)), "s2d_nms_rotated_bev")
    return order[keep[:int(n_keep.item())]]


def circle_nms(centers_xy, scores, min_radius, post_max_size=83):
    """CenterPoint's `_circle_nms` (/root/reference/det3d/models/bbox_heads/center_head.py:499-507 over core/utils/circle_nms_jit.py:4-31):
    indices into the input kept by the greedy centre-distance suppression, in descending-score order, at most post_max_size of them.
    (The reference orders equal scores by numpy's reversed argsort; here the sort is stable descending - float scores do not tie.)"""
    if not centers_xy.is_cuda:
        raise _lib.S2DError("circle_nms: CUDA tensors expected (no CPU fallback)")
    lib = _lib.load()
    order = torch.sort(scores, dim=0, descending=True, stable=True)[1]
    n = int(order.shape[0])
    if n == 0:
        return order
    xy = centers_xy[order].float().contiguous()
    keep = torch.empty(n, dtype=torch.int64, device=xy.device)
    n_keep = torch.empty(1, dtype=torch.int32, device=xy.device)
    ws = _ws(lib.s2d_nms_workspace_bytes(n), xy.device)
    max_keep = n if post_max_size is None else min(n, int(post_max_size))
    _lib.check(lib.s2d_nms_circle(xy.data_ptr(), n, float(min_radius), max_keep, keep.data_ptr(), n_keep.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _stream(xy.device)), "s2d_nms_circle")
    return order[keep[:int(n_keep.item())]]


def _nms_batched(entry, what, rows, segments, counts, thresh, post_max_size, n_keep_on_device=False):
    if not rows.is_cuda or not segments.is_cuda:
        raise _lib.S2DError(f"{what}: CUDA tensors expected (no CPU fallback)")
    lib = _lib.load()
    segs = len(counts)
    if segments.dtype != torch.int32 or tuple(segments.shape) != (2, segs) or not segments.is_contiguous():
        raise _lib.S2DError(f"{what}: segments must be a contiguous int32 [2, {segs}] tensor (offsets, counts)")
    rows = rows.float().contiguous()
    dev = rows.device
    total, max_count = int(rows.shape[0]), max(counts, default=0)
    max_keep = max_count if post_max_size is None else min(max_count, int(post_max_size))
    keep = torch.empty((segs, max_keep), dtype=torch.int64, device=dev)
    n_keep = torch.empty((segs,), dtype=torch.int32, device=dev)
    if segs == 0:
        return keep, (n_keep if n_keep_on_device else [])
    ws = _ws(lib.s2d_nms_batched_workspace_bytes(total, max_count), dev)
    _lib.check(getattr(lib, entry)(rows.data_ptr(), rows.shape[1] if rows.dim() == 2 else 0, segments[0].data_ptr(), segments[1].data_ptr(), segs,
                                   max_count, total, thresh, max_keep, keep.data_ptr(), n_keep.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _stream(dev)), entry)
    return keep, (n_keep if n_keep_on_device else n_keep.tolist())


def rotate_nms_batched(boxes, segments, counts, thresh, post_max_size=None, n_keep_on_device=False):
    """`rotate_nms` for many independent segments in two launches (s2d_nms_rotated_bev_batched): the per-(task, sample) loop of
    /root/reference/det3d/models/bbox_heads/center_head.py:455-481 over box_torch_ops.py:449-464.
    boxes: cuda fp32 [N, 7 or more] packed rows (x, y, z, dx, dy, dz, ..., heading LAST), each segment's rows contiguous and already sorted
    by descending score (a pre_maxsize cut is made by the caller: pass the rows that take part); segments: cuda int32 [2, S] = row
    offsets and row counts; counts: the same counts on the host (a list - they size the launch, each at most 65536).
    Returns (keep, n_keep): keep cuda int64 [S, max_keep] indices into each segment's own rows in descending-score order, of which the
    first n_keep[s] (a host list: the one host read) are valid; max_keep = min(max(counts), post_max_size).  With n_keep_on_device the
    counts come back as the cuda int32 [S] tensor the kernel wrote and nothing is read on the host.  Current stream."""
    return _nms_batched("s2d_nms_rotated_bev_batched", "rotate_nms_batched", boxes, segments, counts, float(thresh), post_max_size,
                        n_keep_on_device)


def circle_nms_batched(centers_xy, segments, counts, min_radius, post_max_size=83):
    """`circle_nms` for many independent segments in two launches (s2d_nms_circle_batched; center_head.py:473-476,499-507 over
    core/utils/circle_nms_jit.py:4-31).  centers_xy: cuda fp32 [N, 2 or more] packed rows with (x, y) first - the packed box list
    itself will do; min_radius: one threshold per segment (a sequence of S floats, or a cuda fp32 [S] tensor), compared with the
    SQUARED centre distance as the reference does.  segments, counts and the result as `rotate_nms_batched`."""
    if not centers_xy.is_cuda:
        raise _lib.S2DError("circle_nms_batched: CUDA tensors expected (no CPU fallback)")
    if not torch.is_tensor(min_radius):
        min_radius = torch.tensor([float(r) for r in min_radius], dtype=torch.float32).to(centers_xy.device)
    if min_radius.numel() != len(counts):
        raise _lib.S2DError(f"circle_nms_batched: {min_radius.numel()} radii for {len(counts)} segments")
    radius = min_radius.float().contiguous()
    return _nms_batched("s2d_nms_circle_batched", "circle_nms_batched", centers_xy, segments, counts, radius.data_ptr(), post_max_size)
