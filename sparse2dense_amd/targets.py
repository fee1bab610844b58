"""Device-side CenterPoint target assignment: `AssignLabel`
(/root/reference/det3d/datasets/pipelines/preprocess.py:478-653) for the one-task Waymo head, produced on the GPU from padded
ground-truth boxes so that no per-frame numpy work is left on the host.  Output fields, dtypes and shapes are those of the
reference's `example` after `collate_kitti` (lists with one entry per task): hm f32[B,3,H,W], anno_box f32[B,500,10],
ind i64[B,500], mask u8[B,500], cat i64[B,500] (+ gt_boxes_and_cls f32[B,500,10] for the two-stage code).
`scene.assign_targets` is the CPU restatement the tests compare against.  `assign_label_tasks` is the same for a table of tasks (the
six-task nuScenes head) from boxes in their original order."""
import ctypes

import numpy as np
import torch

from . import _lib, scene


def pad_boxes(boxes_list, classes_list, device):
    """per-frame numpy boxes [K_b,9] / classes [K_b] -> padded device tensors f32[B,Kmax,9], i32[B,Kmax] (0 = padding)"""
    kmax = max([len(b) for b in boxes_list] + [1])
    boxes = np.zeros((len(boxes_list), kmax, 9), np.float32)
    classes = np.zeros((len(boxes_list), kmax), np.int32)
    for i, (b, c) in enumerate(zip(boxes_list, classes_list)):
        boxes[i, :len(b)] = b
        classes[i, :len(b)] = c
    return torch.from_numpy(boxes).to(device), torch.from_numpy(classes).to(device)


def assign_label(gt_boxes, gt_classes, pc_range=scene.WAYMO_RANGE, voxel_size=scene.WAYMO_VOXEL, out_size_factor=8, num_classes=3,
                 max_objs=500, gaussian_overlap=0.1, min_radius=2, grid_xy=(1504, 1504), with_boxes_and_cls=False):
    """gt_boxes f32[B,K,9] cuda, gt_classes i32[B,K] cuda -> dict of per-task lists (one task)."""
    if not gt_boxes.is_cuda:
        raise _lib.S2DError("assign_label: CUDA tensors expected (scene.assign_targets is the host restatement)")
    lib = _lib.load()
    gt_boxes = gt_boxes.float().contiguous()
    gt_classes = gt_classes.int().contiguous()
    b, k = gt_classes.shape
    fw, fh = grid_xy[0] // out_size_factor, grid_xy[1] // out_size_factor
    dev = gt_boxes.device
    hm = torch.zeros((b, num_classes, fh, fw), dtype=torch.float32, device=dev)
    anno = torch.empty((b, max_objs, 10), dtype=torch.float32, device=dev)
    ind = torch.empty((b, max_objs), dtype=torch.int64, device=dev)
    mask = torch.empty((b, max_objs), dtype=torch.uint8, device=dev)
    cat = torch.empty((b, max_objs), dtype=torch.int64, device=dev)
    bc = torch.empty((b, max_objs, 10), dtype=torch.float32, device=dev) if with_boxes_and_cls else None
    f2 = lambda v: (ctypes.c_float * 2)(float(np.float32(v[0])), float(np.float32(v[1])))
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.s2d_assign_label(p(gt_boxes), p(gt_classes), b, k, f2(pc_range[:2]), f2(voxel_size[:2]), int(out_size_factor), fw, fh,
                                    int(num_classes), int(max_objs), float(gaussian_overlap), int(min_radius), p(hm), p(anno), p(ind), p(mask),
                                    p(cat), p(bc), torch._C._cuda_getCurrentRawStream(dev.index)), "s2d_assign_label")
    out = dict(hm=[hm], anno_box=[anno], ind=[ind], mask=[mask], cat=[cat])
    if with_boxes_and_cls:
        out["gt_boxes_and_cls"] = bc
    return out


def assign_label_tasks(gt_boxes, gt_classes, tasks, pc_range=scene.NUSC_RANGE, voxel_size=scene.NUSC_VOXEL, out_size_factor=8,
                       grid_xy=scene.NUSC_GRID_XY, max_objs=500, gaussian_overlap=0.1, min_radius=2, with_boxes_and_cls=False):
    """AssignLabel for a table of tasks (the six-task nuScenes table: waymo_configs.NUSC_TASKS), one launch for all tasks.
    gt_boxes f32[B,K,9] cuda as (x,y,z,w,l,h,vx,vy,yaw); gt_classes i32[B,K] cuda, the GLOBAL 1-based class of every box in the frame's
    original order (<= 0: padding; above the table's last class: ignored) - the regrouping per task and class is done on the device.
    `tasks` is the config's list of task dicts (or of class counts).  Returns the reference's `example` fields after collation: lists
    with one entry per task of hm f32[B,n_t,H,W] (contiguous views of one allocation), anno_box f32[B,max_objs,10], ind i64, mask u8,
    cat i64 [B,max_objs], and with `with_boxes_and_cls` gt_boxes_and_cls f32[B,max_objs,10] in the flattened task order.  The reference
    asserts that a frame's objects fit into max_objs rows of gt_boxes_and_cls; here the list is cut at max_objs instead (no host read).
    `scene.assign_targets_tasks` is the host restatement."""
    if not gt_boxes.is_cuda:
        raise _lib.S2DError("assign_label_tasks: CUDA tensors expected (scene.assign_targets_tasks is the host restatement)")
    lib = _lib.load()
    counts = scene.task_class_counts(tasks)
    gt_boxes = gt_boxes.float().contiguous()
    gt_classes = gt_classes.int().contiguous()
    b, k = gt_classes.shape
    nt = len(counts)
    fw, fh = grid_xy[0] // out_size_factor, grid_xy[1] // out_size_factor
    dev = gt_boxes.device
    hm = torch.zeros(b * sum(counts) * fh * fw, dtype=torch.float32, device=dev)
    anno = torch.empty((nt, b, max_objs, 10), dtype=torch.float32, device=dev)
    ind = torch.empty((nt, b, max_objs), dtype=torch.int64, device=dev)
    mask = torch.empty((nt, b, max_objs), dtype=torch.uint8, device=dev)
    cat = torch.empty((nt, b, max_objs), dtype=torch.int64, device=dev)
    bc = torch.empty((b, max_objs, 10), dtype=torch.float32, device=dev) if with_boxes_and_cls else None
    f2 = lambda v: (ctypes.c_float * 2)(float(np.float32(v[0])), float(np.float32(v[1])))
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(lib.s2d_assign_label_tasks(p(gt_boxes), p(gt_classes), b, k, (ctypes.c_int32 * nt)(*counts), nt, f2(pc_range[:2]),
                                          f2(voxel_size[:2]), int(out_size_factor), fw, fh, int(max_objs), float(gaussian_overlap),
                                          int(min_radius), p(hm), p(anno), p(ind), p(mask), p(cat), p(bc),
                                          torch._C._cuda_getCurrentRawStream(dev.index)), "s2d_assign_label_tasks")
    offs = [int(o) * b * fh * fw for o in np.concatenate(([0], np.cumsum(counts)))]
    out = dict(hm=[hm[offs[t]:offs[t + 1]].view(b, counts[t], fh, fw) for t in range(nt)], anno_box=list(anno.unbind(0)),
               ind=list(ind.unbind(0)), mask=list(mask.unbind(0)), cat=list(cat.unbind(0)))
    if with_boxes_and_cls:
        out["gt_boxes_and_cls"] = bc
    return out
