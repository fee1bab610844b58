"""Frame preparation of the S2D data step: the reference's `Preprocess.__call__` in training mode
(det3d/datasets/pipelines/preprocess.py:59-272) over csrc/prep.hip.

    points_in_rbbox / points_count_rbbox    box_np_ops.py:15-20,641-647 (strictly inside all six faces)
    compose_clouds                          preprocess.py:81-117: the dense cloud the teacher sees and the reconstruction (object-only) cloud
    global_noise, shuffle_points            core/sampler/preprocess.py:790-813,859-908,1032-1056 and preprocess.py:257-260
    S2DPreprocess                           the pipeline step on the reference's dictionary layout

CUDA tensors take the HIP kernels; numpy arrays and CPU tensors take the numpy restatement below, which is also the definition the tests
compare the kernels with (fp32, the same operations in the same order).  The random draws are the reference's host draws from `np.random`
in the reference's order on both paths, so a seeded run prepares the reference's frame.

Launches per frame on the device: composition 5 (stage boxes, count, scan, segments, fill) with ONE host read (the two cloud sizes and the
number of boxes that are no SIGN, three int32 in one copy), global noise 1, shuffle 1 per shuffled cloud.

    box_collision_test, bev_corners         core/sampler/preprocess.py:922-1005 (`is True / is False` by value: containment collides), box_np_ops.py:265-285
    GTSampler, build_gt_sampler             core/sampler/sample_ops.py:134-359 + preprocess.py:137-168: draws on the host, the collision walk of all
                                            groups in one workgroup, the sampled blocks pasted in front of the three clouds

GT-database sampler on the device: 4 launches (select, count, segments, paste) and ONE more host read (accept[S] and the two row counts);
the old clouds follow the pasted blocks by plain device copies.  Limits: frame boxes + candidates <= 512, candidates <= 128, 16 groups.

Out of scope: group sampling, per-object rotation noise and random_crop of the sampler, `min_points_in_gt`, the evaluation-mode composition
(preprocess.py:215-254), `npoints` subsampling, nuScenes sweep combination, several frames per launch chain.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_BOXES = 512            # S2D_PREP_MAX_BOXES: boxes of a frame staged in LDS
KIND_OTHER, KIND_VEHICLE, KIND_SIGN = 0, 1, 2
COMPOSE_LAUNCHES, NOISE_LAUNCHES, SHUFFLE_LAUNCHES_PER_CLOUD, COMPOSE_HOST_READS = 5, 1, 1, 1
_CHUNK = 16384             # points per slab of the numpy inside test (bounds its temporaries)


def kinds_of(names):
    """gt_names -> int8 kinds (1 VEHICLE, 2 SIGN, 0 everything else)"""
    return np.array([KIND_VEHICLE if n == "VEHICLE" else KIND_SIGN if n == "SIGN" else KIND_OTHER for n in names], np.int8)


# ---- numpy restatement -------------------------------------------------------------------------------------------------------------
def _f32(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _boxes2d(boxes):
    boxes = _f32(boxes)
    if boxes.ndim != 2 or (boxes.shape[0] and boxes.shape[1] < 7):
        raise _lib.S2DError(f"boxes {boxes.shape}: [M, >= 7] expected (centre, size, ..., yaw last)")
    if boxes.shape[0] > MAX_BOXES:
        raise _lib.S2DError(f"{boxes.shape[0]} boxes: at most {MAX_BOXES} per frame")
    return boxes


def _check_points(points, what="points"):
    if points.ndim != 2 or not 3 <= points.shape[1] <= 16:
        raise _lib.S2DError(f"{what} {tuple(points.shape)}: [N, 3..16] expected (x, y, z first)")


def _staged(boxes):
    """centre, half extents, cos r, sin r of every box (fp32; the angles in double, as numpy evaluates them)"""
    r = boxes[:, -1].astype(np.float64)
    return boxes[:, :3], boxes[:, 3:6] * np.float32(0.5), np.cos(r).astype(np.float32), np.sin(r).astype(np.float32)


def _inside_np(points, boxes):
    n, m = points.shape[0], boxes.shape[0]
    out = np.zeros((n, m), np.bool_)
    if n == 0 or m == 0:
        return out
    c, h, cs, sn = _staged(boxes)
    for lo in range(0, n, _CHUNK):
        p = points[lo:lo + _CHUNK]
        dx, dy, dz = p[:, None, 0] - c[None, :, 0], p[:, None, 1] - c[None, :, 1], p[:, None, 2] - c[None, :, 2]
        lx, ly = dx * cs - dy * sn, dx * sn + dy * cs
        out[lo:lo + _CHUNK] = (np.abs(lx) < h[None, :, 0]) & (np.abs(ly) < h[None, :, 1]) & (np.abs(dz) < h[None, :, 2])
    return out


def face_distance(points, boxes):
    """float64 signed distance [N, M] of every point to every box's surface in the inside test's own terms: max over the three axes of
    |local coordinate| - half extent, negative inside.  A membership can only depend on rounding where this is within a few fp32 ulps of
    0; the tests leave out the pairs with |distance| < 1e-3 m."""
    p, b = np.asarray(points, np.float64), np.asarray(boxes, np.float64)
    d = p[:, None, :3] - b[None, :, :3]
    c, s = np.cos(b[:, -1]), np.sin(b[:, -1])
    lx, ly = d[..., 0] * c - d[..., 1] * s, d[..., 0] * s + d[..., 1] * c
    return np.maximum(np.maximum(np.abs(lx) - b[:, 3] / 2, np.abs(ly) - b[:, 4] / 2), np.abs(d[..., 2]) - b[:, 5] / 2)


def _object_block_np(g, kind, box):
    """a stored cloud in the object's frame -> its block in the sweep's frame (preprocess.py:90-104)"""
    g = g.copy()
    if kind == KIND_VEHICLE:
        pos, neg = g[:, 1] > 0, g[:, 1] < 0
        g = g[pos] if pos.sum() > neg.sum() else g[neg]
        mirror = g.copy()
        mirror[:, 1] = -mirror[:, 1]
        g = np.concatenate([g, mirror], 0)
    a = np.pi / 2 + np.float64(box[-1])
    c, s = np.float32(np.cos(a)), np.float32(np.sin(a))
    x, y = g[:, 0].copy(), g[:, 1].copy()
    g[:, 0] = (x * c + y * s) + box[0]
    g[:, 1] = (x * -s + y * c) + box[1]
    g[:, 2] = g[:, 2] + box[2]
    return g


def _offsets_host(obj_offsets, m, p):
    off = obj_offsets.cpu().numpy() if torch.is_tensor(obj_offsets) else np.asarray(obj_offsets)
    off = off.astype(np.int64).reshape(-1)
    if off.shape[0] != m + 1 or (m + 1 and (off[0] != 0 or off[-1] != p or np.any(np.diff(off) < 0))):
        raise _lib.S2DError(f"obj_offsets: {m + 1} non-decreasing entries from 0 to {p} expected")
    return off.astype(np.int32)


def compose_clouds_np(points, boxes, kinds, obj_points, obj_offsets):
    points, boxes, obj_points = _f32(points), _boxes2d(boxes), _f32(obj_points).reshape(-1, np.shape(points)[1])
    _check_points(points)
    kinds = np.asarray(kinds.cpu() if torch.is_tensor(kinds) else kinds).astype(np.int8).reshape(-1)
    m = boxes.shape[0]
    if kinds.shape[0] != m:
        raise _lib.S2DError(f"kinds: {kinds.shape[0]} entries for {m} boxes")
    off = _offsets_host(obj_offsets, m, obj_points.shape[0])
    inside = _inside_np(points, boxes)
    blocks, recon = [points[~inside.any(1)]], []
    for j in range(m):
        if off[j + 1] > off[j] and kinds[j] != KIND_SIGN:
            g = _object_block_np(obj_points[off[j]:off[j + 1]], kinds[j], boxes[j])
        else:
            g = points[inside[:, j]]
        blocks.append(g)
        if kinds[j] != KIND_SIGN:
            recon.append(g)
    dense = np.concatenate(blocks, 0)
    if not recon:
        return dense, np.zeros((1, points.shape[1]), np.float32)
    recon = np.concatenate(recon, 0)
    return dense, recon[_inside_np(recon, boxes).any(1)]


def _noise_np(cloud, d):
    x, y, z = cloud[:, 0].copy(), cloud[:, 1].copy(), cloud[:, 2].copy()
    if d["flip_x"]:
        y = -y
    if d["flip_y"]:
        x = -x
    c, s, k = np.float32(d["cos"]), np.float32(d["sin"]), np.float32(d["scale"])
    xr, yr = (x * c + y * s) * k, (x * -s + y * c) * k
    z = z * k
    if d["translate"] is not None:
        t = d["translate"]
        xr, yr, z = (xr.astype(np.float64) + t[0]).astype(np.float32), (yr.astype(np.float64) + t[1]).astype(np.float32), \
            (z.astype(np.float64) + t[2]).astype(np.float32)
    cloud[:, 0], cloud[:, 1], cloud[:, 2] = xr, yr, z


# ---- device path -------------------------------------------------------------------------------------------------------------------
def _on_device(*xs):
    return any(torch.is_tensor(x) and x.is_cuda for x in xs)


def _dev_f32(x, dev):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    x = x.to(dev)
    return x if x.dtype == torch.float32 and x.is_contiguous() else x.float().contiguous()


def _stream(dev):
    return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())


def _ws(nbytes, device):
    """caller-owned scratch of one entry: a plain allocation of exactly the queried size (the seam tests/ws_guard.py replaces)"""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def _workspace(lib, n, m, p, dev):
    size = lib.s2d_prep_workspace_bytes(n, m, p)
    if size == 0:
        raise _lib.S2DError(f"prep: {n} points, {m} boxes, {p} stored rows is outside the supported sizes")
    return _ws(size, dev)


def _inside_device(points, boxes, want_mask, want_counts):
    lib = _lib.load()
    dev = points.device if torch.is_tensor(points) and points.is_cuda else boxes.device
    if torch.is_tensor(boxes) and boxes.dim() == 2 and boxes.shape[0] > MAX_BOXES:
        raise _lib.S2DError(f"{boxes.shape[0]} boxes: at most {MAX_BOXES} per frame")
    boxes = _dev_f32(boxes if torch.is_tensor(boxes) else _boxes2d(boxes), dev)
    points = _dev_f32(points, dev)
    _check_points(points)
    if boxes.dim() != 2 or (boxes.shape[0] and boxes.shape[1] < 7):
        raise _lib.S2DError(f"boxes {tuple(boxes.shape)}: [M, >= 7] expected (centre, size, ..., yaw last)")
    n, m = points.shape[0], boxes.shape[0]
    mask = torch.zeros((n, m), dtype=torch.bool, device=dev) if want_mask else None
    counts = torch.zeros((m,), dtype=torch.int32, device=dev) if want_counts else None
    if m and (n or want_counts):   # (an empty mask has nothing to write, and no address)
        ws = _workspace(lib, n, m, 0, dev)
        _lib.check(lib.s2d_prep_points_in_rbbox(points.data_ptr(), n, points.shape[1], boxes.data_ptr(), m, boxes.shape[1],
                                                mask.data_ptr() if want_mask else None, counts.data_ptr() if want_counts else None,
                                                ws.data_ptr(), ws.numel(), _stream(dev)), "s2d_prep_points_in_rbbox")
    return mask, counts


def points_in_rbbox(points, boxes):
    """bool [N, M]: point i strictly inside box j (box_np_ops.points_in_rbbox).  numpy in, numpy out; tensor in, tensor out."""
    if _on_device(points, boxes):
        return _inside_device(points, boxes, True, False)[0]
    out = _inside_np(_f32(points), _boxes2d(boxes))
    return torch.from_numpy(out) if torch.is_tensor(points) else out


def points_count_rbbox(points, boxes):
    """int32 [M]: points strictly inside each box (box_np_ops.points_count_rbbox)"""
    if _on_device(points, boxes):
        return _inside_device(points, boxes, False, True)[1]
    out = _inside_np(_f32(points), _boxes2d(boxes)).sum(0).astype(np.int32)
    return torch.from_numpy(out) if torch.is_tensor(points) else out


def compose_clouds(points, boxes, kinds, obj_points, obj_offsets):
    """(dense_points, reconstruction_points) of one training frame with distillation (preprocess.py:81-117).

    kinds int8 [M] (0 other, 1 VEHICLE, 2 SIGN); obj_points [P, C] with obj_offsets int32 [M + 1]: the stored completed clouds in the
    objects' own frames, packed in box order - an empty range means "no file for this object" and the frame's own points inside the box are
    used, as they are for every SIGN.  dense = the points outside every box in input order, then each box's block in box order (a point
    inside two boxes appears in both blocks).  reconstruction = the blocks of the boxes that are no SIGN, without the rows that lie in no box
    of the frame; one row of zeros when the frame has no such box, as the reference makes it.
    Device path: five launches and one host read (the sizes, which the caller needs to allocate and to draw the shuffles)."""
    if not _on_device(points):
        d, r = compose_clouds_np(points, boxes, kinds, obj_points, obj_offsets)
        return (torch.from_numpy(d), torch.from_numpy(r)) if torch.is_tensor(points) else (d, r)
    lib, dev = _lib.load(), points.device
    points = _dev_f32(points, dev)
    _check_points(points)
    if not torch.is_tensor(boxes):
        boxes = _boxes2d(boxes)
    boxes = _dev_f32(boxes, dev)
    n, c, m = points.shape[0], points.shape[1], boxes.shape[0]
    if boxes.dim() != 2 or (m and boxes.shape[1] < 7):
        raise _lib.S2DError(f"boxes {tuple(boxes.shape)}: [M, >= 7] expected (centre, size, ..., yaw last)")
    if m > MAX_BOXES:
        raise _lib.S2DError(f"{m} boxes: at most {MAX_BOXES} per frame")
    obj_points = _dev_f32(obj_points, dev).reshape(-1, c)
    p = obj_points.shape[0]
    if torch.is_tensor(kinds) and kinds.is_cuda:
        kinds = kinds.to(torch.int8).contiguous()
    else:
        kinds = torch.from_numpy(np.asarray(kinds.cpu() if torch.is_tensor(kinds) else kinds).astype(np.int8).reshape(-1)).to(dev)
    if kinds.numel() != m:
        raise _lib.S2DError(f"kinds: {kinds.numel()} entries for {m} boxes")
    if torch.is_tensor(obj_offsets) and obj_offsets.is_cuda:   # (clamped to 0 .. P by the kernels)
        if obj_offsets.numel() != m + 1:
            raise _lib.S2DError(f"obj_offsets: {m + 1} entries expected")
        offsets = obj_offsets.to(torch.int32).contiguous()
    else:
        offsets = torch.from_numpy(_offsets_host(obj_offsets, m, p)).to(dev)
    ws = _workspace(lib, n, m, p, dev)
    totals = torch.empty(3, dtype=torch.int32, device=dev)
    st = _stream(dev)
    _lib.check(lib.s2d_prep_compose_count(points.data_ptr(), n, c, boxes.data_ptr(), m, boxes.shape[1] if m else 7, kinds.data_ptr(),
                                          obj_points.data_ptr(), p, offsets.data_ptr(), ws.data_ptr(), ws.numel(), totals.data_ptr(), st),
               "s2d_prep_compose_count")
    n_dense, n_recon, not_sign = totals.tolist()   # the frame's one host read
    dense = torch.empty((n_dense, c), dtype=torch.float32, device=dev)
    recon = torch.empty((n_recon, c), dtype=torch.float32, device=dev)
    _lib.check(lib.s2d_prep_compose_fill(points.data_ptr(), n, c, m, obj_points.data_ptr(), p, ws.data_ptr(), ws.numel(), dense.data_ptr(), n_dense,
                                         recon.data_ptr(), n_recon, st), "s2d_prep_compose_fill")
    if not_sign == 0:
        recon = torch.zeros((1, c), dtype=torch.float32, device=dev)
    return dense, recon


# ---- global noise ------------------------------------------------------------------------------------------------------------------
def _get(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


def draw_global_noise(cfg):
    """the reference's host draws in its order: two `choice` calls (flips), a `uniform` (rotation), a `uniform` (scale), and three `normal`
    calls only when a translate std is non-zero (the third one with std[0], as core/sampler/preprocess.py:1043-1049 has it)"""
    flip_x = bool(np.random.choice([False, True], replace=False, p=[0.5, 0.5]))
    flip_y = bool(np.random.choice([False, True], replace=False, p=[0.5, 0.5]))
    rotation = _get(cfg, "global_rot_noise")
    if not isinstance(rotation, (list, tuple)):
        rotation = [-rotation, rotation]
    rot = np.random.uniform(rotation[0], rotation[1])
    lo, hi = _get(cfg, "global_scale_noise")
    scale = np.random.uniform(lo, hi)
    std = _get(cfg, "global_translate_std", 0)
    if not isinstance(std, (list, tuple, np.ndarray)):
        std = np.array([std, std, std])
    translate = None
    if not all(e == 0 for e in std):
        translate = np.array([np.random.normal(0, std[0], 1), np.random.normal(0, std[1], 1), np.random.normal(0, std[0], 1)]).T
    return dict(flip_x=flip_x, flip_y=flip_y, rot=rot, cos=np.float32(np.cos(rot)), sin=np.float32(np.sin(rot)), scale=scale,
                translate=None if translate is None else translate.reshape(3))


def _rot_z(b, rot):
    """rotation_points_single_angle's matrix (axis 2) in float64, as an array or a tensor like b"""
    c, s = np.cos(rot), np.sin(rot)
    m = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    return torch.tensor(m, dtype=torch.float64, device=b.device) if torch.is_tensor(b) else np.array(m, dtype=np.float64)


def apply_noise_to_boxes(b, d):
    """the M box rows, as the reference writes them: yaw -r + pi, -r + 2 pi, + noise; velocity columns of 9-column boxes flipped and
    rotated; every column except the last scaled.  In place (numpy array or tensor)."""
    if b.shape[0] == 0:
        return b
    if d["flip_x"]:
        b[:, 1] = -b[:, 1]
        b[:, -1] = -b[:, -1] + np.pi
        if b.shape[1] > 7:
            b[:, 7] = -b[:, 7]
    if d["flip_y"]:
        b[:, 0] = -b[:, 0]
        b[:, -1] = -b[:, -1] + 2 * np.pi
        if b.shape[1] > 7:
            b[:, 6] = -b[:, 6]
    rot = _rot_z(b, d["rot"])
    as_f64 = (lambda v: v.double()) if torch.is_tensor(b) else (lambda v: v.astype(np.float64))
    b[:, :3] = b[:, :3] @ (rot.to(b.dtype) if torch.is_tensor(b) else rot.astype(b.dtype))   # the matrix in the boxes' dtype
    if b.shape[1] > 7:   # (the reference pads the velocities with float64 zeros: this product is in float64)
        b[:, 6:8] = as_f64(b[:, 6:8]) @ rot[:2, :2]
    b[:, -1] += d["rot"]
    b[:, :-1] *= d["scale"]
    if d["translate"] is not None:
        t = d["translate"]
        b[:, :3] += torch.as_tensor(t, device=b.device).to(b.dtype) if torch.is_tensor(b) else t[None]
    return b


def apply_noise_to_clouds(clouds, d):
    """flip, rotation, scale and translation on columns 0-2 of up to three clouds in place: one launch for the device clouds"""
    dev_clouds = [c for c in clouds if torch.is_tensor(c) and c.is_cuda]
    for c in clouds:
        if torch.is_tensor(c) and c.is_cuda:
            if c.dtype != torch.float32 or not c.is_contiguous() or c.dim() != 2 or not 3 <= c.shape[1] <= 16:
                raise _lib.S2DError("global_noise: contiguous fp32 [N, 3..16] device clouds expected (they are changed in place)")
        else:
            a = c.numpy() if torch.is_tensor(c) else c
            if a.dtype != np.float32:
                raise _lib.S2DError("global_noise: fp32 clouds expected (they are changed in place)")
            _noise_np(a, d)
    if not dev_clouds:
        return
    if len({c.shape[1] for c in dev_clouds}) != 1 or len(dev_clouds) > 3:
        raise _lib.S2DError("global_noise: up to three clouds with one column count")
    args = []
    for k in range(3):
        c = dev_clouds[k] if k < len(dev_clouds) else None
        args += [c.data_ptr() if c is not None and c.shape[0] else None, c.shape[0] if c is not None else 0]
    t = d["translate"]
    dev = dev_clouds[0].device
    _lib.check(_lib.load().s2d_prep_global_noise(*args, dev_clouds[0].shape[1], int(d["flip_x"]), int(d["flip_y"]), float(d["cos"]), float(d["sin"]),
                                                 float(np.float32(d["scale"])), int(t is not None), *([0.0] * 3 if t is None else [float(v) for v in t]),
                                                 _stream(dev)), "s2d_prep_global_noise")


def global_noise(gt_boxes, points, *rest):
    """global_noise(gt_boxes, points, dense_points, reconstruction_points, cfg) -> the four, or global_noise(gt_boxes, points, cfg) -> the
    two (distillation=False).  Draws from `np.random` (draw_global_noise), changes the boxes and columns 0-2 of the clouds IN PLACE with the
    same draws.  cfg keys: global_rot_noise, global_scale_noise, global_translate_std."""
    if len(rest) not in (1, 3):
        raise TypeError("global_noise(gt_boxes, points[, dense_points, reconstruction_points], cfg)")
    clouds, cfg = (points,) + tuple(rest[:-1]), rest[-1]
    d = draw_global_noise(cfg)
    apply_noise_to_boxes(gt_boxes, d)
    apply_noise_to_clouds(clouds, d)
    return (gt_boxes,) + clouds


def shuffle_points(points, dense_points=None):
    """`np.random.shuffle` of the sweep and, when given, of the dense cloud (preprocess.py:257-260; the reconstruction cloud is not
    shuffled): `np.random.permutation(n)` consumes the same draws and names the same order; device clouds are gathered by one launch each.
    Returns new clouds."""
    out = []
    for cloud in (points,) if dense_points is None else (points, dense_points):
        perm = np.random.permutation(cloud.shape[0])
        if torch.is_tensor(cloud) and cloud.is_cuda:
            src = _dev_f32(cloud, cloud.device)
            dst = torch.empty_like(src)
            idx = torch.from_numpy(perm.astype(np.int64)).to(cloud.device)
            _lib.check(_lib.load().s2d_prep_gather_rows(src.data_ptr(), src.shape[0], src.shape[1], idx.data_ptr(), dst.data_ptr(),
                                                        _stream(cloud.device)), "s2d_prep_gather_rows")
            out.append(dst)
        else:
            out.append(cloud[torch.from_numpy(perm)] if torch.is_tensor(cloud) else cloud[perm])
    return out[0] if dense_points is None else tuple(out)


# ---- the pipeline step -------------------------------------------------------------------------------------------------------------
def _select(gt_dict, inds):
    for k, v in gt_dict.items():
        gt_dict[k] = v[inds]


class S2DPreprocess:
    """`Preprocess` of the reference's training pipeline as a callable (res, info) -> (res, info) on its dictionary layout.

    Reads res["lidar"]["combined"] or ["points"], res["lidar"]["annotations"] (boxes, names), info["gt_boxes" / "gt_names" / "gt_signs"]
    and the cfg keys mode, shuffle_points, distillation, global_rot_noise, global_scale_noise, global_translate_std, class_names,
    no_augmentation.  `object_store` is a callable name -> [P_j, C] array (or tensor) or None and replaces the reference's pickle paths;
    `db_sampler` is a built GTSampler (cfg.db_sampler alone raises: the database is not read from the config's path here).
    Writes res["lidar"]["points" / "dense_points" / "reconstruction_points"] and the filtered annotations with gt_classes.  A sweep that
    arrives as a CUDA tensor is prepared by the kernels and stays on the device; a numpy sweep takes the numpy restatement."""

    def __init__(self, cfg=None, object_store=None, db_sampler=None, **kwargs):
        self.mode = _get(cfg, "mode")
        self.shuffle_points = _get(cfg, "shuffle_points", False)
        self.distillation = _get(cfg, "distillation", False)
        self.no_augmentation = _get(cfg, "no_augmentation", False)
        self.cfg = cfg
        if _get(cfg, "db_sampler") is not None and db_sampler is None:
            raise NotImplementedError("S2DPreprocess: cfg.db_sampler is set: pass the built sampler as the db_sampler argument "
                                      "(prep.build_gt_sampler(cfg.db_sampler, db_infos, points_of))")
        self.db_sampler = db_sampler
        if (_get(cfg, "min_points_in_gt", -1) or -1) > 0:
            raise NotImplementedError("S2DPreprocess: min_points_in_gt is out of scope")
        if self.mode == "train":
            self.class_names = list(_get(cfg, "class_names"))
        elif self.distillation:
            raise NotImplementedError("S2DPreprocess: the evaluation-mode composition is out of scope")
        self.object_store = object_store if object_store is not None else (lambda name: None)

    def _stored(self, info, kinds, ncols, dev):
        """the stored clouds of the frame packed in box order + their offsets"""
        parts, off = [], [0]
        for name, kind in zip(info["gt_signs"], kinds):
            g = self.object_store(name) if kind != KIND_SIGN else None
            rows = 0 if g is None else int(g.shape[0])
            if rows:
                parts.append(g)
            off.append(off[-1] + rows)
        off = np.asarray(off, np.int32)
        if not parts:
            return np.zeros((0, ncols), np.float32), off
        if dev is not None and any(torch.is_tensor(g) for g in parts):
            return torch.cat([_dev_f32(g, dev) for g in parts], 0), off
        return np.concatenate([_f32(g) for g in parts], 0), off

    def __call__(self, res, info):
        res["mode"] = self.mode
        lidar = res["lidar"]
        points = lidar["combined"] if "combined" in lidar else lidar["points"]
        dev = points.device if torch.is_tensor(points) and points.is_cuda else None
        dense = recon = None
        if self.mode == "train":
            anno = lidar["annotations"]
            gt_dict = {"gt_boxes": anno["boxes"], "gt_names": np.array(anno["names"]).reshape(-1)}
            if self.distillation:
                kinds = kinds_of(info["gt_names"])
                stored, off = self._stored(info, kinds, points.shape[1], dev)
                dense, recon = compose_clouds(points, info["gt_boxes"], kinds, stored, off)
            if not self.no_augmentation:
                keep = np.array([i for i, n in enumerate(gt_dict["gt_names"]) if n not in ("DontCare", "ignore", "UNKNOWN")], np.int64)
                _select(gt_dict, keep)
            mask = np.array([n in self.class_names for n in gt_dict["gt_names"]], np.bool_)
            if self.db_sampler is not None and not self.no_augmentation:
                # preprocess.py:137-168: the sampled blocks go in front of the three clouds, names and boxes behind the frame's
                if dev is not None:
                    points = _dev_f32(points, dev)
                tails = (points, dense, recon) if dev is not None else None
                got = self.db_sampler._run(gt_dict["gt_boxes"], gt_dict["gt_names"], self.object_store, dev, tails, self.distillation)
                if got is not None:
                    gt_dict["gt_names"] = np.concatenate([gt_dict["gt_names"], got["gt_names"]], 0)
                    gt_dict["gt_boxes"] = np.concatenate([_f32(gt_dict["gt_boxes"]).reshape(-1, got["gt_boxes"].shape[1]), got["gt_boxes"]], 0)
                    mask = np.concatenate([mask, got["gt_masks"]], 0)
                    if dev is not None:
                        points, dense, recon = got["_clouds"]
                    else:
                        front = lambda block, cloud: torch.cat([torch.from_numpy(block), cloud], 0) if torch.is_tensor(cloud) \
                            else np.concatenate([block, cloud], 0)
                        if self.distillation:
                            dense, recon = front(got["points"], dense), front(got["recon_points"], recon)
                        points = front(got["points"], points)
            _select(gt_dict, mask)
            gt_dict["gt_classes"] = np.array([self.class_names.index(n) + 1 for n in gt_dict["gt_names"]], np.int32)
            if not self.no_augmentation:
                if self.distillation:
                    gt_dict["gt_boxes"], points, dense, recon = global_noise(gt_dict["gt_boxes"], points, dense, recon, self.cfg)
                else:
                    gt_dict["gt_boxes"], points = global_noise(gt_dict["gt_boxes"], points, self.cfg)
        if self.shuffle_points:
            if self.distillation:
                points, dense = shuffle_points(points, dense)
            else:
                points = shuffle_points(points)
        lidar["points"] = points
        if self.distillation:
            lidar["dense_points"], lidar["reconstruction_points"] = dense, recon
        if self.mode == "train":
            lidar["annotations"] = gt_dict
        return res, info


# ---- GT-database sampler -----------------------------------------------------------------------------------------------------------
_CORNER_SIGNS = ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5))   # corners_nd's clockwise order (box_np_ops.py:78-83)


def _bev_corners_np(boxes, dtype=np.float32):
    b = np.asarray(boxes).astype(dtype, copy=False)
    r = np.asarray(boxes)[:, -1].astype(np.float64)
    c, s = np.cos(r).astype(dtype)[:, None], np.sin(r).astype(dtype)[:, None]
    norm = np.array(_CORNER_SIGNS, dtype)
    x, y = b[:, None, 3] * norm[None, :, 0], b[:, None, 4] * norm[None, :, 1]
    return np.stack([(x * c + y * s) + b[:, None, 0], (x * -s + y * c) + b[:, None, 1]], -1)


def bev_corners(boxes):
    """BEV corners [N, 4, 2] fp32 = center_to_corner_box2d(b[:, 0:2], b[:, 3:5], b[:, -1]) (box_np_ops.py:265-285): the yaw in the last
    column, its cos and sin in double.  numpy in, numpy out; tensor in, tensor out (computed on the host: N is a frame's box count)."""
    if torch.is_tensor(boxes):
        return torch.from_numpy(_bev_corners_np(_f32(boxes).reshape(-1, boxes.shape[-1]))).to(boxes.device)
    b = _f32(boxes)
    if b.ndim != 2 or (b.shape[0] and b.shape[1] < 7):
        raise _lib.S2DError(f"boxes {b.shape}: [N, >= 7] expected (centre, size, ..., yaw last)")
    return _bev_corners_np(b)


def _holds_np(b, q):
    """[N, K]: every corner of q[j] strictly inside b[i] (preprocess.py:973-985)"""
    ok = np.ones((b.shape[0], q.shape[0]), np.bool_)
    for k in range(4):
        v = -(b[:, k] - b[:, (k + 1) % 4])
        for l in range(4):
            cross = v[:, None, 1] * (b[:, None, k, 0] - q[None, :, l, 0])
            cross = cross - v[:, None, 0] * (b[:, None, k, 1] - q[None, :, l, 1])
            ok &= ~(cross >= 0)
    return ok


def _collision_np(c, q):
    """box_collision_test(c, q) in the dtype of its arguments, `is True / is False` by value: crossing edges or containment"""
    n, k = c.shape[0], q.shape[0]
    if n == 0 or k == 0:
        return np.zeros((n, k), np.bool_)
    iw = np.minimum(c[:, :, 0].max(1)[:, None], q[:, :, 0].max(1)[None]) - np.maximum(c[:, :, 0].min(1)[:, None], q[:, :, 0].min(1)[None])
    ih = np.minimum(c[:, :, 1].max(1)[:, None], q[:, :, 1].max(1)[None]) - np.maximum(c[:, :, 1].min(1)[:, None], q[:, :, 1].min(1)[None])
    near = (iw > 0) & (ih > 0)
    hit = np.zeros((n, k), np.bool_)
    for e in range(4):
        a0, a1 = c[:, None, e, 0], c[:, None, e, 1]
        b0, b1 = c[:, None, (e + 1) % 4, 0], c[:, None, (e + 1) % 4, 1]
        for l in range(4):
            c0, c1 = q[None, :, l, 0], q[None, :, l, 1]
            d0, d1 = q[None, :, (l + 1) % 4, 0], q[None, :, (l + 1) % 4, 1]
            acd = (d1 - a1) * (c0 - a0) > (c1 - a1) * (d0 - a0)
            bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0)
            abc = (c1 - a1) * (b0 - a0) > (b1 - a1) * (c0 - a0)
            abd = (d1 - a1) * (b0 - a0) > (b1 - a1) * (d0 - a0)
            hit |= (acd != bcd) & (abc != abd)
    return near & (hit | _holds_np(c, q) | _holds_np(q, c).T)


def _corners_arg(c, what):
    if c.ndim != 3 or c.shape[1:] != (4, 2):
        raise _lib.S2DError(f"{what} {tuple(c.shape)}: [N, 4, 2] expected")
    return c


def box_collision_test(corners, qcorners):
    """bool [N, K] = box_collision_test(corners, qcorners) of the reference (core/sampler/preprocess.py:922-1005), fp32: the stand-up
    boxes overlap and either two edges cross or one rectangle holds all four corners of the other.  The reference's `ret[i, j] is True /
    is False` are read by value, as numba reads them: containment is a collision (run as plain Python the reference skips that test).
    numpy in, numpy out; CUDA tensor in, tensor out."""
    if _on_device(corners, qcorners):
        dev = corners.device if torch.is_tensor(corners) and corners.is_cuda else qcorners.device
        c, q = _corners_arg(_dev_f32(corners, dev), "corners"), _corners_arg(_dev_f32(qcorners, dev), "qcorners")
        out = torch.zeros((c.shape[0], q.shape[0]), dtype=torch.bool, device=dev)
        if out.numel():
            _lib.check(_lib.load().s2d_prep_box_collision(c.data_ptr(), c.shape[0], q.data_ptr(), q.shape[0], out.data_ptr(), _stream(dev)),
                       "s2d_prep_box_collision")
        return out
    out = _collision_np(_corners_arg(_f32(corners), "corners"), _corners_arg(_f32(qcorners), "qcorners"))
    return torch.from_numpy(out) if torch.is_tensor(corners) else out


def collision_clear(boxes, qboxes, eps):
    """bool [N, K], float64: the pair's decision is the same with both rectangles' BEV sizes as given, grown by eps and shrunk by eps.  The
    decision is monotone in the sizes, so a clear pair cannot depend on rounding; the tests evaluate only clear pairs."""
    b, q = np.asarray(boxes, np.float64), np.asarray(qboxes, np.float64)

    def decide(d):
        x, y = b.copy(), q.copy()
        x[:, 3:5], y[:, 3:5] = np.maximum(x[:, 3:5] + d, 0.0), np.maximum(y[:, 3:5] + d, 0.0)
        return _collision_np(_bev_corners_np(x, np.float64), _bev_corners_np(y, np.float64))
    as_given = decide(0.0)
    return (decide(eps) == as_given) & (decide(-eps) == as_given)


class _BatchSampler:
    """BatchSampler of core/sampler/preprocess.py:19-54 on indices: one shuffle at construction, `idx + num >= n` returns the tail
    (possibly fewer than num, also when the sum equals n) and reshuffles"""

    def __init__(self, n):
        self.indices, self.idx, self.n = np.arange(n), 0, n
        np.random.shuffle(self.indices)

    def sample(self, num):
        if self.idx + num >= self.n:
            ret = self.indices[self.idx:].copy()
            np.random.shuffle(self.indices)
            self.idx = 0
        else:
            ret = self.indices[self.idx:self.idx + num]
            self.idx += num
        return ret


def _db_filter(db_infos, step):
    """one entry of db_prep_steps (builder.py:101-111 over DBFilterByDifficulty / DBFilterByMinNumPoint) or a callable"""
    if callable(step):
        return step(db_infos)
    if "filter_by_difficulty" in step:
        removed = step["filter_by_difficulty"]
        return {k: [i for i in v if i["difficulty"] not in removed] for k, v in db_infos.items()}
    if "filter_by_min_num_points" in step:
        out = dict(db_infos)
        for name, min_num in step["filter_by_min_num_points"].items():
            if min_num > 0:
                out[name] = [i for i in out[name] if i["num_points_in_gt"] >= min_num]
        return out
    raise ValueError("unknown database prep type")


MAX_CANDIDATES, MAX_GROUPS = 128, 16   # S2D_PREP_MAX_CANDIDATES, S2D_PREP_MAX_GROUPS (with MAX_BOXES for frame boxes + candidates)
SAMPLER_LAUNCHES, SAMPLER_HOST_READS = 4, 1   # select, count, segments, paste; accept[S] and the two row counts in one copy


def _indexed(device):
    """"cuda" -> the current device with its index, so that a resident store is recognised under either spelling"""
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device


class GTSampler:
    """`DataBaseSamplerV2.sample_all` (core/sampler/sample_ops.py:134-359) without group sampling, per-object rotation and random_crop.

    db_infos: the reference's dictionary name -> list of info dictionaries (name, path, box3d_lidar, num_points_in_gt, difficulty,
    gt_signs).  sample_groups: [{class: max_num}, ...].  db_prep_steps: the config's filter dictionaries (or callables), applied once, in
    order.  points_of(info) -> [P, C] replaces `np.fromfile(root / path)`.  One BatchSampler per class of the filtered dictionary is built in
    its order (one `np.random.shuffle` each) and keeps its position across frames: ONE SAMPLER HOLDS THAT STATE AND IS NOT TO BE SHARED
    BETWEEN THREADS.  A completed cloud of 0 rows counts as none, as in `compose_clouds`."""

    def __init__(self, db_infos, sample_groups, rate=1.0, db_prep_steps=(), points_of=None, global_rot_range=None):
        if callable(db_prep_steps):
            db_prep_steps = (db_prep_steps,)
        for step in db_prep_steps or ():
            db_infos = _db_filter(db_infos, step)
        self.db_infos = {k: list(v) for k, v in db_infos.items()}
        self.rate = rate
        self.classes, self.max_nums = [], []
        for group in sample_groups:
            if len(group) > 1:
                raise NotImplementedError("GTSampler: group sampling (a sample group naming more than one class) is out of scope")
            self.classes += list(group.keys())
            self.max_nums += list(group.values())
        if global_rot_range is not None:   # (an empty list is the builder's "none": builder.py:287-289)
            rot = np.atleast_1d(np.asarray(global_rot_range, np.float64))
            global_rot_range = None if rot.size == 0 else [-rot[0], rot[0]] if rot.size == 1 else rot
        if global_rot_range is not None:
            if len(global_rot_range) != 2:
                raise _lib.S2DError("GTSampler: global_rot_range: a scalar or two values expected")
            if np.abs(global_rot_range[0] - global_rot_range[1]) >= 1e-3:
                raise NotImplementedError("GTSampler: per-object rotation noise (global_random_rotation_range_per_object) is out of scope")
        if points_of is None:
            raise _lib.S2DError("GTSampler: points_of(info) -> [P, C] is required (it replaces the reference's point files)")
        self.points_of = points_of
        self._samplers = {k: _BatchSampler(len(v)) for k, v in self.db_infos.items()}
        self._resident = None

    # -- stores
    def resident(self, device, object_store=None):
        """packs every object's sweep rows (and, with object_store, its completed cloud) after the filters into one store with offsets on the
        device, so a frame uploads only boxes and row ranges.  Returns self."""
        device = _indexed(torch.device(device))
        rows, ccs, index = [], [], {}
        for name, infos in self.db_infos.items():
            for k, info in enumerate(infos):
                index[(name, k)] = len(rows)
                rows.append(_f32(self.points_of(info)))
                g = object_store(info["gt_signs"]) if object_store is not None else None
                ccs.append(None if g is None or not len(g) else _f32(g))
        ncols = rows[0].shape[1] if rows else 5
        pack = lambda parts: torch.from_numpy(np.concatenate(parts, 0) if parts else np.zeros((0, ncols), np.float32)).to(device)
        self._resident = dict(device=device, index=index, ncols=ncols, points=pack(rows), offsets=np.cumsum([0] + [len(r) for r in rows]),
                              cc=pack([g for g in ccs if g is not None]) if object_store is not None else None,
                              cc_offsets=np.cumsum([0] + [0 if g is None else len(g) for g in ccs]))
        return self

    # -- the host draws
    def _draw(self, gt_names):
        """[(class, indices into db_infos[class])] of the groups that sample, in group order: every `np.random` draw of the frame"""
        out = []
        for name, max_num in zip(self.classes, self.max_nums):
            num = np.round(self.rate * int(max_num - np.sum([n == name for n in gt_names]))).astype(np.int64)
            if num <= 0:
                continue
            if not self.db_infos.get(name):
                raise _lib.S2DError(f"GTSampler: class {name!r} is sampled but has no database entries")
            idx = self._samplers[name].sample(num)
            if len(idx):
                out.append((name, idx))
        return out

    def sample_all(self, gt_boxes, gt_names, object_store=None, device=None, random_crop=False):
        """the reference's dictionary (gt_names, difficulty, gt_boxes, points, gt_masks, recon_points, group_ids) or None when nothing is
        accepted.  gt_boxes, gt_names: the frame's objects after the DontCare / ignore / UNKNOWN drop.  object_store: name -> completed
        cloud or None, asked with info["gt_signs"].  device None: the numpy restatement; a CUDA device: the kernels (clouds stay there)."""
        if random_crop:
            raise NotImplementedError("GTSampler: random_crop is out of scope")
        return self._run(gt_boxes, gt_names, object_store, device)

    def _run(self, gt_boxes, gt_names, object_store, device, tails=None, want_recon=True):
        gt_boxes = _f32(gt_boxes)
        if gt_boxes.ndim != 2 or (gt_boxes.shape[0] and gt_boxes.shape[1] < 7):
            raise _lib.S2DError(f"gt_boxes {gt_boxes.shape}: [M, >= 7] expected (centre, size, ..., yaw last)")
        if len(gt_names) != gt_boxes.shape[0]:
            raise _lib.S2DError(f"gt_names: {len(gt_names)} entries for {gt_boxes.shape[0]} boxes")
        groups = self._draw(gt_names)
        if not groups:
            return None
        cand = [(name, int(k), self.db_infos[name][int(k)]) for name, idx in groups for k in idx]
        ends = np.cumsum([len(idx) for _, idx in groups]).astype(np.int32)
        cand_boxes = np.stack([_f32(info["box3d_lidar"]) for _, _, info in cand], 0)
        if gt_boxes.shape[0] and cand_boxes.shape[1] != gt_boxes.shape[1]:
            raise _lib.S2DError(f"GTSampler: database boxes have {cand_boxes.shape[1]} columns, the frame's {gt_boxes.shape[1]}")
        avoid = gt_boxes.reshape(-1, cand_boxes.shape[1])
        object_store = object_store if object_store is not None else (lambda name: None)
        if device is None:
            out = self._run_np(avoid, cand, cand_boxes, ends, object_store, want_recon)
        else:
            out = self._run_device(avoid, cand, cand_boxes, ends, object_store, _indexed(torch.device(device)), tails, want_recon)
        if out is None:
            return None
        accept, points, recon, clouds = out
        kept = [info for ok, (_, _, info) in zip(accept, cand) if ok]
        ret = {"gt_names": np.array([i["name"] for i in kept]), "difficulty": np.array([i["difficulty"] for i in kept]),
               "gt_boxes": cand_boxes[np.asarray(accept, np.bool_)], "points": points, "gt_masks": np.ones((len(kept),), np.bool_),
               "recon_points": recon, "group_ids": np.arange(avoid.shape[0], avoid.shape[0] + len(kept))}
        if clouds is not None:
            ret["_clouds"] = clouds
        return ret

    @staticmethod
    def select_np(avoid, cand_boxes, ends):
        """accept [S] of the restatement: per group, box_collision_test over [avoid; accepted so far; this group's candidates] with the
        diagonal cleared, candidates walked in order, a rejected one's row and column cleared (sample_ops.py:313-359)"""
        accept, start = np.zeros(len(cand_boxes), np.bool_), 0
        for end in ends:
            total = np.concatenate([avoid, cand_boxes[:start][accept[:start]], cand_boxes[start:end]], 0)
            corners = _bev_corners_np(total)
            first, count = len(total) - (end - start), end - start
            coll = _collision_np(corners[first:], corners)   # only the candidates' rows are ever read
            coll[np.arange(count), first + np.arange(count)] = False
            for k in range(count):
                if coll[k].any():
                    coll[k], coll[:, first + k] = False, False
                else:
                    accept[start + k] = True
            start = end
        return accept

    def _run_np(self, avoid, cand, cand_boxes, ends, object_store, want_recon):
        accept = self.select_np(avoid, cand_boxes, ends)
        if not accept.any():
            return None
        blocks, recon = [], []
        for ok, (_, _, info), box in zip(accept, cand, cand_boxes):
            if not ok:
                continue
            rows = _f32(self.points_of(info)).copy()
            rows[:, :3] += box[:3]
            blocks.append(rows)
            if not want_recon:
                continue
            g = object_store(info["gt_signs"])
            if g is None or not len(g):
                recon.append(rows)
            else:
                g = _object_block_np(_f32(g).reshape(-1, rows.shape[1]), kinds_of([info["name"]])[0], box)
                recon.append(g[_inside_np(g, box[None]).any(1)])
        return accept, np.concatenate(blocks, 0), np.concatenate(recon, 0) if want_recon else None, None

    def _run_device(self, avoid, cand, cand_boxes, ends, object_store, dev, tails, want_recon):
        lib = _lib.load()
        m, s = avoid.shape[0], cand_boxes.shape[0]
        size = lib.s2d_prep_gt_scratch_bytes(m, s) if len(ends) <= MAX_GROUPS else 0
        if size == 0:
            raise _lib.S2DError(f"GTSampler: {m} frame boxes + {s} candidates in {len(ends)} groups: at most {MAX_BOXES} boxes, {MAX_CANDIDATES} "
                                f"candidates and {MAX_GROUPS} groups on the device")
        res = self._resident if self._resident is not None and self._resident["device"] == dev else None
        meta = np.zeros((s, 5), np.int32)
        meta[:, 4] = kinds_of([info["name"] for _, _, info in cand])
        if res is not None:
            obj = np.array([res["index"][(name, k)] for name, k, _ in cand], np.int64)
            src, meta[:, 0], meta[:, 1] = res["points"], res["offsets"][obj], res["offsets"][obj + 1]
        else:   # the candidates' rows packed on the host, one upload
            rows = [_f32(self.points_of(info)) for _, _, info in cand]
            off = np.cumsum([0] + [len(r) for r in rows])
            src, meta[:, 0], meta[:, 1] = torch.from_numpy(np.concatenate(rows, 0)).to(dev), off[:-1], off[1:]
        ncols = src.shape[1]
        cc = torch.zeros((0, ncols), dtype=torch.float32, device=dev)
        if want_recon and res is not None and res["cc"] is not None:
            cc, meta[:, 2], meta[:, 3] = res["cc"], res["cc_offsets"][obj], res["cc_offsets"][obj + 1]
        elif want_recon:
            parts = [object_store(info["gt_signs"]) for _, _, info in cand]
            parts = [None if g is None or not len(g) else g for g in parts]
            off = np.cumsum([0] + [0 if g is None else len(g) for g in parts])
            meta[:, 2], meta[:, 3] = off[:-1], off[1:]
            parts = [g for g in parts if g is not None]
            if parts and any(torch.is_tensor(g) for g in parts):
                cc = torch.cat([_dev_f32(g, dev).reshape(-1, ncols) for g in parts], 0)
            elif parts:
                cc = torch.from_numpy(np.concatenate([_f32(g).reshape(-1, ncols) for g in parts], 0)).to(dev)
        for t in tails or ():
            if t is not None and (t.shape[1] != ncols or t.dtype != torch.float32):
                raise _lib.S2DError(f"GTSampler: the database rows have {ncols} columns, the frame's clouds {t.shape[1]}")
        boxes = torch.from_numpy(np.concatenate([avoid, cand_boxes], 0)).to(dev)
        meta_d = torch.from_numpy(meta).to(dev)
        ws = _ws(size, dev)
        header = torch.empty(2 + s, dtype=torch.int32, device=dev)
        st = _stream(dev)
        ends_c = (ctypes.c_int32 * len(ends))(*[int(e) for e in ends])
        _lib.check(lib.s2d_prep_gt_select(boxes.data_ptr(), m, s, boxes.shape[1], ends_c, len(ends), meta_d.data_ptr(), cc.data_ptr() if cc.shape[0] else None,
                                          src.shape[0], cc.shape[0], ncols, ws.data_ptr(), ws.numel(), header.data_ptr(), st), "s2d_prep_gt_select")
        head = header.tolist()   # the step's one host read
        n_s, n_r, accept = head[0], head[1] if want_recon else 0, head[2:]
        if not any(accept):
            return None
        t_points, t_dense, t_recon = tails if tails is not None else (None, None, None)
        room = lambda n, tail: torch.empty((n + (0 if tail is None else tail.shape[0]), ncols), dtype=torch.float32, device=dev)
        points = room(n_s, t_points)
        dense = room(n_s, t_dense) if t_dense is not None else None
        recon = room(n_r, t_recon) if want_recon else None
        _lib.check(lib.s2d_prep_gt_paste(s, ncols, meta_d.data_ptr(), src.data_ptr() if src.shape[0] else None, src.shape[0],
                                         cc.data_ptr() if cc.shape[0] else None, cc.shape[0], ws.data_ptr(), ws.numel(), header.data_ptr(),
                                         points.data_ptr() if n_s else None, dense.data_ptr() if dense is not None and n_s else None, n_s,
                                         recon.data_ptr() if n_r else None, n_r, st), "s2d_prep_gt_paste")
        for cloud, n, tail in ((points, n_s, t_points), (dense, n_s, t_dense), (recon, n_r, t_recon)):
            if cloud is not None and tail is not None:
                cloud[n:].copy_(tail)   # the old cloud follows by a plain device copy
        clouds = (points, dense, recon) if tails is not None else None
        return accept, points[:n_s], recon[:n_r] if want_recon else None, clouds


def build_gt_sampler(cfg, db_infos=None, points_of=None):
    """build_dbsampler (det3d/builder.py:276-294) on the reference's `db_sampler` dictionary: sample_groups, db_prep_steps, rate,
    global_random_rotation_range_per_object; db_info_path is unpickled only when db_infos is not given"""
    if db_infos is None:
        import pickle
        with open(_get(cfg, "db_info_path"), "rb") as f:
            db_infos = pickle.load(f)
    rot = list(_get(cfg, "global_random_rotation_range_per_object", []) or [])
    return GTSampler(db_infos, [dict(g) for g in _get(cfg, "sample_groups")], rate=_get(cfg, "rate", 1.0),
                     db_prep_steps=list(_get(cfg, "db_prep_steps", []) or []), points_of=points_of, global_rot_range=rot or None)
