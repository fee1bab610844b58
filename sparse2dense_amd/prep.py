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

Out of scope: the GT-database sampler (`db_sampler` must be None), `min_points_in_gt`, the evaluation-mode composition
(preprocess.py:215-254), `npoints` subsampling, nuScenes sweep combination, several frames per launch chain.
"""
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
    no_augmentation.  `object_store` is a callable name -> [P_j, C] array (or tensor) or None and replaces the reference's pickle paths.
    Writes res["lidar"]["points" / "dense_points" / "reconstruction_points"] and the filtered annotations with gt_classes.  A sweep that
    arrives as a CUDA tensor is prepared by the kernels and stays on the device; a numpy sweep takes the numpy restatement."""

    def __init__(self, cfg=None, object_store=None, **kwargs):
        self.mode = _get(cfg, "mode")
        self.shuffle_points = _get(cfg, "shuffle_points", False)
        self.distillation = _get(cfg, "distillation", False)
        self.no_augmentation = _get(cfg, "no_augmentation", False)
        self.cfg = cfg
        if _get(cfg, "db_sampler") is not None:
            raise NotImplementedError("S2DPreprocess: the GT-database sampler is out of scope (db_sampler must be None)")
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
            _select(gt_dict, np.array([n in self.class_names for n in gt_dict["gt_names"]], np.bool_))
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
