"""SECOND anchor head plumbing around csrc/anchor_head.hip (Waymo configuration of
configs/waymo/voxelnet/waymo_second_3x_interval_5.py):

  AnchorGeneratorRange / generate_anchors   det3d/core/anchor/anchor_generator.py:64-116 over create_anchors_3d_range
                                            (det3d/core/bbox/box_np_ops.py:857-930); target_assigner.py:139-158
  GroundBox3dCoder                          det3d/core/bbox/box_coders.py (ground_box3d_coder) over second_box_encode / _decode
  assign_anchor_targets                     AssignTarget (det3d/datasets/pipelines/preprocess.py:656-833) on the device
  AnchorLossFn / anchor_loss                MultiGroupHead.loss for one task (det3d/models/bbox_heads/mg_head.py:535-667)
  decode_anchors                            the per-anchor part of MultiGroupHead.predict (mg_head.py:737-765,838-849,995-1001)

The anchors are made once per feature-map size on the host (numpy, the reference's own arithmetic) and cached as a device tensor;
everything per frame runs in HIP kernels.  Options outside the Waymo SECOND configuration raise NotImplementedError naming the option."""
import ctypes

import numpy as np
import torch

from . import _lib

def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


# ---- anchors -----------------------------------------------------------------------------------------------------------------------
def create_anchors_3d_range(feature_size, anchor_range, sizes, rotations, dtype=np.float32):
    """feature_size (D, H, W) -> anchors [D, H, W, num_sizes, num_rotations, 7] (x, y, z, w, l, h, r).  Both centre axes use the x stride,
    as the reference does."""
    anchor_range = np.array(anchor_range, dtype)
    stride = (anchor_range[3] - anchor_range[0]) / feature_size[2]
    z = np.linspace(anchor_range[2], anchor_range[5], feature_size[0], dtype=dtype)
    y = np.linspace(anchor_range[1], anchor_range[4], feature_size[1], endpoint=False, dtype=dtype) + stride / 2
    x = np.linspace(anchor_range[0], anchor_range[3], feature_size[2], endpoint=False, dtype=dtype) + stride / 2
    rotations = np.array(rotations, dtype=dtype)
    sizes = np.reshape(np.array(sizes, dtype=dtype), [-1, 3])
    out = np.zeros((feature_size[0], feature_size[1], feature_size[2], sizes.shape[0], rotations.shape[0], 7), dtype)
    out[..., 0] = x[None, None, :, None, None]
    out[..., 1] = y[None, :, None, None, None]
    out[..., 2] = z[:, None, None, None, None]
    out[..., 3:6] = sizes[None, None, None, :, None, :]
    out[..., 6] = rotations[None, None, None, None, :]
    return out


class AnchorGeneratorRange:
    def __init__(self, anchor_ranges, sizes=(1.6, 3.9, 1.56), rotations=(0, np.pi / 2), class_name=None, match_threshold=-1,
                 unmatch_threshold=-1, dtype=np.float32):
        self.anchor_ranges, self.sizes, self.rotations = list(anchor_ranges), list(sizes), list(rotations)
        self.class_name, self.match_threshold, self.unmatch_threshold, self.dtype = class_name, match_threshold, unmatch_threshold, dtype

    @property
    def num_anchors_per_localization(self):
        return len(self.rotations) * np.array(self.sizes).reshape([-1, 3]).shape[0]

    def generate(self, feature_map_size):
        return create_anchors_3d_range(feature_map_size, self.anchor_ranges, self.sizes, self.rotations, self.dtype)


def build_anchor_generator(cfg):
    """anchor_generator_range only; the Waymo configs carry no velocities: anchors are 7 wide"""
    kind = _get(cfg, "type")
    if kind != "anchor_generator_range":
        raise NotImplementedError(f"anchor generator type {kind!r} is not supported (anchor_generator_range only)")
    if _get(cfg, "velocities") is not None:
        raise NotImplementedError("anchor generator option 'velocities' is not supported (7-wide anchors only)")
    return AnchorGeneratorRange(anchor_ranges=_get(cfg, "anchor_ranges"), sizes=_get(cfg, "sizes"), rotations=_get(cfg, "rotations"),
                                class_name=_get(cfg, "class_name"), match_threshold=_get(cfg, "matched_threshold"),
                                unmatch_threshold=_get(cfg, "unmatched_threshold"))


def generate_anchors(generators, feature_map_size):
    """[H * W * slots, 7] in the head's order: the classes concatenated along the slot axis of each cell"""
    per_class = []
    for g in generators:
        a = g.generate(feature_map_size)
        per_class.append(a.reshape([*a.shape[:3], -1, a.shape[-1]]))
    return np.concatenate(per_class, axis=-2).reshape(-1, per_class[0].shape[-1])


# ---- box coder ---------------------------------------------------------------------------------------------------------------------
class GroundBox3dCoder:
    """ground_box3d_coder with linear_dim=False, encode_angle_vector=False, n_dim=7"""

    def __init__(self, linear_dim=False, encode_angle_vector=False, n_dim=7):
        if linear_dim:
            raise NotImplementedError("box coder option 'linear_dim' is not supported")
        if encode_angle_vector:
            raise NotImplementedError("box coder option 'encode_angle_vector' is not supported")
        if n_dim != 7:
            raise NotImplementedError(f"box coder option 'n_dim'={n_dim} is not supported (7 only)")
        self.linear_dim, self.vec_encode, self.n_dim = False, False, 7

    @property
    def code_size(self):
        return self.n_dim

    @staticmethod
    def _encode(boxes, anchors, lib):
        xa, ya, za, wa, la, ha, ra = [anchors[..., i] for i in range(7)]
        xg, yg, zg, wg, lg, hg, rg = [boxes[..., i] for i in range(7)]
        diagonal = lib.sqrt(la ** 2 + wa ** 2)
        return lib.stack([(xg - xa) / diagonal, (yg - ya) / diagonal, (zg - za) / ha, lib.log(wg / wa), lib.log(lg / la), lib.log(hg / ha),
                          rg - ra], -1)

    @staticmethod
    def _decode(enc, anchors, lib):
        xa, ya, za, wa, la, ha, ra = [anchors[..., i] for i in range(7)]
        xt, yt, zt, wt, lt, ht, rt = [enc[..., i] for i in range(7)]
        diagonal = lib.sqrt(la ** 2 + wa ** 2)
        return lib.stack([xt * diagonal + xa, yt * diagonal + ya, zt * ha + za, lib.exp(wt) * wa, lib.exp(lt) * la, lib.exp(ht) * ha,
                          rt + ra], -1)

    def encode(self, boxes, anchors):
        return self._encode(boxes, anchors, np)

    def decode(self, encodings, anchors):
        return self._decode(encodings, anchors, np)

    def encode_torch(self, boxes, anchors):
        return self._encode(boxes, anchors, torch)

    def decode_torch(self, encodings, anchors):
        return self._decode(encodings, anchors, torch)


def build_box_coder(cfg):
    """a coder object passes through; a dictionary (what the shim's det3d.builder.build_box_coder returns) builds one"""
    if isinstance(cfg, GroundBox3dCoder):
        return cfg
    if not isinstance(cfg, dict):
        raise NotImplementedError(f"box coder {type(cfg).__name__} is not supported (ground_box3d_coder only)")
    kind = cfg.get("type", "ground_box3d_coder")
    if kind != "ground_box3d_coder":
        raise NotImplementedError(f"box coder type {kind!r} is not supported (ground_box3d_coder only)")
    extra = sorted(set(cfg) - {"type", "code_size", "linear_dim", "encode_angle_vector", "n_dim"})
    if extra:
        raise NotImplementedError(f"box coder option(s) {extra} are not supported")
    return GroundBox3dCoder(**{k: v for k, v in cfg.items() if k not in ("type", "code_size")})


# ---- target assignment -------------------------------------------------------------------------------------------------------------
class AnchorAssigner:
    """the parsed `assigner` dictionary of a SECOND config (train_cfg.assigner): generators, thresholds, cached device anchors"""

    def __init__(self, cfg):
        ta = _get(cfg, "target_assigner")
        self.box_coder = build_box_coder(_get(cfg, "box_coder"))
        self.out_size_factor = int(_get(cfg, "out_size_factor", 8))
        if _get(ta, "type", "iou") != "iou":
            raise NotImplementedError(f"target_assigner type {_get(ta, 'type')!r} is not supported ('iou' only)")
        sim = _get(_get(ta, "region_similarity_calculator"), "type")
        if sim != "nearest_iou_similarity":
            raise NotImplementedError(f"region_similarity_calculator {sim!r} is not supported (nearest_iou_similarity only)")
        if _get(ta, "sample_positive_fraction", -1) >= 0:
            raise NotImplementedError("target_assigner option 'sample_positive_fraction' >= 0 (anchor sampling) is not supported")
        if _get(ta, "pos_area_threshold", -1) >= 0:
            raise NotImplementedError("target_assigner option 'pos_area_threshold' >= 0 (anchors_mask) is not supported")
        tasks = _get(ta, "tasks")
        if len(tasks) != 1:
            raise NotImplementedError(f"{len(tasks)} tasks are not supported (one task only)")
        self.class_names = list(_get(tasks[0], "class_names"))
        self.generators = [build_anchor_generator(g) for g in _get(ta, "anchor_generators")]
        if [g.class_name for g in self.generators] != self.class_names:
            raise NotImplementedError("anchor_generators must list one generator per class of the task, in the task's class order")
        rots = {len(g.rotations) for g in self.generators}
        if len(rots) != 1 or any(g.num_anchors_per_localization != len(g.rotations) for g in self.generators):
            raise NotImplementedError("anchor_generators must share the number of rotations and carry one size each")
        self.rotations = rots.pop()
        self.num_classes = len(self.generators)
        self.matched = np.asarray([g.match_threshold for g in self.generators], np.float32)
        self.unmatched = np.asarray([g.unmatch_threshold for g in self.generators], np.float32)
        self._cache = {}

    def anchors_numpy(self, feature_map_size):
        return generate_anchors(self.generators, feature_map_size)

    def anchors(self, feature_map_size, device):
        key = (tuple(int(s) for s in feature_map_size), str(device))
        a = self._cache.get(key)
        if a is None:
            a = self._cache[key] = torch.from_numpy(self.anchors_numpy(feature_map_size)).to(device)
        return a


_assigners = {}


def get_assigner(cfg):
    if isinstance(cfg, AnchorAssigner):
        return cfg
    a = _assigners.get(id(cfg))
    if a is None or a[0] is not cfg:
        a = _assigners[id(cfg)] = (cfg, AnchorAssigner(cfg))
    return a[1]


def _stream(dev):
    return torch._C._cuda_getCurrentRawStream(dev.index)


def _floats(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def _ws(nbytes, device):
    """caller-owned scratch of one entry: a plain allocation of exactly the queried size (the seam tests/ws_guard.py replaces)"""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def assign_anchor_targets(gt_boxes, gt_classes, cfg, grid_xy=(1504, 1504)):
    """gt_boxes f32[B,K,7] (x,y,z,w,l,h,r; a 9-wide tensor with the velocities in columns 6:8 is accepted and narrowed) cuda,
    gt_classes i32[B,K] cuda (0 = padding), cfg = the config's `assigner` dictionary -> the example fields of AssignTarget after
    collate_kitti, one list entry per task: anchors [f32[B,A,7]], labels [i32[B,A]], reg_targets [f32[B,A,7]], reg_weights [f32[B,A]]."""
    if not (torch.is_tensor(gt_boxes) and gt_boxes.is_cuda and torch.is_tensor(gt_classes) and gt_classes.is_cuda):
        raise _lib.S2DError("assign_anchor_targets: CUDA tensors expected (no CPU fallback)")
    asg = get_assigner(cfg)
    lib = _lib.load()
    if gt_boxes.shape[-1] == 9:
        gt_boxes = torch.cat((gt_boxes[..., :6], gt_boxes[..., 8:9]), -1)
    if gt_boxes.dim() != 3 or gt_boxes.shape[-1] != 7:
        raise _lib.S2DError(f"assign_anchor_targets: gt_boxes must be [B, K, 7], got {tuple(gt_boxes.shape)}")
    gt_boxes, gt_classes = gt_boxes.float().contiguous(), gt_classes.int().contiguous()
    b, k = gt_classes.shape
    dev = gt_boxes.device
    fmap = [1, grid_xy[1] // asg.out_size_factor, grid_xy[0] // asg.out_size_factor]
    anchors = asg.anchors(fmap, dev)
    a = anchors.shape[0]
    labels = torch.empty((b, a), dtype=torch.int32, device=dev)
    reg_targets = torch.empty((b, a, 7), dtype=torch.float32, device=dev)
    reg_weights = torch.empty((b, a), dtype=torch.float32, device=dev)
    ws = _ws(max(int(lib.s2d_anchor_assign_workspace_bytes(b, k)), 256), dev)
    _lib.check(lib.s2d_anchor_assign(gt_boxes.data_ptr(), gt_classes.data_ptr(), b, k, anchors.data_ptr(), a, asg.num_classes, asg.rotations,
                                     _floats(asg.matched), _floats(asg.unmatched), labels.data_ptr(), reg_targets.data_ptr(),
                                     reg_weights.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "s2d_anchor_assign")
    return dict(anchors=[anchors.unsqueeze(0).expand(b, a, 7)], labels=[labels], reg_targets=[reg_targets], reg_weights=[reg_weights])


# ---- loss --------------------------------------------------------------------------------------------------------------------------
LOSS_KEYS = ("loss", "cls_pos_loss", "cls_neg_loss", "dir_loss_reduced", "cls_loss_reduced", "loc_loss_reduced")


def loss_params(loss_norm, loss_cls, loss_bbox, loss_aux, direction_offset=0.0, encode_rad_error_by_sin=True):
    """the nine floats s2d_anchor_loss_* take, from the head's loss dictionaries; anything but the Waymo SECOND combination raises"""
    if loss_norm is None or loss_cls is None or loss_bbox is None:
        raise NotImplementedError("MultiGroupHead.loss needs loss_norm, loss_cls and loss_bbox (a forward-only head was built)")
    if loss_aux is None:
        raise NotImplementedError("MultiGroupHead without a direction classifier (loss_aux) is not supported")
    if not encode_rad_error_by_sin:
        raise NotImplementedError("encode_rad_error_by_sin=False is not supported")
    if _get(loss_norm, "type") != "NormByNumPositives":
        raise NotImplementedError(f"loss_norm type {_get(loss_norm, 'type')!r} is not supported (NormByNumPositives only)")
    if _get(loss_cls, "type") != "SigmoidFocalLoss":
        raise NotImplementedError(f"loss_cls type {_get(loss_cls, 'type')!r} is not supported (SigmoidFocalLoss only)")
    if _get(loss_bbox, "type") != "WeightedSmoothL1Loss":
        raise NotImplementedError(f"loss_bbox type {_get(loss_bbox, 'type')!r} is not supported (WeightedSmoothL1Loss only)")
    if not _get(loss_bbox, "codewise", True):
        raise NotImplementedError("loss_bbox option 'codewise'=False is not supported")
    if _get(loss_aux, "type") != "WeightedSoftmaxClassificationLoss":
        raise NotImplementedError(f"loss_aux type {_get(loss_aux, 'type')!r} is not supported (WeightedSoftmaxClassificationLoss only)")
    if float(_get(loss_aux, "logit_scale", 1.0)) != 1.0:
        raise NotImplementedError("loss_aux option 'logit_scale' != 1 is not supported")
    gamma = float(_get(loss_cls, "gamma", 2.0))
    if gamma != 2.0:
        raise NotImplementedError(f"loss_cls option 'gamma'={gamma} is not supported (2.0 only)")
    # (the reference's WeightedSmoothL1Loss drops its code_weights - losses.py:167-173 - so they are not applied here either)
    return [float(_get(loss_norm, "pos_cls_weight", 1.0)), float(_get(loss_norm, "neg_cls_weight", 1.0)), float(_get(loss_cls, "alpha", 0.25)),
            gamma, float(_get(loss_bbox, "sigma", 3.0)), float(_get(loss_bbox, "loss_weight", 1.0)), float(_get(loss_cls, "loss_weight", 1.0)),
            float(_get(loss_aux, "loss_weight", 1.0)), float(direction_offset)]


def _check_loss_inputs(box_preds, cls_preds, dir_preds, labels, reg_targets, anchors):
    for name, t in (("box_preds", box_preds), ("cls_preds", cls_preds), ("dir_cls_preds", dir_preds), ("labels", labels),
                    ("reg_targets", reg_targets), ("anchors", anchors)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.S2DError(f"anchor loss: {name} must be a CUDA tensor (no CPU fallback)")
    b, a = labels.shape
    if box_preds.numel() != b * a * 7 or dir_preds.numel() != b * a * 2 or cls_preds.numel() % (b * a) or reg_targets.numel() != b * a * 7 \
            or anchors.shape != (a, 7):
        raise _lib.S2DError(f"anchor loss: shapes disagree (labels {tuple(labels.shape)}, box_preds {tuple(box_preds.shape)}, cls_preds "
                            f"{tuple(cls_preds.shape)}, dir_cls_preds {tuple(dir_preds.shape)}, anchors {tuple(anchors.shape)})")
    return b, a, cls_preds.numel() // (b * a)


class AnchorLossFn(torch.autograd.Function):
    """MultiGroupHead.loss of one task in two launches forward, one backward (csrc/anchor_head.hip).  Returns the 15-float result vector
    (loss, cls_pos_loss, cls_neg_loss, dir_loss_reduced, cls_loss_reduced, loc_loss_reduced, loc_loss_elem[7], num_pos, num_neg); only
    element 0 carries a gradient."""

    @staticmethod
    def forward(ctx, box_preds, cls_preds, dir_preds, labels, reg_targets, anchors, params):
        lib = _lib.load()
        b, a, c = _check_loss_inputs(box_preds, cls_preds, dir_preds, labels, reg_targets, anchors)
        box_preds, cls_preds, dir_preds = box_preds.float().contiguous(), cls_preds.float().contiguous(), dir_preds.float().contiguous()
        labels, reg_targets, anchors = labels.int().contiguous(), reg_targets.float().contiguous(), anchors.float().contiguous()
        dev = box_preds.device
        res = torch.empty(15, dtype=torch.float32, device=dev)
        norm = torch.empty(b, dtype=torch.float32, device=dev)
        ws = _ws(lib.s2d_anchor_loss_workspace_bytes(b), dev)
        cparams = _floats(params)
        _lib.check(lib.s2d_anchor_loss_fwd(box_preds.data_ptr(), cls_preds.data_ptr(), dir_preds.data_ptr(), labels.data_ptr(),
                                           reg_targets.data_ptr(), anchors.data_ptr(), b, a, c, cparams, res.data_ptr(), norm.data_ptr(),
                                           ws.data_ptr(), ws.numel(), _stream(dev)), "s2d_anchor_loss_fwd")
        ctx.save_for_backward(box_preds, cls_preds, dir_preds, labels, reg_targets, anchors, norm)
        ctx.params, ctx.dims = list(params), (b, a, c)
        return res

    @staticmethod
    def backward(ctx, go):
        box_preds, cls_preds, dir_preds, labels, reg_targets, anchors, norm = ctx.saved_tensors
        b, a, c = ctx.dims
        go0 = go[0:1].float().contiguous()   # the incoming gradient of `loss`: a device scalar, never read on the host
        dbox, dcls, ddir = torch.empty_like(box_preds), torch.empty_like(cls_preds), torch.empty_like(dir_preds)
        _lib.check(_lib.load().s2d_anchor_loss_bwd(box_preds.data_ptr(), cls_preds.data_ptr(), dir_preds.data_ptr(), labels.data_ptr(),
                                                   reg_targets.data_ptr(), anchors.data_ptr(), b, a, c, _floats(ctx.params), norm.data_ptr(),
                                                   go0.data_ptr(), dbox.data_ptr(), dcls.data_ptr(), ddir.data_ptr(), _stream(dbox.device)),
                   "s2d_anchor_loss_bwd")
        return dbox, dcls, ddir, None, None, None, None


def anchor_loss(box_preds, cls_preds, dir_preds, labels, reg_targets, anchors, params):
    """-> the reference's per-task return dictionary (device scalars; `loss` carries the graph)"""
    res = AnchorLossFn.apply(box_preds, cls_preds, dir_preds, labels, reg_targets, anchors, params)
    det = res.detach()
    ret = {"loss": res[0]}
    for i, k in enumerate(LOSS_KEYS[1:], 1):
        ret[k] = det[i]
    ret["loc_loss_elem"] = [det[6 + i] for i in range(7)]
    ret["num_pos"], ret["num_neg"] = det[13].long(), det[14].long()
    return ret


# ---- decode ------------------------------------------------------------------------------------------------------------------------
def decode_anchors(box_preds, cls_preds, dir_preds, anchors, score_threshold):
    """box_preds [B,...,A*7 flattened], cls_preds, dir_preds (or None), anchors [A,7] -> boxes f32[B,A,7], scores f32[B,A],
    labels i32[B,A], dir_labels i32[B,A], keep bool[B,A] (score >= threshold)"""
    for t in (box_preds, cls_preds, anchors):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise _lib.S2DError("decode_anchors: CUDA tensors expected (no CPU fallback)")
    lib = _lib.load()
    a = anchors.shape[0]
    b = box_preds.shape[0]
    if box_preds.numel() != b * a * 7 or cls_preds.numel() % (b * a) or (dir_preds is not None and dir_preds.numel() != b * a * 2):
        raise _lib.S2DError(f"decode_anchors: shapes disagree (box_preds {tuple(box_preds.shape)}, cls_preds {tuple(cls_preds.shape)}, "
                            f"anchors {tuple(anchors.shape)})")
    c = cls_preds.numel() // (b * a)
    box_preds, cls_preds, anchors = box_preds.float().contiguous(), cls_preds.float().contiguous(), anchors.float().contiguous()
    dir_preds = None if dir_preds is None else dir_preds.float().contiguous()
    dev = box_preds.device
    boxes = torch.empty((b, a, 7), dtype=torch.float32, device=dev)
    scores = torch.empty((b, a), dtype=torch.float32, device=dev)
    labels = torch.empty((b, a), dtype=torch.int32, device=dev)
    dirs = torch.empty((b, a), dtype=torch.int32, device=dev)
    keep = torch.empty((b, a), dtype=torch.uint8, device=dev)
    _lib.check(lib.s2d_anchor_decode(box_preds.data_ptr(), cls_preds.data_ptr(), None if dir_preds is None else dir_preds.data_ptr(),
                                     anchors.data_ptr(), b, a, c, float(np.float32(score_threshold)), boxes.data_ptr(), scores.data_ptr(),
                                     labels.data_ptr(), dirs.data_ptr(), keep.data_ptr(), _stream(dev)), "s2d_anchor_decode")
    return boxes, scores, labels, dirs, keep.bool()
