"""Makes the reference's own import paths resolve to this package, so its unmodified config files
and call sites load our implementation as a drop-in for the hot path:

    import sparse2dense_amd.det3d_shim as shim; shim.install()
    from det3d.torchie import Config                 # det3d/torchie/utils/config.py:77-100
    from det3d.models import build_detector          # det3d/models/builder.py:49
    cfg = Config.fromfile("configs/waymo/voxelnet/waymo_centerpoint_voxelnet_3x_distill_interval_5.py")
    student = build_detector(cfg.S_model, train_cfg=cfg.train_cfg, test_cfg=cfg.test_cfg)

Provided module paths (everything else of det3d is out of scope and absent on purpose):
  det3d.models{,.registry,.builder}            registries + build_* (same keys)
  det3d.ops.point_cloud.point_cloud_ops        points_to_voxel
  det3d.ops.dcn                                DeformConv, DeformConvFunction, deform_conv  (sparse2dense_amd/dcn.py; DCN v1 only)
  det3d.core.input.voxel_generator             VoxelGenerator
  det3d.core.bbox.box_np_ops                   points_in_rbbox, points_count_rbbox  (sparse2dense_amd/prep.py; numpy in, numpy out; tensor in, tensor out)
                                               center_to_corner_box2d (= prep.bev_corners)
  det3d.core.sampler.preprocess                box_collision_test  (containment collides: the reference's `is True` read by value)
  det3d.core.sampler.sample_ops                DataBaseSamplerV2 = prep.GTSampler under the reference's positional order (no group sampling, per-object
                                               rotation or random_crop; points_of replaces the point files)
  det3d.datasets.pipelines.preprocess          Preprocess = prep.S2DPreprocess (training mode; the object store and the built db_sampler are constructor arguments)
  det3d.utils.config_tool                      get_downsample_factor  (config_tool.py:39-53; imported by configs)
  det3d.builder                                build_box_coder stub   (imported by the SECOND configs), build_dbsampler = prep.build_gt_sampler
  det3d.torchie                                Config, ConfigDict
  spconv                                       SparseConvTensor, SubMConv3d, SparseConv3d, SparseSequential, SparseModule
"""
import importlib.util
import os
import sys
import types

import numpy as np


class ConfigDict(dict):
    """attribute-access dict (the reference uses addict.Dict, det3d/torchie/utils/config.py:12-33)"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(f"'ConfigDict' object has no attribute '{name}'")

    def __setattr__(self, name, value):
        self[name] = value


def _wrap(v):
    if isinstance(v, dict):
        return ConfigDict({k: _wrap(x) for k, x in v.items()})
    if isinstance(v, (list, tuple)):
        return type(v)(_wrap(x) for x in v)
    return v


class Config:
    def __init__(self, cfg_dict=None, filename=None):
        object.__setattr__(self, "_cfg_dict", _wrap(cfg_dict or {}))
        object.__setattr__(self, "_filename", filename)

    @staticmethod
    def fromfile(filename):
        filename = os.path.abspath(os.path.expanduser(filename))
        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)
        install()
        spec = importlib.util.spec_from_file_location("_s2d_cfg_" + str(abs(hash(filename))), filename)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        cfg = {k: v for k, v in mod.__dict__.items() if not k.startswith("__") and not isinstance(v, types.ModuleType)
               and not callable(v)}
        return Config(cfg, filename)

    @property
    def filename(self):
        return self._filename

    def __getattr__(self, name):
        return getattr(self._cfg_dict, name)

    def __getitem__(self, name):
        return self._cfg_dict[name]

    def __contains__(self, name):
        return name in self._cfg_dict

    def get(self, name, default=None):
        return self._cfg_dict.get(name, default)


def get_downsample_factor(model_config):
    """neck ds strides / last us stride * backbone ds_factor (det3d/utils/config_tool.py:39-53)."""
    try:
        neck_cfg = model_config["neck"]
    except Exception:
        model_config = model_config["first_stage_cfg"]
        neck_cfg = model_config["neck"]
    factor = np.prod(neck_cfg.get("ds_layer_strides", [1]))
    if len(neck_cfg.get("us_layer_strides", [])) > 0:
        factor /= neck_cfg.get("us_layer_strides", [])[-1]
    factor *= model_config["backbone"]["ds_factor"]
    factor = int(factor)
    assert factor > 0
    return factor


def _center_to_corner_box2d(centers, dims, angles=None, origin=0.5):
    """box_np_ops.center_to_corner_box2d (box_np_ops.py:265-285) for origin 0.5 = prep.bev_corners of (centre, size, yaw)"""
    from . import prep
    if origin != 0.5:
        raise NotImplementedError("center_to_corner_box2d: origin 0.5 only")
    n = len(centers)
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, 0:2], boxes[:, 3:5] = centers, dims
    if angles is not None:
        boxes[:, 6] = angles
    return prep.bev_corners(boxes)


def DataBaseSamplerV2(db_infos, groups, db_prepor=None, rate=1.0, global_rot_range=None, logger=None, points_of=None):
    """prep.GTSampler under the reference's positional constructor order (sample_ops.py:50-58); db_prepor: a callable on db_infos or the
    config's list of filter dictionaries; points_of(info) -> [P, C] replaces the point files"""
    from . import prep
    steps = () if db_prepor is None else db_prepor
    return prep.GTSampler(db_infos, groups, rate=rate, db_prep_steps=steps, points_of=points_of, global_rot_range=global_rot_range)


def _module(name, **attrs):
    m = sys.modules.get(name)
    if m is None:
        m = types.ModuleType(name)
        m.__path__ = []  # behave like a package so that dotted imports continue
        sys.modules[name] = m
        parent, _, leaf = name.rpartition(".")
        if parent:
            setattr(_module(parent), leaf, m)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


_installed = False


def install():
    """Idempotent.  Refuses to shadow a real `det3d` that is already imported."""
    global _installed
    if _installed:
        return
    if "det3d" in sys.modules and not getattr(sys.modules["det3d"], "__s2d_shim__", False):
        raise RuntimeError("a real det3d package is already imported; the shim would shadow it")
    from . import backbones, dcn, detectors, heads, necks, pillars, prep, registry, spconv, voxel_ops  # noqa: F401 (registers keys)

    _module("det3d", __s2d_shim__=True)
    reg_attrs = {k: getattr(registry, k) for k in ["READERS", "BACKBONES", "NECKS", "HEADS", "LOSSES", "DETECTORS",
                                                   "SECOND_STAGE", "ROI_HEAD"]}
    build_attrs = {k: getattr(registry, k) for k in ["build_reader", "build_backbone", "build_neck", "build_head",
                                                     "build_loss", "build_detector", "build"]}
    _module("det3d.models", **reg_attrs, **build_attrs)
    _module("det3d.models.registry", **reg_attrs)
    _module("det3d.models.builder", **build_attrs)
    _module("det3d.utils", Registry=registry.Registry, build_from_cfg=registry.build_from_cfg)
    _module("det3d.utils.registry", Registry=registry.Registry, build_from_cfg=registry.build_from_cfg)
    _module("det3d.utils.config_tool", get_downsample_factor=get_downsample_factor)
    _module("det3d.builder", build_dbsampler=prep.build_gt_sampler, build_box_coder=lambda cfg, **kw: ConfigDict(
        dict(cfg, code_size=cfg.get("n_dim", 7) + (1 if cfg.get("encode_angle_vector", False) else 0))))
    _module("det3d.torchie", Config=Config, ConfigDict=ConfigDict)
    _module("det3d.ops")
    _module("det3d.ops.point_cloud")
    _module("det3d.ops.point_cloud.point_cloud_ops", points_to_voxel=voxel_ops.points_to_voxel)
    _module("det3d.ops.dcn", DeformConv=dcn.DeformConv, DeformConvFunction=dcn.DeformConvFunction, deform_conv=dcn.deform_conv)
    _module("det3d.core")
    _module("det3d.core.input")
    _module("det3d.core.input.voxel_generator", VoxelGenerator=voxel_ops.VoxelGenerator)
    _module("det3d.core.bbox")
    _module("det3d.core.bbox.box_np_ops", points_in_rbbox=prep.points_in_rbbox, points_count_rbbox=prep.points_count_rbbox,
            center_to_corner_box2d=_center_to_corner_box2d)
    _module("det3d.core.sampler")
    _module("det3d.core.sampler.preprocess", box_collision_test=prep.box_collision_test)
    _module("det3d.core.sampler.sample_ops", DataBaseSamplerV2=DataBaseSamplerV2)
    _module("det3d.datasets")
    _module("det3d.datasets.pipelines")
    _module("det3d.datasets.pipelines.preprocess", Preprocess=prep.S2DPreprocess)
    from . import evaluation as ev
    _module("det3d.datasets.kitti")
    _module("det3d.datasets.kitti.eval", **{k: getattr(ev, k) for k in [
        "get_thresholds", "clean_data", "eval_class_v3", "get_mAP", "do_eval_v3", "do_coco_style_eval", "get_official_eval_result",
        "get_coco_eval_result"]})
    _module("det3d.datasets.utils")
    _module("det3d.datasets.utils.eval", **{k: getattr(ev, k) for k in [
        "calculate_iou_partly", "compute_statistics_jit", "prepare_data", "bev_box_overlap", "box3d_overlap", "image_box_overlap"]})
    _module("det3d.ops.nms")
    _module("det3d.ops.nms.nms_gpu", rotate_iou_gpu_eval=ev.rotate_iou_gpu_eval)
    if "spconv" not in sys.modules:
        _module("spconv", SparseConvTensor=spconv.SparseConvTensor, SubMConv3d=spconv.SubMConv3d,
                SparseConv3d=spconv.SparseConv3d, SparseSequential=spconv.SparseSequential,
                SparseModule=spconv.SparseModule)
    _installed = True
