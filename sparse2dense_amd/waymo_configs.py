"""Model dictionaries of the BASELINE.json configurations, with the same keys and values as the
reference config files (the drop-in contract is that those files load unchanged through
det3d_shim.Config.fromfile; these literals exist so that bench.py and the GPU tests do not need
/root/reference at run time):

  centerpoint_voxelnet()   configs/waymo/voxelnet/waymo_centerpoint_voxelnet_3x_distill_interval_5.py:18-46  (`model`, teacher / plain)
  s2d_student()            same file :48-76 (`S_model`)
  second_voxelnet_parts()  configs/waymo/voxelnet/waymo_second_3x_interval_5.py (reader/backbone/neck of config 1)
  second_voxelnet_train()  same file :58-106 with the full head dictionaries (:78-105); SECOND_ASSIGNER :15-55,108-113; SECOND_TEST_CFG :117-130
  two_stage_voxelnet()     configs/waymo/voxelnet/two_stage/waymo_centerpoint_voxelnet_two_stage_distill.py:19-101 (`S_model`; BASELINE configs 3, 5)
  nusc_centerpoint_dcn()   configs/nusc/voxelnet/nusc_centerpoint_voxelnet_0075voxel_dcn.py:6-13,23-55 (`model`: CenterHead with dcn_head=True)
"""
import logging

TASKS = [dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])]


def _head():
    return dict(type="CenterHead", in_channels=sum([256, 256]), tasks=TASKS, dataset="waymo", weight=2,
                code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)})


def _neck(kind):
    return dict(type=kind, layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256],
                us_layer_strides=[1, 2], us_num_filters=[256, 256], num_input_features=256,
                logger=logging.getLogger(kind))


def centerpoint_voxelnet():
    return dict(type="VoxelNet", pretrained=None,
                reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
                backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8),
                neck=_neck("RPN"), bbox_head=_head())


def s2d_student():
    return dict(type="KD_VoxelNet", pretrained=None,
                reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
                backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8),
                neck=_neck("S2D_RPN"), bbox_head=_head())


def two_stage_voxelnet():
    """the two-stage student: frozen KD_VoxelNet first stage (`pretrained` left empty: no checkpoint travels with the repository),
    five BEV sample points per box, the RoI MLP with its IoU-guided targets"""
    sampler = dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75,
                   CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55)
    loss = dict(CLS_LOSS="BinaryCrossEntropy", REG_LOSS="L1",
                LOSS_WEIGHTS={"rcnn_cls_weight": 1.0, "rcnn_reg_weight": 1.0, "code_weights": [1.0] * 7})
    return dict(type="TwoStageDetector", first_stage_cfg=s2d_student(),
                second_stage_modules=[dict(type="BEVFeatureExtractor", pc_start=[-75.2, -75.2], voxel_size=[0.1, 0.1], out_stride=8)],
                roi_head=dict(type="RoIHead", input_channels=512 * 5, code_size=7,
                              model_cfg=dict(CLASS_AGNOSTIC=True, SHARED_FC=[256, 256], CLS_FC=[256, 256], REG_FC=[256, 256], DP_RATIO=0.3,
                                             TARGET_CONFIG=sampler, LOSS_CONFIG=loss)),
                NMS_POST_MAXSIZE=500, num_point=5, freeze=True)


TWO_STAGE_TEST_CFG = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], max_per_img=4096, score_threshold=0.1, pc_range=[-75.2, -75.2],
                          out_size_factor=8, voxel_size=[0.1, 0.1],
                          nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=4096, nms_post_max_size=500,
                                   nms_iou_threshold=0.7))


def second_voxelnet():
    """configs/waymo/voxelnet/waymo_second_3x_interval_5.py:58-104 (BASELINE config 1); loss dictionaries of the
    anchor head are omitted (forward only)."""
    parts = second_voxelnet_parts()
    return dict(type="VoxelNet", pretrained=None, **parts,
                bbox_head=dict(type="MultiGroupHead", mode="3d", in_channels=sum([128, ]), tasks=TASKS, weights=[1, ],
                               box_coder=dict(type="ground_box3d_coder", n_dim=7, linear_dim=False,
                                              encode_angle_vector=False, code_size=7),
                               encode_background_as_zeros=True, use_sigmoid_score=True, encode_rad_error_by_sin=True,
                               loss_aux=dict(type="WeightedSoftmaxClassificationLoss", name="direction_classifier",
                                             loss_weight=0.2), direction_offset=0.0))


SECOND_BOX_CODER = dict(type="ground_box3d_coder", n_dim=7, linear_dim=False, encode_angle_vector=False)


def _anchor_generator(sizes, matched, unmatched, class_name):
    return dict(type="anchor_generator_range", sizes=sizes, anchor_ranges=[-74.88, -74.88, 0, 74.88, 74.88, 0], rotations=[0, 1.57],
                matched_threshold=matched, unmatched_threshold=unmatched, class_name=class_name)


# `assigner` of the config (train_cfg.assigner): what anchors.assign_anchor_targets takes
SECOND_ASSIGNER = dict(
    box_coder=SECOND_BOX_CODER,
    target_assigner=dict(type="iou",
                         anchor_generators=[_anchor_generator([2.08, 4.73, 1.77], 0.55, 0.4, "VEHICLE"),
                                            _anchor_generator([0.84, 0.91, 1.74], 0.5, 0.35, "PEDESTRIAN"),
                                            _anchor_generator([0.84, 1.81, 1.77], 0.5, 0.3, "CYCLIST")],
                         sample_positive_fraction=-1, sample_size=512,
                         region_similarity_calculator=dict(type="nearest_iou_similarity"), pos_area_threshold=-1, tasks=TASKS),
    out_size_factor=8, debug=False)

SECOND_TEST_CFG = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], max_per_img=4096,
                       nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=1000, nms_post_max_size=100,
                                nms_iou_threshold=0.01),
                       score_threshold=0.1, pc_range=[-74.88, -74.88], out_size_factor=8)


def second_voxelnet_train():
    """configs/waymo/voxelnet/waymo_second_3x_interval_5.py:58-106 with every head dictionary: the model that trains and tests"""
    parts = second_voxelnet_parts()
    return dict(type="VoxelNet", pretrained=None, **parts,
                bbox_head=dict(type="MultiGroupHead", mode="3d", in_channels=sum([128, ]), tasks=TASKS, weights=[1, ],
                               box_coder=dict(SECOND_BOX_CODER, code_size=7), encode_background_as_zeros=True,
                               loss_norm=dict(type="NormByNumPositives", pos_cls_weight=1.0, neg_cls_weight=2.0),
                               loss_cls=dict(type="SigmoidFocalLoss", alpha=0.25, gamma=2.0, loss_weight=1.0),
                               use_sigmoid_score=True,
                               loss_bbox=dict(type="WeightedSmoothL1Loss", sigma=3.0, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                                              codewise=True, loss_weight=2.0),
                               encode_rad_error_by_sin=True,
                               loss_aux=dict(type="WeightedSoftmaxClassificationLoss", name="direction_classifier", loss_weight=0.2),
                               direction_offset=0.0))


def second_voxelnet_parts():
    return dict(reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
                backbone=dict(type="SpMiddleFHD", num_input_features=5, ds_factor=8),
                neck=dict(type="RPN", layer_nums=[5], ds_layer_strides=[1], ds_num_filters=[128], us_layer_strides=[1],
                          us_num_filters=[128], num_input_features=128, logger=logging.getLogger("RPN")))


def _pp_reader():
    return dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False,
                voxel_size=(0.32, 0.32, 6.0), pc_range=(-74.88, -74.88, -2, 74.88, 74.88, 4.0))


def _pp_neck():
    return dict(type="RPN", layer_nums=[3, 5, 5], ds_layer_strides=[1, 2, 2], ds_num_filters=[64, 128, 256],
                us_layer_strides=[1, 2, 4], us_num_filters=[128, 128, 128], num_input_features=64,
                logger=logging.getLogger("RPN"))


def _pp_head():
    h = _head()
    h["in_channels"] = 128 * 3
    return h


def centerpoint_pillar():
    """configs/waymo/pp/waymo_centerpoint_pp_two_pfn_stride1_3x_distill_interval_5.py:18-51 (`model`)"""
    return dict(type="PointPillars", pretrained=None, reader=_pp_reader(),
                backbone=dict(type="PointPillarsScatter", ds_factor=1), neck=_pp_neck(), bbox_head=_pp_head())


def pillar_s2d_student():
    """same file :55-88 (`S_model`) — BASELINE config 5"""
    return dict(type="KD_PointPillars", pretrained=None, reader=_pp_reader(),
                backbone=dict(type="PointPillarsScatter_S2D", ds_factor=1), neck=_pp_neck(), bbox_head=_pp_head())


NUSC_TASKS = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["truck", "construction_vehicle"]),
              dict(num_class=2, class_names=["bus", "trailer"]), dict(num_class=1, class_names=["barrier"]),
              dict(num_class=2, class_names=["motorcycle", "bicycle"]), dict(num_class=2, class_names=["pedestrian", "traffic_cone"])]


def nusc_centerpoint_dcn():
    """configs/nusc/voxelnet/nusc_centerpoint_voxelnet_0075voxel_dcn.py:23-55 (`model`): six tasks with a velocity head, and the
    deformable feature adaption in front of every task's branches"""
    return dict(type="VoxelNet", pretrained=None,
                reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
                backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8),
                neck=_neck("RPN"),
                bbox_head=dict(type="CenterHead", in_channels=sum([256, 256]), tasks=NUSC_TASKS, dataset="nuscenes", weight=0.25,
                               code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0],
                               common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)},
                               share_conv_channel=64, dcn_head=True))
