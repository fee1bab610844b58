"""CPU side of the device two-stage RoI path: the host restatement of the RoI sampling against the torch one under equal seeds, the
argument validation of the new C entries (no GPU, no launch), and the two-stage model dictionary."""
import os

import numpy as np
import pytest
import torch

from sparse2dense_amd import _lib, build, registry, second_stage as S
from test_second_stage import ROI_TRAIN_CFG


def _layer(**over):
    return S.ProposalTargetLayer(dict(ROI_TRAIN_CFG["TARGET_CONFIG"], **over))


def _both(layer, overlaps, seed):
    """(torch indices, host indices, states equal) with both samplers started from the same numpy / torch generator states"""
    np.random.seed(seed); torch.manual_seed(seed)
    ref = layer.subsample_rois(torch.from_numpy(overlaps)).numpy()
    ref_state = (np.random.get_state(), torch.get_rng_state())
    np.random.seed(seed); torch.manual_seed(seed)
    got = layer.subsample_rois_host(overlaps)
    now = (np.random.get_state(), torch.get_rng_state())
    same = (ref_state[0][0] == now[0][0] and np.array_equal(ref_state[0][1], now[0][1]) and ref_state[0][2:] == now[0][2:]
            and torch.equal(ref_state[1], now[1]))
    return ref, got, same


def _fixture_overlaps(golden_dir):
    """max_overlaps of both fixture samples, as the CPU reference test computes them (CPU oracle for the rotated BEV IoU)"""
    from oracle import iou_nms as OI
    g = np.load(os.path.join(golden_dir, "roi_training.npz"))
    layer = S.ProposalTargetLayer(ROI_TRAIN_CFG["TARGET_CONFIG"],
                                  iou_fn=lambda a, b: S.boxes_iou3d(a, b, bev_iou=lambda x, y: torch.from_numpy(OI.bev_iou(x.numpy(), y.numpy()))))
    out = []
    for i in range(2):
        gt = torch.from_numpy(g["gt"][i])
        k = max(int(np.nonzero(g["gt"][i].sum(-1))[0].max()), 0)
        gt = gt[:k + 1]
        mo, _ = layer.get_max_iou_with_same_class(torch.from_numpy(g["rois"][i]), torch.from_numpy(g["roi_labels"][i]), gt[:, :7], gt[:, -1].long())
        out.append(mo.numpy())
    return out


def test_host_sampling_draws_what_the_torch_sampling_draws_on_the_fixture(golden_dir):
    layer = _layer()
    for i, mo in enumerate(_fixture_overlaps(golden_dir)):
        assert (mo >= 0.55).any() and (mo < 0.1).any() and ((mo < 0.55) & (mo >= 0.1)).any(), i   # all three groups are present
        ref, got, same = _both(layer, mo, 11 + i)
        assert got.dtype == np.int64 and got.shape == (32,) and np.array_equal(ref, got) and same, i


@pytest.mark.parametrize("name,overlaps,over", [
    ("fg_only", np.linspace(0.6, 0.9, 9, dtype=np.float32), {}),
    ("bg_only", np.array([0.0, 0.05, 0.2, 0.3, 0.5, 0.54], np.float32), {}),
    ("hard_only", np.linspace(0.1, 0.5, 7, dtype=np.float32), {}),
    ("easy_only", np.linspace(0.0, 0.09, 5, dtype=np.float32), {}),
    ("fg_and_both_bg", np.array([0.9, 0.0, 0.3, 0.7, 0.05, 0.2, 0.56, 0.1, 0.55], np.float32), {}),
    ("fg_and_hard", np.array([0.9, 0.3, 0.7, 0.2, 0.56], np.float32), {}),
    ("fg_and_easy", np.array([0.9, 0.01, 0.7, 0.02, 0.56], np.float32), {}),
    ("more_fg_than_fg_per", np.concatenate([np.linspace(0.56, 0.99, 40), np.linspace(0.0, 0.5, 11)]).astype(np.float32), {}),
    ("no_hard_share", np.array([0.9, 0.0, 0.3, 0.7], np.float32), dict(HARD_BG_RATIO=0.0)),
])
def test_host_sampling_draws_what_the_torch_sampling_draws(name, overlaps, over):
    layer = _layer(**over)
    for seed in (0, 3):
        ref, got, same = _both(layer, overlaps, seed)
        assert np.array_equal(ref, got), (name, seed, ref, got)
        assert same, (name, seed)   # the generators stand where the torch sampling leaves them
        assert len(got) == 32


def test_host_sampling_with_nothing_to_sample_raises_as_the_torch_sampling_does():
    layer = _layer()
    with pytest.raises(NotImplementedError):
        layer.subsample_rois_host(np.full((4,), np.nan, np.float32))


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()   # loads without a GPU


P = 0x1000   # a non-null stand-in; every call below must fail before any HIP call


def _rejected(rc, text):
    assert rc != 0 and text in _lib.last_error(), (rc, text, _lib.last_error())


def test_feature_entry_validates_its_arguments(lib):
    def feats(map_=P, dtype=1, batch=2, c=8, h=4, w=4, strides=(128, 1, 32, 8), boxes=P, total=5, box_dim=7, row=P, cap=3, num_point=5, out=P):
        return lib.s2d_roi_bev_features(map_, dtype, batch, c, h, w, *strides, boxes, total, box_dim, row, cap, num_point, -75.2, -75.2, 0.1, 0.1, 8.0,
                                        out, None)
    for kw, text in [(dict(map_=None), "null argument"), (dict(row=None), "null argument"), (dict(out=None), "null argument"),
                     (dict(boxes=None), "null box list"), (dict(num_point=3), "num_point 3"), (dict(num_point=0), "num_point 0"),
                     (dict(dtype=2), "map dtype 2"), (dict(batch=-1), "negative size"), (dict(cap=-1), "negative size"), (dict(total=-1), "negative size"),
                     (dict(c=0), "empty map"), (dict(h=0), "empty map"), (dict(strides=(128, 1, -32, 8)), "negative stride"),
                     (dict(box_dim=6), "box_dim 6"), (dict(total=1 << 31), "int32 row table")]:
        _rejected(feats(**kw), text)
    assert feats(batch=0, map_=None, row=None, out=None) == 0 and feats(cap=0, map_=None) == 0   # nothing to do: no launch, no error


def test_pack_entry_validates_its_arguments(lib):
    import ctypes
    off = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def pack(boxes=P, scores=P, labels=P, box_dim=7, offsets=off(0, 2, 5), batch=2, cap=4, rois=P, roi_scores=P, roi_labels=P):
        return lib.s2d_roi_pack(boxes, scores, labels, box_dim, offsets, batch, cap, rois, roi_scores, roi_labels, None)
    for kw, text in [(dict(offsets=None), "null argument"), (dict(rois=None), "null argument"), (dict(roi_labels=None), "null argument"),
                     (dict(boxes=None), "null box list"), (dict(labels=None), "null box list"), (dict(box_dim=5), "box_dim 5"),
                     (dict(batch=65, offsets=off(*range(66))), "batch 65"), (dict(batch=-1), "batch -1"), (dict(cap=-2), "cap -2"),
                     (dict(offsets=off(0, 3, 2)), "must not decrease"), (dict(offsets=off(-1, 3, 4)), "must not decrease")]:
        _rejected(pack(**kw), text)
    assert pack(batch=0, offsets=None) == 0 and pack(cap=0, rois=None) == 0


def test_match_entry_validates_its_arguments(lib):
    def match(rois=P, labels=P, batch=2, cap=60, gt=P, num_gt=20, gt_dim=8, out=(P, P, P)):
        return lib.s2d_roi_match_gt(rois, labels, batch, cap, gt, num_gt, gt_dim, 1, *out, None)
    assert S.ROI_MAX_GT == 512
    for kw, text in [(dict(rois=None), "null argument"), (dict(labels=None), "null argument"), (dict(out=(None, P, P)), "null argument"),
                     (dict(out=(P, None, P)), "null argument"), (dict(out=(P, P, None)), "null ground truth or count"),
                     (dict(gt=None), "null ground truth or count"), (dict(num_gt=S.ROI_MAX_GT + 1), "513 ground-truth rows per sample (1..512 supported)"),
                     (dict(num_gt=0), "0 ground-truth rows"), (dict(gt_dim=7), "gt_dim 7"), (dict(batch=-1), "batch -1"), (dict(batch=65536), "batch 65536"),
                     (dict(cap=-1), "cap -1")]:
        _rejected(match(**kw), text)
    assert match(batch=0, gt=None) == 0


def test_targets_entry_validates_its_arguments(lib):
    def targets(idx=P, batch=2, per=32, cap=60, roi_dim=7, ins=(P,) * 6, num_gt=20, gt_dim=8, kind=1, outs=(P,) * 8):
        return lib.s2d_roi_targets(idx, batch, per, cap, roi_dim, *ins, num_gt, gt_dim, 0.55, 0.75, 0.25, kind, *outs, None)
    for kw, text in [(dict(roi_dim=9), "roi_dim 9 (code size 7 only)"), (dict(idx=None), "null input"), (dict(kind=2), "cls_score_type 2"),
                     (dict(batch=-1), "negative size"), (dict(per=-1), "negative size"), (dict(cap=0), "cap 0"), (dict(num_gt=0), "0 ground-truth rows"),
                     (dict(gt_dim=7), "gt_dim 7")]:
        _rejected(targets(**kw), text)
    for k in range(6):
        _rejected(targets(ins=tuple(None if i == k else P for i in range(6))), "null input")
    for k in range(8):
        _rejected(targets(outs=tuple(None if i == k else P for i in range(8))), "null output")
    assert targets(per=0, idx=None) == 0


def test_refine_entry_validates_its_arguments(lib):
    def refine(ins=(P,) * 5, n=100, outs=(P,) * 3):
        return lib.s2d_roi_refine(*ins, n, *outs, None)
    for k in range(5):
        _rejected(refine(ins=tuple(None if i == k else P for i in range(5))), "null input")
    for k in range(3):
        _rejected(refine(outs=tuple(None if i == k else P for i in range(3))), "null output")
    _rejected(refine(n=-1), "-1 RoIs")
    assert refine(n=0, ins=(None,) * 5) == 0


def test_host_api_fails_loudly_on_cpu_tensors():
    z = torch.zeros
    with pytest.raises(_lib.S2DError):
        S.pack_rois(z(3, 7), z(3), z(3, dtype=torch.long), [0, 3], 4)
    with pytest.raises(_lib.S2DError):
        S.roi_bev_features(z(1, 8, 4, 4), z(3, 7), z(1, 3, dtype=torch.int32), [-75.2, -75.2], [0.1, 0.1], 8)
    with pytest.raises(_lib.S2DError):
        S.match_rois_to_gt(z(1, 4, 7), z(1, 4, dtype=torch.long), z(1, 2, 8))
    with pytest.raises(_lib.S2DError):
        S.roi_targets(z(1, 2, dtype=torch.int32), z(1, 4, 7), z(1, 4, dtype=torch.long), z(1, 4), z(1, 4), z(1, 4, dtype=torch.long), z(1, 2, 8),
                      ROI_TRAIN_CFG["TARGET_CONFIG"])
    with pytest.raises(_lib.S2DError):
        S.refine_rois(z(1, 4, 7), z(1, 4), z(1, 4, dtype=torch.long), z(4, 1), z(4, 7))


def test_two_stage_model_dictionary_builds_through_the_registry():
    from sparse2dense_amd import waymo_configs
    cfg = waymo_configs.two_stage_voxelnet()
    assert cfg["NMS_POST_MAXSIZE"] == 500 and cfg["num_point"] == 5 and cfg["freeze"] and cfg["roi_head"]["input_channels"] == 2560
    assert cfg["roi_head"]["model_cfg"]["TARGET_CONFIG"]["ROI_PER_IMAGE"] == 128
    det = registry.build_detector(cfg)
    sd = det.state_dict()
    keys = list(sd)
    # `single_det.` / `roi_head.`, plus the reference's alias `bbox_head` = `single_det.bbox_head` (two_stage.py:29: the same tensors twice)
    alias = [k for k in keys if k.startswith("bbox_head.")]
    assert all(sd[k].data_ptr() == sd["single_det." + k].data_ptr() for k in alias)
    assert keys and all(k.startswith(("single_det.", "roi_head.")) for k in keys if k not in alias)
    assert any(k.startswith("single_det.") for k in keys) and "roi_head.shared_fc_layer.0.weight" in keys
    assert det.roi_paths == {"device": 0, "torch": 0} and det.roi_head.proposal_target_layer is not None
    assert all(not p.requires_grad for p in det.single_det.parameters()) and all(p.requires_grad for p in det.roi_head.parameters())
    # CPU maps take the torch chain
    assert "CUDA" in det.device_path_reason([dict(box3d_lidar=torch.zeros(0, 7))], torch.zeros(1, 512, 4, 4), {}, False)
