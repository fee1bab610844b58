"""Host side of the static second stage (second_stage.StaticRoIPlan, s2d_roi_pack_static, s2d_roi_refine_static): what the plan refuses,
before any HIP call, so all of it runs without a GPU; the C boundary of the two new entries; and the pack and clamp rule restated in numpy
(roi_static_util.pack_static_host, which the GPU tests use as the expectation for `row` and `out_counts`) against the contract written
in include/s2d.h, case by case."""
import os
import re

import numpy as np
import pytest
import torch

from roi_static_util import clamp_counts, pack_static_host, trapped_rows
from sparse2dense_amd import _lib, center_predict, second_stage as S
from test_roi_mlp_cpu import make_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = dict(pc_start=[-6.4, -6.4], voxel_size=[0.1, 0.1], out_stride=8)


@pytest.fixture
def no_hip(monkeypatch):
    """a refusal must come before the library is even loaded"""
    def load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", load)
    monkeypatch.delenv("S2D_ROI_MLP", raising=False)


def _plan(head=None, modules=None, num_point=5, samples=2, det_cap=16, cap=16, channels=16, dtype=torch.float32, device="cuda"):
    head = make_head(num_point * channels if num_point in (1, 5) else 80, (32, 16), (16,), (32, 16)) if head is None else head
    modules = [S.BEVFeatureExtractor(**EXT)] if modules is None else modules
    return S.StaticRoIPlan(head, modules, num_point, samples, det_cap, cap, channels, dtype, device)


def test_the_plan_refuses_before_any_hip_call(no_hip):
    with pytest.raises(_lib.S2DError, match="CUDA device expected"):
        _plan(device="cpu")
    with pytest.raises(_lib.S2DError, match="65 samples"):
        _plan(samples=65)
    with pytest.raises(_lib.S2DError, match="0 samples"):
        _plan(samples=0)
    with pytest.raises(_lib.S2DError, match="det_cap 0"):
        _plan(det_cap=0)
    with pytest.raises(_lib.S2DError, match="num_point 3"):
        _plan(num_point=3)
    with pytest.raises(_lib.S2DError, match="code_size 9"):
        _plan(head=make_head(80, (32,), (16,), (16,), code_size=9))
    two_classes = make_head(80, (32,), (16,), (16,))
    two_classes.num_class = 2
    with pytest.raises(_lib.S2DError, match="num_class 2"):
        _plan(head=two_classes)
    with pytest.raises(_lib.S2DError, match="other than one BEVFeatureExtractor"):
        _plan(modules=[S.BEVFeatureExtractor(**EXT), S.BEVFeatureExtractor(**EXT)])
    with pytest.raises(_lib.S2DError, match="other than one BEVFeatureExtractor"):
        _plan(modules=[torch.nn.Identity()])
    with pytest.raises(_lib.S2DError, match="other than one BEVFeatureExtractor"):
        _plan(modules=[])
    with pytest.raises(_lib.S2DError, match="torch.float16"):
        _plan(dtype=torch.float16)
    # a head for which mlp_reason is not None
    with pytest.raises(_lib.S2DError, match="training mode"):
        _plan(head=make_head(80, (32, 16), (16,), (32, 16)).train())
    with pytest.raises(_lib.S2DError, match="width 200"):
        _plan(head=make_head(80, (32, 200), (16,), (16,)))
    with pytest.raises(_lib.S2DError, match="3 shared layers"):
        _plan(head=make_head(80, (32, 32, 32), (16,), (16,)))
    with pytest.raises(_lib.S2DError, match="40 feature channels for a head of 80"):
        _plan(channels=8, head=make_head(80, (32,), (16,), (16,)))
    # (a head that needs a gradient is refused as well; without a GPU its parameters cannot lie on the plan's device, and that reason
    # is the one `_mlp_check_for` meets first - the GPU tests see "a gradient is required")
    with torch.enable_grad(), pytest.raises(_lib.S2DError, match="another device|gradient"):
        _plan()


def _host_plan(samples=2, det_cap=16, channels=16, dtype=torch.float32):
    """the attributes `StaticRoIPlan._check` reads, on the CPU: what `run` refuses on the host comes before its first HIP call"""
    plan = object.__new__(S.StaticRoIPlan)
    plan.samples, plan.det_cap, plan.cap, plan.channels, plan.map_dtype, plan.device = samples, det_cap, 16, channels, dtype, torch.device("cpu")
    plan.cin, plan.head = 5 * channels, make_head(5 * channels, (32, 16), (16,), (32, 16))
    return plan


def _det(samples=2, det_cap=16, dim=7):
    return center_predict.StaticDetections(torch.zeros(samples, det_cap, dim), torch.zeros(samples, det_cap), torch.zeros(samples, det_cap, dtype=torch.int64),
                                           torch.zeros(samples, dtype=torch.int32), torch.zeros(samples, dtype=torch.int32))


def test_run_refuses_on_the_host_before_any_hip_call(no_hip):
    plan, bev = _host_plan(), torch.zeros(2, 16, 16, 16)
    with pytest.raises(_lib.S2DError, match="7-column"):
        plan.run(_det(dim=9), bev)
    with pytest.raises(_lib.S2DError, match="built for"):
        plan.run(_det(samples=3), bev)
    with pytest.raises(_lib.S2DError, match="built for"):
        plan.run(_det(det_cap=17), bev)
    d = _det()
    d.labels = d.labels.int()
    with pytest.raises(_lib.S2DError, match="labels is torch.int32"):
        plan.run(d, bev)
    d = _det()
    d.counts = d.counts.long()
    with pytest.raises(_lib.S2DError, match="counts is torch.int64"):
        plan.run(d, bev)
    d = _det()
    d.boxes = torch.zeros(2, 7, 16).permute(0, 2, 1)
    with pytest.raises(_lib.S2DError, match="not contiguous"):
        plan.run(d, bev)
    with pytest.raises(_lib.S2DError, match="torch.bfloat16"):     # a map of another dtype
        plan.run(_det(), bev.to(torch.bfloat16))
    with pytest.raises(_lib.S2DError, match=r"\[2, 16, H, W\]"):   # ... channel count
        plan.run(_det(), torch.zeros(2, 24, 16, 16))
    with pytest.raises(_lib.S2DError, match=r"\[2, 16, H, W\]"):   # ... batch
        plan.run(_det(), torch.zeros(3, 16, 16, 16))
    with pytest.raises(_lib.S2DError, match="not a"):
        plan.run(_det(), torch.zeros(2, 16, 16))
    with pytest.raises(_lib.S2DError, match="training mode"):      # the head changed its mode behind the plan
        plan.head.train()
        plan.run(_det(), bev)


def test_forward_static_refuses_cpu_maps_before_any_hip_call(no_hip):
    from roi_static_util import FixedMapsFirstStage
    from sparse2dense_amd import registry
    head_cfg = dict(type="CenterHead", in_channels=16, tasks=[dict(num_class=3, class_names=["a", "b", "c"])], dataset="waymo", weight=2,
                    code_weights=[1.0] * 8, common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2)})
    det = registry.build_detector(dict(type="TwoStageDetector", first_stage_cfg=dict(type=FixedMapsFirstStage, bbox_head=head_cfg), NMS_POST_MAXSIZE=16,
                                       num_point=5, second_stage_modules=[dict(type="BEVFeatureExtractor", **EXT)],
                                       roi_head=dict(type="RoIHead", input_channels=80, code_size=7,
                                                     model_cfg=dict(CLASS_AGNOSTIC=True, SHARED_FC=[32, 16], CLS_FC=[16], REG_FC=[32, 16], DP_RATIO=0.3)))).eval()
    det.single_det.maps = [dict(hm=torch.zeros(1, 3, 16, 16), reg=torch.zeros(1, 2, 16, 16), height=torch.zeros(1, 1, 16, 16),
                                dim=torch.zeros(1, 3, 16, 16), rot=torch.zeros(1, 2, 16, 16))]
    det.single_det.bev = torch.zeros(1, 16, 16, 16)
    with pytest.raises(_lib.S2DError, match="CUDA tensors expected"):
        det.forward_static({})
    assert det.static_calls == 0 and det.roi_paths == {"device": 0, "torch": 0} and det._static_roi_plans == {}


def test_header_and_binding_agree_on_the_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s2d.h")).read(), flags=re.S)
    for name, count in (("s2d_roi_pack_static", 13), ("s2d_roi_refine_static", 12)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.ctypes.c_int and len(params) == len(argtypes) == count, name
        for p, a in zip(params, argtypes):
            assert a is (_lib.ctypes.c_void_p if "*" in p or p.startswith("s2d_stream_t") else _lib.ctypes.c_int), (name, p)
    assert S.STATIC_ROI_LAUNCHES == 4 and S.ROI_MAX_BATCH == 64 and re.search(r"#define\s+S2D_ROI_MAX_BATCH\s+64\b", src)


def test_the_entries_refuse_bad_arguments_without_a_device():
    """the library loads without a GPU; every refusal comes before any HIP call and names its argument"""
    from sparse2dense_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    keep = np.zeros(64, np.uint8)   # any non-null address: a refused call never reads it
    p = keep.ctypes.data

    def pack(batch=2, det_cap=16, cap=16, null=None):
        ptrs = dict.fromkeys(("boxes", "scores", "labels", "counts", "rois", "roi_scores", "roi_labels", "row", "out_counts"), p)
        if null:
            ptrs[null] = None
        return lib.s2d_roi_pack_static(ptrs["boxes"], ptrs["scores"], ptrs["labels"], ptrs["counts"], batch, det_cap, cap, ptrs["rois"], ptrs["roi_scores"],
                                       ptrs["roi_labels"], ptrs["row"], ptrs["out_counts"], None)

    def refine(batch=2, cap=16, null=None):
        ptrs = dict.fromkeys(("rois", "roi_scores", "roi_labels", "cls", "reg", "counts", "boxes", "scores", "labels"), p)
        if null:
            ptrs[null] = None
        return lib.s2d_roi_refine_static(ptrs["rois"], ptrs["roi_scores"], ptrs["roi_labels"], ptrs["cls"], ptrs["reg"], ptrs["counts"], batch, cap,
                                         ptrs["boxes"], ptrs["scores"], ptrs["labels"], None)
    for call, bad, word in [(pack, dict(batch=65), "batch 65"), (pack, dict(batch=0), "batch 0"), (pack, dict(det_cap=0), "det_cap 0"),
                            (pack, dict(cap=0), "cap 0"), (pack, dict(batch=64, det_cap=2 ** 25), "detection rows"),
                            (pack, dict(null="counts"), "null boxes, scores, labels or counts"), (pack, dict(null="boxes"), "null boxes"),
                            (pack, dict(null="row"), "null output"), (pack, dict(null="out_counts"), "null output"),
                            (refine, dict(batch=0), "batch 0"), (refine, dict(cap=0), "cap 0"), (refine, dict(null="counts"), "null input"),
                            (refine, dict(null="reg"), "null input"), (refine, dict(null="labels"), "null output")]:
        assert call(**bad) == -1 and word in _lib.last_error(), (bad, _lib.last_error())


# ---- the pack and clamp rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det_cap,cap", [(8, 16), (16, 16), (24, 16)])
def test_the_numpy_restatement_follows_the_documented_contract(det_cap, cap):
    """n_b = clamp(counts[b], 0, min(det_cap, cap)) for counts 0, 1, cap, above cap, above det_cap and negative; slots < n_b copied with
    label + 1 and row = b * det_cap + slot; slots >= n_b zero, label 0, row -1; nothing behind counts[b] is read (the traps are NaN)"""
    counts = [0, 1, cap, cap + 3, det_cap + 5, -2]
    lim = min(det_cap, cap)
    want = [0, 1, lim, lim, lim, 0]
    assert clamp_counts(counts, det_cap, cap).tolist() == want
    boxes, scores, labels = [t.numpy() for t in trapped_rows(6, det_cap, counts, 7)]
    rois, roi_scores, roi_labels, row, n = pack_static_host(boxes, scores, labels, counts, cap)
    assert n.dtype == np.int32 and row.dtype == np.int32 and roi_labels.dtype == np.int64 and rois.shape == (6, cap, 7) and n.tolist() == want
    assert not np.isnan(rois).any()   # no trap row was copied
    for b, k in enumerate(want):
        assert np.array_equal(rois[b, :k], boxes[b, :k]) and np.array_equal(roi_scores[b, :k], scores[b, :k])
        assert np.array_equal(roi_labels[b, :k], labels[b, :k] + 1) and (roi_labels[b, :k] >= 1).all()
        assert row[b, :k].tolist() == list(range(b * det_cap, b * det_cap + k))
        assert not rois[b, k:].any() and not roi_scores[b, k:].any() and not roi_labels[b, k:].any() and (row[b, k:] == -1).all()
    # the row table indexes the boxes viewed as [B * det_cap, 7]
    flat = boxes.reshape(-1, 7)
    assert np.array_equal(flat[row[row >= 0]], rois[row >= 0])
