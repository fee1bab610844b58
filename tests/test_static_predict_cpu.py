"""Host side of the static predict path (center_predict.StaticPredictPlan, CenterHead.predict_static): what it refuses - before any HIP
call, so all of it runs without a GPU - the padded result struct, and the C boundary of its two entries."""
import os
import re
import sys

import pytest
import torch

from sparse2dense_amd import _lib, center_predict

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import predict_tasks_util as U   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(U.CFG, double_flip=False, circular_nms=False, min_radius=[4, 12, 10, 1, 0.85, 0.175, 1, 1, 1])


def _maps(tasks=2, vel=True, h=6, w=5):
    return [U.seeded_task_maps(1, 10 + i, h, w, 2, False, vel=vel) for i in range(tasks)]


def _head(tasks=2, vel=True):
    from sparse2dense_amd.heads import CenterHead
    heads = {k: v for k, v in U.COMMON_HEADS.items() if vel or k != "vel"}
    table = [dict(num_class=1, class_names=[f"c{i}"]) for i in range(tasks)]
    return CenterHead(in_channels=64, tasks=table, dataset="nuscenes", weight=0.25, code_weights=[1.0] * (10 if vel else 8), common_heads=heads).eval()


@pytest.fixture
def no_hip(monkeypatch):
    """a refusal must come before the library is even loaded"""
    def load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", load)


def test_the_plan_refuses_k_above_4096_and_more_than_8_tasks_and_a_cpu_device(no_hip):
    build = lambda cfg=CFG, classes=(1, 1), device="cuda", **kw: center_predict.StaticPredictPlan(cfg, list(classes), 2, 6, 5, True, device, **kw)
    with pytest.raises(_lib.S2DError, match="4097 candidates per segment"):
        build(dict(CFG, nms=dict(CFG["nms"], nms_pre_max_size=4097)))
    with pytest.raises(_lib.S2DError, match="5000 candidates per segment"):
        build(dict(CFG, circular_nms=True), max_candidates=5000)
    with pytest.raises(_lib.S2DError, match="0 candidates per segment"):
        build(dict(CFG, circular_nms=True), max_candidates=0)
    with pytest.raises(_lib.S2DError, match="9 tasks"):
        build(classes=[1] * 9)
    with pytest.raises(_lib.S2DError, match="CUDA device expected"):
        build(device="cpu")


def test_predict_static_refuses_maps_it_would_have_to_copy_or_widen(no_hip):
    head = _head()
    with pytest.raises(_lib.S2DError, match="CUDA tensors expected"):
        head.predict_static({}, _maps(), CFG)
    bf16 = _maps()
    bf16[1]["dim"] = bf16[1]["dim"].bfloat16()
    with pytest.raises(_lib.S2DError, match="map 'dim' is torch.bfloat16: fp32 maps only"):
        head.predict_static({}, bf16, CFG)
    strided = _maps()
    strided[0]["rot"] = strided[0]["rot"].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)   # W-major: neither layout
    assert strided[0]["rot"].shape == bf16[0]["rot"].shape
    with pytest.raises(_lib.S2DError, match="map 'rot' is neither NCHW-contiguous nor channels_last"):
        head.predict_static({}, strided, CFG)
    partial = _maps()
    del partial[1]["vel"]
    with pytest.raises(_lib.S2DError, match="velocity branch on some tasks only"):
        head.predict_static({}, partial, CFG)
    with pytest.raises(_lib.S2DError, match="9 tasks"):
        _head(9).predict_static({}, _maps(9), CFG)
    assert head.static_predict_calls == 0 and head.predict_paths == {"device": 0, "torch": 0} and head._static_plans == {}


def test_plan_keys_tell_apart_what_a_plan_depends_on():
    key = lambda cfg=CFG, classes=(1, 1), images=2, h=6, w=5, vel=True, dev="cuda:0", m=4096: center_predict.static_plan_key(cfg, classes, images, h, w, vel, dev, m)
    base = key()
    assert base == key(dict(CFG)) and hash(base) == hash(key())
    others = [key(dict(CFG, score_threshold=0.2)), key(dict(CFG, double_flip=True)), key(dict(CFG, circular_nms=True)), key(classes=(1, 2)),
              key(images=4), key(h=7), key(w=6), key(vel=False), key(dev="cuda:1"), key(m=100),
              key(dict(CFG, nms=dict(CFG["nms"], nms_post_max_size=10))), key(dict(CFG, post_center_limit_range=[]))]
    assert len({base, *others}) == len(others) + 1
    # the radii count under the circle NMS only
    assert key(dict(CFG, min_radius=[1, 1])) == base
    assert key(dict(CFG, circular_nms=True, min_radius=[1, 1])) != key(dict(CFG, circular_nms=True))


def test_as_list_cuts_the_padding():
    boxes = torch.arange(2 * 4 * 7, dtype=torch.float32).reshape(2, 4, 7)
    scores = torch.tensor([[0.9, 0.8, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    labels = torch.tensor([[3, 1, -1, -1], [-1, -1, -1, -1]])
    det = center_predict.StaticDetections(boxes, scores, labels, torch.tensor([2, 0], dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    assert [t is u for t, u in zip(det, (boxes, scores, labels, det.counts, det.overflow))] == [True] * 5
    out = det.as_list()
    assert [sorted(d) for d in out] == [["box3d_lidar", "label_preds", "metadata", "scores"]] * 2
    assert torch.equal(out[0]["box3d_lidar"], boxes[0, :2]) and out[0]["scores"].tolist() == pytest.approx([0.9, 0.8]) and out[0]["label_preds"].tolist() == [3, 1]
    assert out[1]["box3d_lidar"].shape == (0, 7) and out[1]["scores"].shape == (0,) and out[1]["label_preds"].dtype == torch.int64
    assert [d["metadata"] for d in out] == [None, None]
    assert [d["metadata"] for d in det.as_list(["a", "b"])] == ["a", "b"]


def test_header_and_binding_agree_on_the_two_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s2d.h")).read(), flags=re.S)
    for name in ("s2d_segment_topk", "s2d_predict_static_gather"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.ctypes.c_int and len(params) == len(argtypes), (name, len(params), len(argtypes))
        for p, a in zip(params, argtypes):
            if "*" in p or p.startswith("s2d_stream_t"):
                assert a is _lib.ctypes.c_void_p, (name, p)
            else:
                assert a is (_lib.ctypes.c_int64 if p.startswith("int64_t") else _lib.ctypes.c_int), (name, p)
    assert not [n for n in ("s2d_segment_topk_workspace_bytes", "s2d_predict_static_workspace_bytes") if n in _lib.SIGNATURES]


def test_the_entries_refuse_bad_sizes_without_a_device():
    from sparse2dense_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    topk = lambda segs=2, row_len=100, stride=100, k=10, out_stride=10: lib.s2d_segment_topk(None, segs, row_len, stride, k, None, None, None, out_stride,
                                                                                           None, None, None, None)
    for bad, word in ((dict(k=0), "k 0"), (dict(k=4097), "k 4097"), (dict(row_len=101), "row_stride"), (dict(out_stride=9), "out_stride"),
                      (dict(row_len=(1 << 20) + 1, stride=1 << 21), "row_len"), (dict(segs=-1), "segments"), ({}, "null argument")):
        assert topk(**bad) == -1 and word in _lib.last_error(), (bad, _lib.last_error())
    assert topk(segs=0) == 0
    gather = lambda tasks=2, samples=2, max_keep=4, box_dim=9: lib.s2d_predict_static_gather(None, None, None, None, None, None, tasks, samples, max_keep,
                                                                                             box_dim, 16, None, None, None, None, None)
    for bad, word in ((dict(tasks=9), "9 tasks"), (dict(box_dim=8), "box_dim 8"), (dict(max_keep=-1), "bad size"), ({}, "null")):
        assert gather(**bad) == -1 and word in _lib.last_error(), (bad, _lib.last_error())
    assert gather(samples=0) == 0
