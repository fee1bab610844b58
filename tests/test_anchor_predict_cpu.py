"""MultiGroupHead.predict on the device, the parts that need no GPU: the numpy restatement of tests/anchor_predict_ref.py pinned to the
reference's numbers (tests/golden/anchor_predict.npz), and the host logic of sparse2dense_amd/anchor_predict.py and of the head's path
choice."""
import os

import numpy as np
import pytest
import torch

import anchor_predict_ref as R
import anchor_util as AU
from sparse2dense_amd import _lib, waymo_configs as WC
from sparse2dense_amd.registry import build_head


def test_restatement_reproduces_the_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "anchor_predict.npz"))
    box, cls, dirs = AU.predict_inputs(2)
    out, segments = R.predict([dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)], [R.second_table(AU.H, AU.W)], WC.SECOND_TEST_CFG, [3])
    for i in range(2):
        idx, boxes, scores, labels, dlab = segments[0][i][0]
        assert np.array_equal(idx, g[f"cand_index_{i}"]) and np.array_equal(labels, g[f"cand_labels_{i}"])
        assert np.array_equal(dlab, g[f"cand_dir_{i}"])
        np.testing.assert_allclose(scores, g[f"cand_scores_{i}"], rtol=1e-5)
        np.testing.assert_allclose(boxes, g[f"cand_boxes_{i}"], rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(out[i]["scores"], g[f"scores_{i}"], rtol=1e-5)   # same keep set in the same order
        assert np.array_equal(out[i]["label_preds"], g[f"label_preds_{i}"]) and out[i]["label_preds"].dtype == np.int64
        np.testing.assert_allclose(out[i]["box3d_lidar"], g[f"box3d_lidar_{i}"], rtol=1e-4, atol=2e-4)


def test_small_case_has_the_properties_it_is_built_for():
    out, _ = R.check_small_case(*R.small_case())
    assert [len(o["scores"]) for o in out][2] == 0 and len(out[0]["scores"]) > 0 and len(out[1]["scores"]) > 0


def test_segment_layout_from_pass_counts():
    from sparse2dense_amd import anchor_predict as AP
    assert AP.segment_layout([24, 9, 0, 17], 16) == ([16, 9, 0, 16], [0, 16, 25, 25], 41)
    assert AP.segment_layout([24, 9, 0, 17]) == ([24, 9, 0, 17], [0, 24, 33, 33], 50)
    assert AP.segment_layout([0, 0], 1000) == ([0, 0], [0, 0], 0)
    assert AP.segment_layout([], 5) == ([], [], 0)
    assert (AP.MAX_TASKS, AP.NMS_MAX_BOXES, AP.NMS_MAX_WORKSPACE_BYTES) == (8, 65536, 256 << 20)   # the bounds of center_predict.py


def test_assembly_is_sample_major_then_task_then_keep_order():
    from sparse2dense_amd import anchor_predict as AP
    # 2 tasks x 3 samples, padded to 4 rows per segment; segment = task * samples + sample
    final = [2, 0, 1, 3, 4, 0]
    rows, sizes = AP.assembly_rows(final, tasks=2, samples=3, max_keep=4)
    assert sizes == [5, 4, 1]
    assert rows == [0, 1, 12, 13, 14,   16, 17, 18, 19,   8]
    assert AP.assembly_rows([0, 0], 1, 2, 7) == ([], [0, 0])


def _cpu_case():
    head = build_head(WC.second_voxelnet_train()["bbox_head"])
    preds = [dict(box_preds=torch.zeros(1, 1, 1, 42), cls_preds=torch.zeros(1, 1, 1, 18), dir_cls_preds=torch.zeros(1, 1, 1, 12))]
    return head, preds, dict(anchors=[torch.zeros(1, 6, 7)])


def test_device_predict_reason(monkeypatch):
    head, preds, _ = _cpu_case()
    monkeypatch.delenv("S2D_ANCHOR_DEVICE_PREDICT", raising=False)
    assert "CPU tensors" in head.device_predict_reason(preds)
    assert "more than 8 tasks" in head.device_predict_reason(preds * 9)
    monkeypatch.setenv("S2D_ANCHOR_DEVICE_PREDICT", "0")
    assert "S2D_ANCHOR_DEVICE_PREDICT=0" in head.device_predict_reason(preds)
    assert head.predict_paths == {"device": 0, "torch": 0}


def test_predict_on_cpu_tensors_raises_as_before():
    head, preds, ex = _cpu_case()
    with pytest.raises(_lib.S2DError, match="CUDA tensors expected"):
        head.predict(ex, preds, WC.SECOND_TEST_CFG)
    assert head.predict_paths == {"device": 0, "torch": 1}
    with pytest.raises(_lib.S2DError, match="CUDA tensors expected"):
        head.predict_torch(ex, preds, WC.SECOND_TEST_CFG)
    from sparse2dense_amd import anchor_predict as AP
    with pytest.raises(_lib.S2DError, match="CUDA tensors expected"):
        AP.decode_anchor_candidates(preds, [torch.zeros(6, 7)], WC.SECOND_TEST_CFG)


def test_c_abi_argument_validation():
    """error codes without a device: every entry checks its arguments before it launches"""
    from sparse2dense_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    one = 8   # a non-null pointer value that is never dereferenced
    t = (_lib.AnchorPredictTask * 1)()
    t[0].box_preds = t[0].cls_preds = t[0].anchors = one
    t[0].num_anchors, t[0].classes = 6, 3
    assert lib.s2d_anchor_predict_score(None, 1, 1, 6, 0.1, one, one, one, None) == -1 and "null task table" in _lib.last_error()
    assert lib.s2d_anchor_predict_score(t, 9, 1, 6, 0.1, one, one, one, None) == -1 and "tasks" in _lib.last_error()
    assert lib.s2d_anchor_predict_score(t, 1, 1, 5, 0.1, one, one, one, None) == -1 and "anchors" in _lib.last_error()
    assert lib.s2d_anchor_predict_score(t, 1, 1, 6, 0.1, one, one, None, None) == -1 and "null count" in _lib.last_error()
    assert lib.s2d_anchor_predict_score(t, 1, 1, 6, 0.1, None, one, one, None) == -1 and "null output" in _lib.last_error()
    t[0].classes = 0
    assert lib.s2d_anchor_predict_score(t, 1, 1, 6, 0.1, one, one, one, None) == -1 and "classes" in _lib.last_error()
    t[0].classes = 3
    boxes = lambda *a: lib.s2d_anchor_predict_boxes(t, 1, 1, 6, None, *a, None)   # noqa: E731
    assert boxes(one, one, one, one, one, -1, 4, one, one, one, one, one) == -1 and "negative size" in _lib.last_error()
    assert boxes(None, one, one, one, one, 4, 4, one, one, one, one, one) == -1 and "null input" in _lib.last_error()
    assert boxes(one, one, one, one, one, 4, 4, one, one, one, one, None) == -1 and "null output" in _lib.last_error()
    assert boxes(None, None, None, None, None, 0, 0, None, None, None, None, None) == 0   # nothing to decode: no launch
    fin = lambda tasks, nt, *a: lib.s2d_anchor_predict_finish(tasks, nt, 1, *a, None)   # noqa: E731
    args = [one] * 7 + [4, one, one, 4, 1, 0.0, one, one, one, one]
    assert fin(None, 1, *args) == -1 and "null task table" in _lib.last_error()
    assert fin(t, 0, *args) == -1 and "tasks" in _lib.last_error()
    bad = list(args)
    bad[9] = None   # n_keep
    assert fin(t, 1, *bad) == -1 and "null segment arrays" in _lib.last_error()
    bad = list(args)
    bad[0] = None   # boxes
    assert fin(t, 1, *bad) == -1 and "null input" in _lib.last_error()
    bad = list(args)
    bad[13] = None   # out_boxes
    assert fin(t, 1, *bad) == -1 and "null output" in _lib.last_error()
