"""MultiGroupHead.predict on the device (csrc/anchor_predict.hip, anchor_predict.py, nms.rotate_nms_batched) against the reference's numbers
(tests/golden/anchor_predict.npz), against the per-segment chain it replaces (MultiGroupHead.predict_torch: the same kept anchors in the
same order, scores, labels AND boxes bit for bit - both decode through csrc/anchor_decode.h under -ffp-contract=off) and against the
numpy restatement of tests/anchor_predict_ref.py (which tests/test_anchor_predict_cpu.py pins to the same fixture)."""
import copy
import os

import numpy as np
import pytest
import torch

import anchor_predict_ref as R
import anchor_util as AU
from sparse2dense_amd import anchor_predict as AP, waymo_configs as WC
from sparse2dense_amd.registry import build_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
META = [dict(token="a"), dict(token="b"), dict(token="c")]


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv("S2D_ANCHOR_DEVICE_PREDICT", raising=False)


def _head():
    return build_head(WC.second_voxelnet_train()["bbox_head"]).to(DEV)


def _cuda(preds):
    return [{k: v.to(DEV) for k, v in p.items()} for p in preds]


def _example(tables, batch):
    return dict(anchors=[torch.from_numpy(t).to(DEV).unsqueeze(0).expand(batch, -1, -1) for t in tables], metadata=META[:batch])


def _identical(got, want, what=""):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert set(a) == {"box3d_lidar", "scores", "label_preds", "metadata"} and a["metadata"] == b["metadata"], (what, i)
        for k in ("scores", "label_preds", "box3d_lidar"):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, i, k, a[k].shape, b[k].shape)
            if not torch.equal(a[k], b[k]):
                print(f"{what} sample {i} {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} elements differ, "
                      f"max |difference| {float((a[k].double() - b[k].double()).abs().max()):.3e}")
            assert torch.equal(a[k], b[k]), (what, i, k)


def _close(got, ref, what=""):
    """the tolerances of test_predict_vs_reference for anchor_predict.npz; kept scores and labels in order"""
    assert len(got) == len(ref), what
    for i, (a, r) in enumerate(zip(got, ref)):
        assert a["scores"].shape == r["scores"].shape, (what, i, a["scores"].shape, r["scores"].shape)
        np.testing.assert_allclose(a["scores"].cpu().numpy(), r["scores"], rtol=1e-5, err_msg=f"{what} {i}")
        assert np.array_equal(a["label_preds"].cpu().numpy(), r["label_preds"]) and a["label_preds"].dtype == torch.int64, (what, i)
        np.testing.assert_allclose(a["box3d_lidar"].cpu().numpy(), r["box3d_lidar"], rtol=1e-4, atol=2e-4, err_msg=f"{what} {i}")


def _both(head, example, preds, cfg):
    """(device path, chain) on the same inputs, asserting that predict() took the device path"""
    before = dict(head.predict_paths)
    dev = head.predict(example, preds, cfg)
    assert head.predict_paths == dict(before, device=before["device"] + 1), (head.predict_paths, head.device_predict_reason(preds))
    return dev, head.predict_torch(example, preds, cfg)


def test_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "anchor_predict.npz"))
    head = _head()
    box, cls, dirs = [t.to(DEV) for t in AU.predict_inputs(2)]
    preds = [dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)]
    example = _example([R.second_table(AU.H, AU.W)], 2)
    dev, old = _both(head, example, preds, WC.SECOND_TEST_CFG)
    assert head.predict_paths == {"device": 1, "torch": 0}
    _close(dev, [dict(scores=g[f"scores_{i}"], label_preds=g[f"label_preds_{i}"], box3d_lidar=g[f"box3d_lidar_{i}"]) for i in range(2)], "golden")
    _identical(dev, old, "golden")
    # the candidates themselves: the pass set of the fixture, sorted by descending score
    cand = AP.decode_anchor_candidates(preds, [example["anchors"][0][0]], WC.SECOND_TEST_CFG)
    assert cand.passed == cand.counts == [len(g["cand_index_0"]), len(g["cand_index_1"])] and cand.offsets == [0, cand.counts[0]]
    for i in range(2):
        rows = slice(cand.offsets[i], cand.offsets[i] + cand.counts[i])
        order = np.argsort(-g[f"cand_scores_{i}"], kind="stable")
        np.testing.assert_allclose(cand.scores[rows].cpu().numpy(), g[f"cand_scores_{i}"][order], rtol=1e-5)
        assert np.array_equal(cand.labels[rows].cpu().numpy(), g[f"cand_labels_{i}"][order])
        assert np.array_equal(cand.dirs[rows].cpu().numpy(), g[f"cand_dir_{i}"][order])
        want = g[f"cand_boxes_{i}"][order] * np.array([1, 1, 1, 1, 1, 1, -1], np.float32)   # the NMS form: heading negated
        np.testing.assert_allclose(cand.boxes[rows].cpu().numpy(), want, rtol=1e-4, atol=2e-4)
        assert bool(cand.in_range[rows].all())


def test_small_shapes_every_cut_and_the_range_after_the_nms():
    box, cls, dirs, table, cfg = R.small_case()
    ref, segments = R.check_small_case(box, cls, dirs, table, cfg)   # asserts the properties of the inputs on the host (see its docstring)
    head = _head()
    preds = _cuda([dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)])
    dev, old = _both(head, _example([table], R.SMALL_B), preds, cfg)
    _identical(dev, old, "small")
    _close(dev, ref, "small")
    assert [len(d["scores"]) for d in dev][2] == 0 and dev[2]["box3d_lidar"].shape == (0, 7)
    cand = AP.decode_anchor_candidates(preds, [torch.from_numpy(table).to(DEV)], cfg)
    assert cand.passed == [len(c[0]) for c, _ in segments[0]] and cand.counts == [16, cand.passed[1], 0]
    # no range: nothing is dropped after the NMS
    open_cfg = dict(cfg, post_center_limit_range=None)
    dev, old = _both(head, _example([table], R.SMALL_B), preds, open_cfg)
    _identical(dev, old, "small, no range")
    _close(dev, R.predict(preds, [table], open_cfg, [3])[0], "small, no range")
    assert len(dev[1]["scores"]) == cfg["nms"]["nms_post_max_size"]


def test_two_tasks_with_different_anchor_and_class_counts():
    preds, tables = R.two_task_case()
    assert [t.shape[0] for t in tables] == [128, 256]
    head = R.two_task_head().to(DEV)
    assert head.num_classes == [1, 2]
    cfg = copy.deepcopy(WC.SECOND_TEST_CFG)
    dev, old = _both(head, _example(tables, 2), _cuda(preds), cfg)
    _identical(dev, old, "two tasks")
    ref, segments = R.predict(preds, tables, cfg, [1, 2])
    _close(dev, ref, "two tasks")
    for i, d in enumerate(dev):   # task order inside a sample, the labels of task 1 offset by the one class of task 0
        n0 = len(segments[0][i][1]["scores"])
        labels = d["label_preds"].cpu().numpy()
        assert n0 > 0 and len(labels) > n0 and (labels[:n0] == 0).all() and (labels[n0:] >= 1).all() and set(labels[n0:]) <= {1, 2}


def test_no_anchor_passes_anywhere():
    box, cls, dirs, table, cfg = R.small_case()
    head = _head()
    preds = _cuda([dict(box_preds=box[:2], cls_preds=torch.full_like(cls[:2], -6.0), dir_cls_preds=dirs[:2])])
    example = _example([table], 2)
    dev, old = _both(head, example, preds, cfg)
    _identical(dev, old, "empty")
    for i, d in enumerate(dev):
        assert d["box3d_lidar"].shape == (0, 7) and d["scores"].shape == (0,) and d["label_preds"].shape == (0,)
        assert d["box3d_lidar"].dtype == torch.float32 and d["scores"].dtype == torch.float32 and d["label_preds"].dtype == torch.int64
        assert d["metadata"] == example["metadata"][i] and d["box3d_lidar"].is_cuda


def test_switch_and_bounds_fall_back_to_the_chain(monkeypatch):
    box, cls, dirs, table, cfg = R.small_case()
    head = _head()
    preds = _cuda([dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)])
    example = _example([table], R.SMALL_B)
    on = head.predict(example, preds, cfg)
    assert head.predict_paths == {"device": 1, "torch": 0} and head.device_predict_reason(preds) is None
    monkeypatch.setenv("S2D_ANCHOR_DEVICE_PREDICT", "0")
    off = head.predict(example, preds, cfg)
    assert head.predict_paths == {"device": 1, "torch": 1} and "S2D_ANCHOR_DEVICE_PREDICT=0" in head.device_predict_reason(preds)
    _identical(on, off, "switch")
    monkeypatch.delenv("S2D_ANCHOR_DEVICE_PREDICT")
    monkeypatch.setattr(AP, "NMS_MAX_BOXES", 8)   # below the 16 candidates of frame 0: the whole call takes the chain
    assert AP.predict_on_device(preds, [example["anchors"][0][0]], cfg, [3]) is None
    low = head.predict(example, preds, cfg)
    assert head.predict_paths == {"device": 1, "torch": 2}
    _identical(on, low, "candidate bound")
    monkeypatch.setattr(AP, "NMS_MAX_BOXES", 65536)
    monkeypatch.setattr(AP, "NMS_MAX_WORKSPACE_BYTES", 64)
    ws = head.predict(example, preds, cfg)
    assert head.predict_paths == {"device": 1, "torch": 3}
    _identical(on, ws, "workspace bound")


def test_unsupported_options_raise_before_any_launch():
    box, cls, dirs, table, cfg = R.small_case()
    preds = _cuda([dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)])
    example = _example([table], R.SMALL_B)
    head = _head()

    def edit(section, key, value):
        c = copy.deepcopy(cfg)
        (c[section] if section else c)[key] = value
        return c
    for bad, text in ((edit("nms", "use_multi_class_nms", True), "MultiGroupHead.predict: test_cfg.nms.use_multi_class_nms=True is not supported"),
                      (edit("nms", "use_rotate_nms", False), "MultiGroupHead.predict: test_cfg.nms.use_rotate_nms=False is not supported"),
                      (edit(None, "score_threshold", 0.0), "MultiGroupHead.predict: test_cfg.score_threshold <= 0 is not supported")):
        with pytest.raises(NotImplementedError) as err:
            head.predict(example, preds, bad)
        assert str(err.value) == text
    with pytest.raises(NotImplementedError) as err:
        head.predict(dict(example, anchors_mask=[None]), preds, cfg)
    assert str(err.value) == "MultiGroupHead.predict: anchors_mask (pos_area_threshold >= 0) is not supported"
    bev = copy.deepcopy(WC.second_voxelnet_train()["bbox_head"])
    bev["mode"] = "bev"
    bev_head = build_head(bev).to(DEV)
    with pytest.raises(NotImplementedError) as err:
        bev_head.predict(example, preds, cfg)
    assert str(err.value) == "MultiGroupHead.predict: mode='bev' is not supported"
    assert head.predict_paths == bev_head.predict_paths == {"device": 0, "torch": 0}


def test_layouts_non_contiguous_and_bf16():
    box, cls, dirs, table, cfg = R.small_case()
    head = _head()
    example = _example([table], R.SMALL_B)
    box16 = box.to(DEV).bfloat16()
    wide = torch.zeros((R.SMALL_B, R.SMALL_H, R.SMALL_W, 2 * cls.shape[-1]), device=DEV)
    wide[..., ::2] = cls.to(DEV)
    strided = wide[..., ::2]
    assert not strided.is_contiguous() and torch.equal(strided, cls.to(DEV))
    got = head.predict(example, [dict(box_preds=box16, cls_preds=strided, dir_cls_preds=dirs.to(DEV))], cfg)
    want = head.predict(example, [dict(box_preds=box16.float().contiguous(), cls_preds=strided.float().contiguous(), dir_cls_preds=dirs.to(DEV))], cfg)
    assert head.predict_paths == {"device": 2, "torch": 0}
    _identical(got, want, "layouts")
    assert sum(len(d["scores"]) for d in got) > 0


def test_two_calls_are_bit_equal():
    box, cls, dirs, table, cfg = R.small_case()
    head = _head()
    preds = _cuda([dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)])
    example = _example([table], R.SMALL_B)
    first = head.predict(example, preds, cfg)
    second = head.predict(example, preds, cfg)
    assert head.predict_paths == {"device": 2, "torch": 0}
    _identical(first, second, "repeat")
