"""CPU side of the device CenterHead.predict: the float64 restatement (tests/predict_ref.py) against the reference's recorded outputs,
and the argument validation of the new C entries (no GPU, no compute)."""
import os
import sys

import numpy as np
import pytest

import predict_ref as R
from sparse2dense_amd import _lib, build

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import predict_tasks_util as U   # noqa: E402


def _check_against_golden(out, g):
    """labels and keep order exactly; scores to 1e-6; boxes to 1e-5 (relative, with the same absolute floor: the recorded boxes are
    float32 and x = cell * 0.8 - 51.2 (or - 75.2) cancels, so a coordinate near 0 carries the rounding of a value near 75: 4e-6)"""
    assert len(out) == int(g["samples"])
    for i, r in enumerate(out):
        assert np.array_equal(r["label_preds"], g[f"labels{i}"]), i   # same boxes kept, in the same order, with the same classes
        np.testing.assert_allclose(r["scores"], g[f"scores{i}"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(r["box3d_lidar"], g[f"boxes{i}"], rtol=1e-5, atol=1e-5)


def test_restatement_matches_the_six_task_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "predict_tasks_flip_circle.npz"))
    preds = [{k: v.numpy() for k, v in p.items()} for p in U.predict_tasks_inputs()]
    out, margins = R.predict(preds, U.CFG)
    margins.check()   # the fixture's seed keeps clear of every decision boundary: the device test compares it exactly as well
    assert out[0]["box3d_lidar"].shape[1] == 9 and len(set(out[0]["label_preds"].tolist())) == 10
    _check_against_golden(out, g)


def test_restatement_matches_the_waymo_flip_circle_golden(golden_dir):
    from golden_util import PREDICT_FLIP_CIRCLE_CFG as CFG, predict_flip_circle_inputs
    g = np.load(os.path.join(golden_dir, "predict_flip_circle.npz"))
    out, _ = R.predict([{k: v.numpy() for k, v in predict_flip_circle_inputs().items()}], CFG, pair_margins=False)
    assert out[0]["box3d_lidar"].shape == (83, 7)
    _check_against_golden(out, g)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()   # loads without a GPU


def _task(vel=True, classes=2, bad_map=None, stride=1):
    t = _lib.CenterPredictTask()
    for m in range(6):
        t.map[m] = None if (m == 4 and not vel) or m == bad_map else 0x1000   # never dereferenced: validation fails first
        t.channel_stride[m], t.pixel_stride[m] = stride, 1
    t.classes = classes
    return t


def _tasks(n, **kw):
    arr = (_lib.CenterPredictTask * max(n, 1))()
    for i in range(n):
        arr[i] = _task(**kw)
    return arr


def test_decode_entries_validate_their_arguments(lib):
    P = 0x1000   # a non-null stand-in; every call below must fail before any HIP call
    geo = (4.0, 0.2, 0.2, -51.2, -51.2)

    def score(tasks, nt, samples=1, h=4, w=4):
        return lib.s2d_center_predict_score(tasks, nt, samples, h, w, 0, 0.1, None, *geo, P, P, P, None)

    def boxes(tasks, nt, samples=1, h=4, w=4, max_count=4, total=4, order=P):
        return lib.s2d_center_predict_boxes(tasks, nt, samples, h, w, 0, *geo, order, P, P, P, P, max_count, total, P, P, P, None)

    for fn in (score, boxes):
        for call, text in [(lambda: fn(None, 1), "null task table"), (lambda: fn(_tasks(1), 0), "0 tasks"), (lambda: fn(_tasks(9), 9), "9 tasks"),
                           (lambda: fn(_tasks(1), 1, samples=-1), "negative size"), (lambda: fn(_tasks(1), 1, h=-4), "negative size"),
                           (lambda: fn(_tasks(1, bad_map=0), 1), "null map 0"), (lambda: fn(_tasks(1, bad_map=5), 1), "null map 5"),
                           (lambda: fn(_tasks(1, classes=0), 1), "0 classes"), (lambda: fn(_tasks(1, stride=-1), 1), "negative stride")]:
            rc = call()
            assert rc == -1 and text in _lib.last_error(), (fn.__name__, text, rc, _lib.last_error())
    mixed = _tasks(2)
    mixed[1] = _task(vel=False)
    assert score(mixed, 2) == -1 and "vel on some tasks only" in _lib.last_error()
    assert lib.s2d_center_predict_score(_tasks(1), 1, 1, 4, 4, 0, 0.1, None, *geo, P, P, None, None) == -1 and "null count" in _lib.last_error()
    assert boxes(_tasks(1), 1, max_count=-1) == -1 and "negative size" in _lib.last_error()
    assert boxes(_tasks(1), 1, total=-1) == -1 and "negative size" in _lib.last_error()
    assert boxes(_tasks(1), 1, order=None) == -1 and "null argument" in _lib.last_error()
    with pytest.raises(_lib.S2DError):
        _lib.check(-1, "s2d_center_predict_boxes")


def test_batched_nms_entries_validate_their_arguments(lib):
    P = 0x1000
    assert lib.s2d_nms_batched_workspace_bytes(0, 0) == 256
    need = lib.s2d_nms_batched_workspace_bytes(4990, 4097)
    assert need >= 4990 * 65 * 8 and need % 256 == 0

    def rot(rows=P, stride=7, off=P, cnt=P, segs=2, max_count=100, total=150, max_keep=10, keep=P, n_keep=P, ws=P, ws_bytes=1 << 30):
        return lib.s2d_nms_rotated_bev_batched(rows, stride, off, cnt, segs, max_count, total, 0.2, max_keep, keep, n_keep, ws, ws_bytes, None)

    def circ(rows=P, stride=2, off=P, cnt=P, segs=2, max_count=100, total=150, max_keep=10, keep=P, n_keep=P, ws=P, ws_bytes=1 << 30, thresh=P):
        return lib.s2d_nms_circle_batched(rows, stride, off, cnt, segs, max_count, total, thresh, max_keep, keep, n_keep, ws, ws_bytes, None)

    for fn, min_stride in ((rot, 7), (circ, 2)):
        for kw, text in [(dict(segs=-1), "segments"), (dict(segs=65536), "segments"), (dict(max_count=-1), "max_count"),
                         (dict(max_count=65537), "max_count"), (dict(total=-1), "negative size"), (dict(max_keep=-1), "negative size"),
                         (dict(stride=min_stride - 1), "row stride"), (dict(n_keep=None), "null segment arrays"), (dict(off=None), "null segment arrays"),
                         (dict(cnt=None), "null segment arrays"), (dict(rows=None), "null argument"), (dict(keep=None), "null argument")]:
            rc = fn(**kw)
            assert rc == -1 and text in _lib.last_error(), (fn.__name__, kw, rc, _lib.last_error())
        small = lib.s2d_nms_batched_workspace_bytes(150, 100) - 1
        for kw in (dict(ws_bytes=small), dict(ws=None)):
            rc = fn(**kw)
            assert rc == -4 and "workspace too small" in _lib.last_error(), (fn.__name__, kw, rc)   # S2D_ERR_WORKSPACE
    assert circ(thresh=None) == -1 and "null argument" in _lib.last_error()


def test_host_api_fails_loudly_on_cpu_tensors():
    import torch
    from sparse2dense_amd import center_predict, nms
    seg = torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(_lib.S2DError):
        nms.rotate_nms_batched(torch.zeros(3, 7), seg, [3], 0.5)
    with pytest.raises(_lib.S2DError):
        nms.circle_nms_batched(torch.zeros(3, 2), seg, [3], [1.0])
    with pytest.raises(_lib.S2DError):
        center_predict.decode_center_maps([{k: v for k, v in U.seeded_task_maps(1, 0, 3, 3, 1, False).items()}], U.CFG)
