"""CenterPoint target assignment for a table of tasks (the six-task nuScenes head): the host restatement
`scene.assign_targets_tasks` against outputs of the reference's own `AssignLabel` class (tests/golden/assign_label_nusc.npz, generated
by tests/golden/make_golden_nusc.py), and the device kernel (csrc/targets.hip, s2d_assign_label_tasks) against the host restatement.
Bars as in tests/test_targets.py: ind / mask / cat exact, hm within 1e-6 absolute, anno_box / gt_boxes_and_cls within 1e-6."""
import os

import numpy as np
import pytest
import torch

from sparse2dense_amd import scene
from sparse2dense_amd.waymo_configs import NUSC_TASKS

N_TASKS = len(NUSC_TASKS)


def _frames(golden_dir):
    g = np.load(os.path.join(golden_dir, "assign_label_nusc.npz"))
    assert int(g["n_tasks"]) == N_TASKS
    return g, [(g[f"f{fi}.gt_boxes"], g[f"f{fi}.gt_classes"], int(g[f"f{fi}.max_objs"])) for fi in range(int(g["n_frames"]))]


def _check(got, want, where, boxes_and_cls=True):
    """got / want: dicts of per-task lists of numpy arrays (+ gt_boxes_and_cls)"""
    for ti in range(len(want["hm"])):
        for k in ("ind", "mask", "cat"):
            assert got[k][ti].dtype == want[k][ti].dtype and np.array_equal(got[k][ti], want[k][ti]), (where, ti, k)
        np.testing.assert_allclose(got["hm"][ti], want["hm"][ti], rtol=0, atol=1e-6, err_msg=f"{where} hm task {ti}")
        np.testing.assert_allclose(got["anno_box"][ti], want["anno_box"][ti], rtol=1e-6, atol=1e-6, err_msg=f"{where} anno_box task {ti}")
    if boxes_and_cls:
        np.testing.assert_allclose(got["gt_boxes_and_cls"], want["gt_boxes_and_cls"], rtol=1e-6, atol=1e-6, err_msg=f"{where} gt_boxes_and_cls")


@pytest.mark.parametrize("fi", [0, 1, 2])
def test_host_restatement_matches_reference_assignlabel_six_tasks(golden_dir, fi):
    g, frames = _frames(golden_dir)
    boxes, classes, max_objs = frames[fi]
    t = scene.assign_targets_tasks(boxes, classes, NUSC_TASKS, max_objs=max_objs)
    want = {k: [g[f"f{fi}.t{ti}.{k}"] for ti in range(N_TASKS)] for k in ("hm", "anno_box", "ind", "mask", "cat")}
    assert t["hm"][1].shape == (2, 180, 180) and t["anno_box"][0].shape == (max_objs, 10)
    has_bc = f"f{fi}.gt_boxes_and_cls" in g   # (the reference cannot finish a frame with more objects than max_objs: make_golden_nusc.py)
    if has_bc:
        want["gt_boxes_and_cls"] = g[f"f{fi}.gt_boxes_and_cls"]
    _check(t, want, f"frame {fi}", boxes_and_cls=has_bc)
    n_pos = [int(m.sum()) for m in t["mask"]]
    if fi == 2:   # the edge frame: the car task is cut at max_objs, the barrier task is empty
        assert has_bc is False and n_pos[0] == max_objs == 16 and int((classes == 1).sum()) > max_objs and n_pos[3] == 0
        assert t["gt_boxes_and_cls"].shape == (16, 10) and np.all(t["gt_boxes_and_cls"][:, 9] == 1)   # the first 16 rows of the flattened list: cars
    else:
        assert has_bc and sum(n_pos) > 30


def test_one_task_table_equals_assign_targets(golden_dir):
    g = np.load(os.path.join(golden_dir, "assign_label.npz"))
    boxes, classes = g["f2.gt_boxes"], g["f2.gt_classes"]
    order = np.concatenate([np.where(classes == c)[0] for c in (1, 2, 3)])
    kw = dict(pc_range=scene.WAYMO_RANGE, voxel_size=scene.WAYMO_VOXEL, grid_xy=(1504, 1504))
    one = scene.assign_targets(boxes[order], classes[order], **kw)
    for b, c in ((boxes[order], classes[order]), (boxes, classes)):   # (the task form regroups by class itself)
        t = scene.assign_targets_tasks(b, c, [dict(num_class=3, class_names=["VEHICLE", "PEDESTRIAN", "CYCLIST"])], **kw)
        for k in ("hm", "anno_box", "ind", "mask", "cat"):
            assert len(t[k]) == 1 and t[k][0].dtype == one[k].dtype and np.array_equal(t[k][0], one[k]), k
    np.testing.assert_allclose(t["gt_boxes_and_cls"], g["f2.gt_boxes_and_cls"], rtol=1e-6, atol=1e-6)


def _device(frames, tasks, **kw):
    from sparse2dense_amd import targets
    boxes, classes = targets.pad_boxes([f[0] for f in frames], [f[1] for f in frames], "cuda")
    out = targets.assign_label_tasks(boxes, classes, tasks, with_boxes_and_cls=True, **kw)
    torch.cuda.synchronize()
    return out


def _frame_of(out, fi):
    d = {k: [v[fi].cpu().numpy() for v in out[k]] for k in ("hm", "anno_box", "ind", "mask", "cat")}
    d["gt_boxes_and_cls"] = out["gt_boxes_and_cls"][fi].cpu().numpy()
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("max_objs", [500, 16])
def test_device_assign_label_tasks_matches_host_restatement(golden_dir, max_objs):
    """the three fixture frames plus an empty frame, at the fixture's max_objs (500) and at the edge frame's (16: every frame is cut)"""
    _, frames = _frames(golden_dir)
    frames = [f[:2] for f in frames] + [(np.zeros((0, 9), np.float32), np.zeros((0,), np.int32))]
    out = _device(frames, NUSC_TASKS, max_objs=max_objs)
    assert len(out["hm"]) == N_TASKS
    for ti, t in enumerate(NUSC_TASKS):
        assert out["hm"][ti].shape == (4, t["num_class"], 180, 180) and out["hm"][ti].is_contiguous() and out["hm"][ti].dtype == torch.float32
        assert out["anno_box"][ti].shape == (4, max_objs, 10) and out["anno_box"][ti].is_contiguous()
        assert out["ind"][ti].dtype == torch.int64 and out["mask"][ti].dtype == torch.uint8 and out["cat"][ti].dtype == torch.int64
        assert all(out[k][ti].is_contiguous() for k in ("ind", "mask", "cat"))
    for fi, (b, c) in enumerate(frames):
        _check(_frame_of(out, fi), scene.assign_targets_tasks(b, c, NUSC_TASKS, max_objs=max_objs), f"frame {fi}")
    assert all(int(m[3].sum()) == 0 for m in out["mask"]) and float(out["gt_boxes_and_cls"][3].abs().sum()) == 0


def _small_map_frames():
    """K = 300 boxes over a 23 x 17 map for the table [2, 3], max_objs 64: the ranking loop runs two passes (K > 256), the cut falls
    inside both tasks, boxes sit on all four borders and corners (clipped windows), and the class ids include 0, -1 and 11 (ignored)"""
    rs = np.random.RandomState(5)
    k = 300
    classes = rs.randint(1, 6, k).astype(np.int32)
    classes[[3, 77, 255, 256, 299]] = [0, -1, 11, 0, 11]
    vs, f = 0.5, 2
    w_m, h_m = 23 * vs * f, 17 * vs * f
    boxes = np.zeros((k, 9), np.float32)
    boxes[:, 0] = rs.uniform(0, w_m, k)
    boxes[:, 1] = rs.uniform(0, h_m, k)
    boxes[:, 2] = rs.uniform(-1, 1, k)
    boxes[:, 3:6] = rs.uniform(0.5, 9.0, (k, 3))
    boxes[:, 6:8] = rs.normal(0, 2, (k, 2))
    boxes[:, 8] = rs.uniform(-7, 7, k)
    corners = [(0.1, 0.1), (w_m - 0.1, 0.1), (0.1, h_m - 0.1), (w_m - 0.1, h_m - 0.1), (w_m / 2, 0.05), (w_m / 2, h_m - 0.05), (0.05, h_m / 2),
               (w_m - 0.05, h_m / 2)]
    for i, (x, y) in enumerate(corners):   # early original indices of classes 1 and 3: inside the cut of both tasks
        boxes[10 + i, :2] = (x, y)
        classes[10 + i] = 1 if i % 2 == 0 else 3
        boxes[10 + i, 3:5] = 8.0
    boxes[40, :2] = (w_m + 0.2, 1.0)   # outside
    boxes[41, 3] = 0.0                  # degenerate
    second = (boxes.copy()[::-1].copy(), classes[::-1].copy())
    kw = dict(pc_range=(0.0, 0.0, -3.0, w_m, h_m, 3.0), voxel_size=(vs, vs, 6.0), out_size_factor=f, grid_xy=(23 * f, 17 * f), max_objs=64)
    return [(boxes, classes), second], [dict(num_class=2, class_names=["a", "b"]), dict(num_class=3, class_names=["c", "d", "e"])], kw


@pytest.mark.gpu
def test_device_ranking_above_block_size_cut_inside_task_and_clipped_windows():
    frames, tasks, kw = _small_map_frames()
    out = _device(frames, tasks, **kw)
    for fi, (b, c) in enumerate(frames):
        want = scene.assign_targets_tasks(b, c, tasks, **kw)
        assert int((c == 1).sum() + (c == 2).sum()) > 64 and int((c >= 3).sum() - (c == 11).sum()) > 64   # both tasks are cut
        assert [int(m.sum()) for m in want["mask"]] == [int(m[fi].sum()) for m in out["mask"]]
        _check(_frame_of(out, fi), want, f"frame {fi}")
        assert set(np.unique(want["gt_boxes_and_cls"][:, 9])) <= {1.0, 2.0}   # 64 rows of the flattened list: the first task only
    assert out["hm"][0].shape == (2, 2, 17, 23) and out["hm"][1].shape == (2, 3, 17, 23) and all(h.is_contiguous() for h in out["hm"])


@pytest.mark.gpu
def test_device_assign_label_tasks_is_deterministic():
    frames, tasks, kw = _small_map_frames()
    a, b = _device(frames, tasks, **kw), _device(frames, tasks, **kw)
    for k in ("hm", "anno_box", "ind", "mask", "cat"):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x, y), k
    assert torch.equal(a["gt_boxes_and_cls"], b["gt_boxes_and_cls"])
