"""The tracker's host side (sparse2dense_amd/tracking.py) against the golden of the reference's two PubTracker classes
(tests/golden/tracking.npz): the numpy restatement `step_host`, the `Tracker` on CPU tensors and the dictionary class `PubTracker`, both
flavours; ids, classes, ages, active and the list order exactly, ct within 1e-9 m.  `decision_clear` at 2e-3 m holds before every golden
step, which is what makes the exact comparison a condition and not a measurement.  Then the limits, the rejected inputs, the empty frame
and the single deviation from the reference (a frame whose rows are all filtered ages the tracks)."""
import numpy as np
import pytest
import torch

import tracking_util as U
from sparse2dense_amd import _lib, tracking as T


@pytest.fixture(scope="module")
def golden(golden_dir):
    return U.load_golden(golden_dir)


@pytest.mark.parametrize("tag", ["w", "n"])
def test_step_host_equals_the_reference(golden, tag):
    table, thresh, _ = U.flavour(golden, tag)
    state, last = T.new_state(1), None
    for f in U.frames(golden, tag):
        lag = 0.0 if f["first"] else f["stamp"] - last
        last = f["stamp"]
        args = (f["boxes"], f["labels"], [0, len(f["boxes"])], f["pose"][None], [lag], [f["first"]], [False], table)
        assert T.decision_clear(state, *args, U.EPS), (tag, f["index"])
        tid, act = T.step_host(state, f["boxes"], f["labels"], f["scores"], [0, len(f["boxes"])], f["pose"][None], [lag], [f["first"]], [False],
                               table, U.MAX_AGE, thresh)
        U.check_step(golden, tag, f["index"], tid, act, U.host_state(state, 0))


@pytest.mark.parametrize("tag", ["w", "n"])
def test_tracker_on_cpu_tensors_equals_the_reference(golden, tag):
    table, thresh, _ = U.flavour(golden, tag)
    tracker = T.Tracker(1, table, U.MAX_AGE, thresh, device="cpu")
    for f in U.frames(golden, tag):
        dets = [dict(box3d_lidar=torch.from_numpy(f["boxes"]), label_preds=torch.from_numpy(f["labels"]), scores=torch.from_numpy(f["scores"]))]
        tid, act, off = tracker.step(dets, f["pose"][None], [f["stamp"]], first=[f["first"]])
        assert tid.dtype == torch.int32 and act.dtype == torch.int32 and off.tolist() == [0, len(f["boxes"])]
        U.check_step(golden, tag, f["index"], tid.numpy(), act.numpy(), tracker.state(0))


def _annos(f, names):
    """the reference driver's dictionaries of one frame: the boxes in the global frame (float64) by the pose"""
    b = f["boxes"].astype(np.float64)
    centre = b[:, :3] @ f["pose"][:3, :3].T + f["pose"][:3, 3]
    vel = b[:, 6:8] @ f["pose"][:2, :2].T
    return [dict(translation=centre[i], velocity=vel[i], detection_name=names[f["labels"][i]], score=f["scores"][i], box_id=i)
            for i in range(len(b))]


@pytest.mark.parametrize("tag", ["w", "n"])
def test_pub_tracker_equals_the_reference(golden, tag):
    _, _, dist = U.flavour(golden, tag)
    tracker = T.PubTracker(max_age=U.MAX_AGE, max_dist=dist, score_thresh=0.75) if tag == "w" else T.PubTracker(max_age=U.MAX_AGE, hungarian=False)
    names, last = (U.WAYMO_NAMES if tag == "w" else U.NUSC_NAMES), None
    for f in U.frames(golden, tag):
        if f["first"]:
            tracker.reset()
            last = f["stamp"]
        lag, last = f["stamp"] - last, f["stamp"]
        out = tracker.step_centertrack(_annos(f, names), lag)
        assert out == tracker.tracks
        tid, act = np.full(len(f["boxes"]), -1, np.int32), np.zeros(len(f["boxes"]), np.int32)
        for o in out:
            if o["active"] > 0:
                tid[o["box_id"]], act[o["box_id"]] = o["tracking_id"], o["active"]
        state = dict(ids=np.array([t["tracking_id"] for t in out], np.int64), classes=np.array([t["label_preds"] for t in out], np.int64),
                     ages=np.array([t["age"] for t in out], np.int64), active=np.array([t["active"] for t in out], np.int64),
                     ct=np.array([t["ct"] for t in out], np.float64).reshape(-1, 2))
        U.check_step(golden, tag, f["index"], tid, act, state)


def test_golden_holds_what_it_promises(golden):
    for tag in ("w", "n"):
        tracks, off = golden[f"{tag}_tracks"], golden[f"{tag}_track_offsets"]
        per_step = [tracks[off[i]:off[i + 1]] for i in range(len(off) - 1)]
        assert len(per_step) == 12 and len(per_step[6]) == 0 and np.diff(golden[f"{tag}_offsets"])[6] == 0
        ages = np.concatenate(per_step)[:, 2]
        assert ages.max() == U.MAX_AGE and (np.concatenate(per_step)[:, 3] == 0).any()
        back = [t for t in per_step[4] if t[3] == 1 and t[0] in set(per_step[1][:, 0])]   # matched again after two frames away: active restarts at 1
        assert back, tag
        assert per_step[8][:, 0].min() == 1 and per_step[7][:, 0].max() > 1, tag   # the second sequence starts at id 1 again
        table, _, _ = U.flavour(golden, tag)
        assert any(table[l][0] < 0 for l in golden[f"{tag}_labels"]), tag
    s = golden["w_scores"]
    assert (s > 0.76).any() and (s < 0.74).any() and np.abs(s - 0.75).min() >= 0.0099
    assert np.abs(golden["w_poses"][:, :3, 3]).max() < 2000 and len(set(np.round(np.diff(golden["w_stamps"]), 3))) > 2


def _one(n, label=0, x0=0.0):
    boxes = np.zeros((n, 9), np.float32)
    boxes[:, 0] = x0 + 10.0 * np.arange(n)
    return boxes, np.full(n, label, np.int64), np.full(n, 0.9, np.float32)


def test_limits_and_rejected_inputs():
    table = [(0, 1.0), (-1, 0.0)]
    pose = np.eye(4)[None]
    tracker = T.Tracker(1, table, max_age=4, device="cpu")   # (with max_age <= 3 four frames of 1024 rows are all a segment can hold)
    with pytest.raises(_lib.S2DError, match="1024"):
        tracker.step((*_one(1025), [0, 1025]), pose, [0.0])
    for k in range(4):
        tracker.step((*_one(1024, x0=float(k)), [0, 1024]), pose, [0.5 * k])
    with pytest.raises(_lib.S2DError, match="4096"):   # 4 x 1024 + 1 rows in the last max_age + 1 = 5 frames
        tracker.step((*_one(1), [0, 1]), pose, [2.0])
    tracker.step((np.zeros((0, 9), np.float32), np.zeros(0, np.int64), np.zeros(0, np.float32), [0, 0]), pose, [2.0])   # an empty frame clears
    tracker.step((*_one(1024), [0, 1024]), pose, [2.5])
    with pytest.raises(ValueError, match="7-column"):
        tracker.step((np.zeros((3, 7), np.float32), np.zeros(3, np.int64), np.zeros(3, np.float32), [0, 3]), pose, [3.0])
    with pytest.raises(ValueError, match="7-column"):
        T.step_host(T.new_state(1), np.zeros((3, 7), np.float32), np.zeros(3), np.zeros(3), [0, 3], pose, [0.0], [True], [False], table, 3)
    with pytest.raises(NotImplementedError):
        T.Tracker(1, table, 3, device="cpu", hungarian=True)
    with pytest.raises(NotImplementedError):
        T.Tracker.nuscenes(device="cpu", hungarian=True)
    with pytest.raises(NotImplementedError):
        T.PubTracker(hungarian=True, max_age=3)
    with pytest.raises(_lib.S2DError):
        T.Tracker(65, table, 3, device="cpu")
    with pytest.raises(_lib.S2DError):
        tracker.step((*_one(4), [0, 5]), pose, [3.0])
    with pytest.raises(ValueError):
        T.Tracker(2, table, 3, device="cpu").step((*_one(4), [0, 2, 4]), np.eye(4)[None].repeat(2, 0), [0.0, 0.0], first=[True, False])


def test_constructors_follow_the_reference_tables():
    n = T.Tracker.nuscenes(device="cpu")
    assert n.max_age == 3 and n.score_thresh is None and len(n.class_table) == 10
    assert n.class_table[0] == (2, 4.0) and n.class_table[2] == (-1, 0.0) and n.class_table[6] == (3, 13.0) and n.class_table[8] == (4, 1.0)
    w = T.Tracker.waymo(dict(VEHICLE=0.8, PEDESTRIAN=0.4, CYCLIST=0.6), device="cpu")
    assert w.max_age == 3 and w.score_thresh == 0.75 and w.class_table == [(0, 0.8), (1, 0.4), (2, 0.6)]
    p = T.PubTracker(3, dict(VEHICLE=0.8), 0.5)
    assert (p.max_age, p.score_thresh, p.names) == (3, 0.5, T.WAYMO_TRACKING_NAMES)
    q = T.PubTracker(False, 2)
    assert (q.max_age, q.score_thresh, q.names) == (2, None, T.NUSCENES_TRACKING_NAMES)


def test_empty_frame_keeps_id_count_and_all_filtered_frame_ages():
    table = [(0, 1.0), (-1, 0.0)]
    pose = np.eye(4)[None]
    tracker = T.Tracker(1, table, max_age=2, device="cpu")
    tid, act, _ = tracker.step((*_one(3), [0, 3]), pose, [0.0])
    assert tid.tolist() == [1, 2, 3] and act.tolist() == [1, 1, 1]
    # THE DEVIATION: rows present, all filtered (the reference raises IndexError): every track is unmatched and ages
    tid, act, _ = tracker.step((*_one(2, label=1), [0, 2]), pose, [0.5])
    st = tracker.state(0)
    assert tid.tolist() == [-1, -1] and act.tolist() == [0, 0]
    assert st["ids"].tolist() == [1, 2, 3] and st["ages"].tolist() == [2, 2, 2] and st["active"].tolist() == [0, 0, 0] and st["id_count"] == 3
    tracker.step((*_one(2, label=1), [0, 2]), pose, [1.0])
    assert len(tracker.state(0)["ids"]) == 0 and tracker.state(0)["id_count"] == 3   # age 2 is not < max_age
    tid, _, _ = tracker.step((*_one(1), [0, 1]), pose, [1.5])
    assert tid.tolist() == [4]
    # a frame without rows clears the tracks and keeps id_count
    tracker.step((np.zeros((0, 9), np.float32), np.zeros(0, np.int64), np.zeros(0, np.float32), [0, 0]), pose, [2.0])
    assert len(tracker.state(0)["ids"]) == 0 and tracker.state(0)["id_count"] == 4
    tid, _, _ = tracker.step((*_one(2), [0, 2]), pose, [2.5])
    assert tid.tolist() == [5, 6]
    tid, _, _ = tracker.step((*_one(2), [0, 2]), pose, [3.0], first=[True])   # reset(): ids start at 1 again
    assert tid.tolist() == [1, 2]
    pub = T.PubTracker(max_age=2)
    pub.step_centertrack([dict(translation=np.zeros(3), velocity=np.zeros(2), detection_name="car")], 0.0)
    assert pub.step_centertrack([], 0.5) == [] and pub.tracks == [] and pub.id_count == 1


def test_decision_clear_sees_gates_and_near_ties():
    table = [(0, 1.0)]
    pose = np.eye(4)[None]
    state = T.new_state(1)
    trk = np.zeros((2, 9), np.float32)
    trk[:, 0] = [0.0, 3.0]
    T.step_host(state, trk, np.zeros(2, np.int64), np.ones(2, np.float32), [0, 2], pose, [0.0], [True], [False], table, 3)

    def clear(x):
        det = np.zeros((1, 9), np.float32)
        det[0, 0] = x
        return T.decision_clear(state, det, np.zeros(1, np.int64), [0, 1], pose, [0.5], [False], [False], table, U.EPS)
    assert clear(0.5) and clear(2.5) and clear(1.5)              # one valid track; exactly between the two, both out of range
    assert not clear(0.999) and not clear(1.001) and clear(1.01)  # at the gate
    table[0] = (0, 2.0)
    assert clear(1.5) and not clear(1.5005) and clear(1.51)       # an exact tie is decided by index; a near tie is not clear
