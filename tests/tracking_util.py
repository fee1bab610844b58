"""Shared by test_tracking_cpu.py and test_tracking_gpu.py: the golden of the reference's two trackers (tests/golden/tracking.npz,
make_golden_tracking.py), the comparison of a step with it (ids, classes, ages, active and list order exactly, ct within CT_ATOL), and
seeded random sequences on a 1/64 m grid for the comparison of the kernel with the restatement."""
import os

import numpy as np

from sparse2dense_amd import tracking as T
from sparse2dense_amd.waymo_configs import NUSC_TASKS

EPS = 2e-3       # decision_clear: no decision within 2 mm of flipping (a float32 ulp below 2000 m is 1.2e-4 m)
CT_ATOL = 1e-9   # double contraction may differ in the last bit of a centre near 2000 m (ulp 2.3e-13 m)
WAYMO_NAMES = ["VEHICLE", "PEDESTRIAN", "CYCLIST", "SIGN"]
NUSC_NAMES = [n for t in NUSC_TASKS for n in t["class_names"]]
MAX_AGE = 3


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "tracking.npz")))


def flavour(g, tag):
    """(class table with the golden's label order, score threshold, max_dist by name or None)"""
    if tag == "w":
        dist = dict(zip(T.WAYMO_TRACKING_NAMES, g["w_max_dist"].tolist()))
        return T.class_table_of(WAYMO_NAMES, T.WAYMO_TRACKING_NAMES, dist), 0.75, dist
    return T.class_table_of(NUSC_NAMES, T.NUSCENES_TRACKING_NAMES, T.NUSCENE_CLS_VELOCITY_ERROR), None, None


def frames(g, tag, sequence=None):
    """[dict(index, boxes, labels, scores, pose, stamp, first)] of a flavour, of one of its two sequences when asked"""
    off, seq = g[f"{tag}_offsets"], g[f"{tag}_sequence"]
    out = []
    for f in range(len(seq)):
        if sequence is not None and seq[f] != sequence:
            continue
        lo, hi = off[f], off[f + 1]
        out.append(dict(index=f, boxes=g[f"{tag}_boxes"][lo:hi], labels=g[f"{tag}_labels"][lo:hi], scores=g[f"{tag}_scores"][lo:hi],
                        pose=g[f"{tag}_poses"][f], stamp=g[f"{tag}_stamps"][f], first=f == 0 or seq[f] != seq[f - 1]))
    return out


def check_step(g, tag, index, tid, act, state):
    """a step's per-row outputs and track list against the golden's frame `index`"""
    items = g[f"{tag}_out"][g[f"{tag}_out_offsets"][index]:g[f"{tag}_out_offsets"][index + 1]]
    want = g[f"{tag}_tracks"][g[f"{tag}_track_offsets"][index]:g[f"{tag}_track_offsets"][index + 1]]
    tid, act = np.asarray(tid), np.asarray(act)
    assert np.array_equal(np.nonzero(act > 0)[0], np.sort(items[:, 0])), (tag, index)
    assert np.array_equal(tid[items[:, 0]], items[:, 1]) and np.array_equal(act[items[:, 0]], items[:, 2]), (tag, index)
    assert np.all(tid[act == 0] == -1), (tag, index)
    got = np.stack([state["ids"], state["classes"], state["ages"], state["active"]], 1)
    assert np.array_equal(got, want[:, :4].astype(np.int64)), (tag, index)
    assert state["ct"].shape == want[:, 4:].shape and np.abs(state["ct"] - want[:, 4:]).max(initial=0) <= CT_ATOL, (tag, index)


def host_state(state, segment):
    """the dictionary of Tracker.state from a numpy state"""
    count, id_count = (int(v) for v in state["head"][segment])
    meta = state["meta"][segment, :count]
    return dict(ids=meta[:, 1], classes=meta[:, 0], ages=meta[:, 2], active=meta[:, 3], ct=state["ct"][segment, :count],
                tracking=state["tracking"][segment, :count], id_count=id_count)


def same_state(got, want, what=""):
    """Tracker.state against the restatement's: everything exact but ct / tracking (CT_ATOL)"""
    for k in ("ids", "classes", "ages", "active"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["id_count"] == want["id_count"], what
    for k in ("ct", "tracking"):
        assert got[k].shape == want[k].shape and np.abs(got[k] - want[k]).max(initial=0) <= CT_ATOL, (what, k)


# ---- random sequences ----------------------------------------------------------------------------------------------------------------
GRID = 1.0 / 64
RANDOM_TABLE = [(0, 1.0), (1, 1.5), (-1, 0.0), (2, 0.75)]   # label 2 is no tracking class
SIZES = (0, 1, 63, 64, 65, 257, 1024)
SMALL_SIZES = SIZES[:-1]


def _snap(a):
    return np.round(np.asarray(a, np.float64) / GRID) * GRID


def random_pose(rng):
    """a quarter-turn about z and a grid translation: every product and sum of the transform is exact in float64 and in float32"""
    k = rng.randint(4)
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k]
    pose = np.eye(4)
    pose[:2, :2] = [[c, -s], [s, c]]
    pose[:3, 3] = _snap(rng.uniform(-500, 500, 3))
    return pose


def random_sequence(seed, rows_of, frames=6):
    """frames of one segment: rows_of(frame) objects of a pool twice the largest frame (so about half of a frame's detections find a
    track and the unmatched tracks pile up until max_age) on a 3 m lattice (jittered by up to 0.5 m), each moving with a constant
    grid velocity and detected with grid noise, seen through a fresh exact pose every frame; time steps are powers of two.  A lattice cell
    holds one object, so a detection's second-best valid track is rare and clear.  Returns [dict(boxes, labels, scores, pose, stamp)]."""
    rng = np.random.RandomState(seed)
    pool = 2 * max(max(rows_of(f) for f in range(frames)), 1)
    side = int(np.ceil(np.sqrt(pool)))
    cells = rng.permutation(side * side)[:pool]
    xy = np.stack([cells // side, cells % side], 1) * 3.0 + _snap(rng.uniform(-0.5, 0.5, (pool, 2)))
    vel = _snap(rng.uniform(-0.5, 0.5, (pool, 2)))
    labels = rng.randint(0, len(RANDOM_TABLE), pool)
    out, stamp = [], 100.0
    for f in range(frames):
        stamp += [0.5, 0.25, 0.5, 1.0][rng.randint(4)]
        n = rows_of(f)
        pick = rng.permutation(pool)[:n]
        pose = random_pose(rng)
        g = xy[pick] + vel[pick] * (stamp - 100.0) + _snap(rng.uniform(-0.1, 0.1, (n, 2)))
        local = (g - pose[:2, 3]) @ pose[:2, :2]          # R^T (g - t), exact for a quarter-turn
        v = vel[pick] @ pose[:2, :2]
        boxes = np.zeros((n, 9), np.float32)
        boxes[:, :2], boxes[:, 2], boxes[:, 3:6], boxes[:, 6:8] = local, _snap(rng.uniform(-2, 2, n)), 1.0, v
        out.append(dict(boxes=boxes, labels=labels[pick].astype(np.int64), scores=rng.uniform(0.05, 0.95, n).astype(np.float32), pose=pose,
                        stamp=stamp))
    return out


def pack(frames_of_segments):
    """one step's inputs of several segments: (boxes, labels, scores, offsets, poses, stamps)"""
    off = np.cumsum([0] + [len(f["boxes"]) for f in frames_of_segments])
    cat = lambda k: np.concatenate([f[k] for f in frames_of_segments], 0)
    return cat("boxes"), cat("labels"), cat("scores"), off, np.stack([f["pose"] for f in frames_of_segments]), \
        np.array([f["stamp"] for f in frames_of_segments])
