"""The tracker on the device (csrc/tracking.hip through sparse2dense_amd/tracking.Tracker): against the golden of the reference's two
PubTracker classes (ids, classes, ages, active and list order exactly, ct within 1e-9 m), as one segment, as two segments of one tracker and
among 63 other segments; against the numpy restatement `step_host` on seeded random sequences at the sizes where the kernel changes path
(a wave of 64 tracks or rows and its neighbours, more than one pass of the 16 waves, the limits of 1024 rows and 4096 tracks); and the
targeted cases: contention (the recompute path of phase 2), exact ties, skip, first, bit-equal repetition, the dictionaries of a
CenterHead.predict device call.

Condition, not measurement: `decision_clear` at 2e-3 m is asserted on the restatement alone before every random step; the seeds below were
found with the restatement.  Random coordinates lie on a 1/64 m grid behind quarter-turn poses with grid translations and time steps that
are powers of two, so every float64 and float32 operation of the transform is exact and both sides see the same float32 centres; the
float32 distance is the same sequence of IEEE operations on both sides.  The contention and tie cases rest on that alone: they hold near
ties on purpose and compare exactly.

Track counts: with max_age 3 a track lives three frames, so 1024 rows a frame reach 3072 tracks; the crossing of 4096 - 1 needs max_age 4
and has its own case."""
import os
import sys

import numpy as np
import pytest
import torch

import tracking_util as U
from sparse2dense_amd import _lib, tracking as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return U.load_golden(golden_dir)


def _dets(f):
    return dict(box3d_lidar=cuda(f["boxes"]), label_preds=cuda(f["labels"]), scores=cuda(f["scores"]))


def _empty():
    return dict(boxes=np.zeros((0, 9), np.float32), labels=np.zeros(0, np.int64), scores=np.zeros(0, np.float32), pose=np.eye(4), stamp=0.0)


def _host_buffers(tracker):
    return [t.cpu().numpy() for t in tracker.buffers()]


def _state_of(buffers, seg):
    ct, tracking, meta, head = buffers
    return U.host_state(dict(ct=ct, tracking=tracking, meta=meta, head=head), seg)


# ---- golden parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["w", "n"])
def test_golden_one_segment(golden, tag):
    table, thresh, _ = U.flavour(golden, tag)
    tracker = T.Tracker(1, table, U.MAX_AGE, thresh, device=DEV)
    assert tracker.on_device
    for f in U.frames(golden, tag):
        tid, act, off = tracker.step([_dets(f)], f["pose"][None], [f["stamp"]], first=[f["first"]])
        assert tid.is_cuda and act.is_cuda and off.is_cuda and tid.dtype == torch.int32 and off.tolist() == [0, len(f["boxes"])]
        U.check_step(golden, tag, f["index"], tid.cpu().numpy(), act.cpu().numpy(), tracker.state(0))


@pytest.mark.parametrize("tag", ["w", "n"])
def test_golden_two_sequences_as_two_segments(golden, tag):
    table, thresh, _ = U.flavour(golden, tag)
    seqs = [U.frames(golden, tag, 0), U.frames(golden, tag, 1)]
    tracker = T.Tracker(2, table, U.MAX_AGE, thresh, device=DEV)
    for k in range(len(seqs[0])):
        live = [k < len(s) for s in seqs]
        fr = [s[k] if ok else _empty() for s, ok in zip(seqs, live)]
        tid, act, off = tracker.step([_dets(f) for f in fr], np.stack([f["pose"] for f in fr]), [f["stamp"] for f in fr],
                                     first=[k == 0, k == 0], skip=[not ok for ok in live])
        tid, act, off = tid.cpu().numpy(), act.cpu().numpy(), off.tolist()
        for s in range(2):   # (a finished sequence is skipped: its last state stays)
            index = fr[s]["index"] if live[s] else seqs[s][-1]["index"]
            rows = slice(off[s], off[s + 1]) if live[s] else slice(0, 0)
            if live[s]:
                U.check_step(golden, tag, index, tid[rows], act[rows], tracker.state(s))
            else:
                want = golden[f"{tag}_tracks"][golden[f"{tag}_track_offsets"][index]:golden[f"{tag}_track_offsets"][index + 1]]
                assert np.array_equal(tracker.state(s)["ids"], want[:, 0].astype(np.int64))


@pytest.mark.parametrize("tag", ["w", "n"])
def test_golden_segment_alone_and_among_63_others(golden, tag):
    table, thresh, _ = U.flavour(golden, tag)
    seq = U.frames(golden, tag, 0)
    alone, crowd, at = T.Tracker(1, table, U.MAX_AGE, thresh, device=DEV), T.Tracker(64, table, U.MAX_AGE, thresh, device=DEV), 17
    for k, f in enumerate(seq):
        a_tid, a_act, _ = alone.step([_dets(f)], f["pose"][None], [f["stamp"]], first=[k == 0])
        fr = [f if s == at else seq[(k + s) % len(seq)] for s in range(64)]   # the others see the frames in another order
        c_tid, c_act, off = crowd.step([_dets(x) for x in fr], np.stack([x["pose"] for x in fr]), [x["stamp"] for x in fr], first=[k == 0] * 64)
        lo, hi = off.tolist()[at:at + 2]
        assert torch.equal(a_tid, c_tid[lo:hi]) and torch.equal(a_act, c_act[lo:hi])
        for a, c in zip(alone.buffers(), crowd.buffers()):
            assert torch.equal(a[0], c[at])
        U.check_step(golden, tag, f["index"], c_tid[lo:hi].cpu().numpy(), c_act[lo:hi].cpu().numpy(), crowd.state(at))


# ---- random sequences against step_host ----------------------------------------------------------------------------------------------
def _rows_plan(n, segments):
    """segment 0 and the last one see n rows every frame; the others walk through the small sizes"""
    return lambda s, f: n if s in (0, segments - 1) else U.SMALL_SIZES[(s + f) % len(U.SMALL_SIZES)]


# (n, max_age, segments) -> base seed with decision_clear at every step, found with the restatement alone; default 1
SEEDS = {(1024, 0, 64): 2}


@pytest.mark.parametrize("segments", [1, 3, 64])
@pytest.mark.parametrize("max_age", [0, 3])
@pytest.mark.parametrize("n", U.SIZES)
def test_random_sequences_equal_the_restatement(n, max_age, segments):
    thresh = 0.5 if max_age else None
    plan = _rows_plan(n, segments)
    seed = SEEDS.get((n, max_age, segments), 1)
    seqs = [U.random_sequence(seed * 1000 + s, lambda f, s=s: plan(s, f)) for s in range(segments)]
    tracker, state = T.Tracker(segments, U.RANDOM_TABLE, max_age, thresh, device=DEV), T.new_state(segments)
    last, peak = np.zeros(segments), 0
    for k in range(6):
        boxes, labels, scores, off, poses, stamps = U.pack([q[k] for q in seqs])
        first = [k == 0] * segments
        lag = np.where(first, 0.0, stamps - last)
        last = stamps
        assert T.decision_clear(state, boxes, labels, off, poses, lag, first, None, U.RANDOM_TABLE, U.EPS), (n, max_age, segments, k)
        want_tid, want_act = T.step_host(state, boxes, labels, scores, off, poses, lag, first, None, U.RANDOM_TABLE, max_age, thresh)
        tid, act, _ = tracker.step((cuda(boxes), cuda(labels), cuda(scores), off), poses, stamps, first=first)
        assert np.array_equal(tid.cpu().numpy(), want_tid) and np.array_equal(act.cpu().numpy(), want_act), (n, max_age, segments, k)
        buffers = _host_buffers(tracker)
        for s in range(segments):
            U.same_state(_state_of(buffers, s), U.host_state(state, s), (n, max_age, segments, k, s))
        peak = max(peak, int(state["head"][:, 0].max()))
    if n >= 257 and max_age:
        assert peak > 256   # the track lists cross a wave (64) and 256 on their way up
    if n >= 63 and max_age:
        assert peak > 64


def test_track_count_reaches_4096_and_the_bound_refuses_more():
    """max_age 4: four frames of 1024 detections that match nothing leave 1024, 2048, 3072 and 4096 tracks (crossing 4096 - 1); a fifth
    frame with one more row could make 4097 and is refused on the host before the launch."""
    table = [(0, 0.25)]
    tracker, state = T.Tracker(1, table, 4, None, device=DEV), T.new_state(1)
    pose = np.eye(4)[None]
    for k in range(4):
        boxes = np.zeros((1024, 9), np.float32)
        boxes[:, 0], boxes[:, 1] = np.arange(1024) % 32 * 4.0 + k, np.arange(1024) // 32 * 4.0   # frame k is shifted by k m: no match at 0.25 m
        labels, scores = np.zeros(1024, np.int64), np.ones(1024, np.float32)
        want_tid, want_act = T.step_host(state, boxes, labels, scores, [0, 1024], pose, [0.5 if k else 0.0], [k == 0], None, table, 4)
        tid, act, _ = tracker.step((cuda(boxes), cuda(labels), cuda(scores), [0, 1024]), pose, [0.5 * k])
        assert np.array_equal(tid.cpu().numpy(), want_tid) and np.array_equal(act.cpu().numpy(), want_act)
        assert int(state["head"][0, 0]) == 1024 * (k + 1)
        U.same_state(tracker.state(0), U.host_state(state, 0), k)
    with pytest.raises(_lib.S2DError, match="4096"):
        tracker.step((cuda(np.zeros((1, 9), np.float32)), cuda(np.zeros(1, np.int64)), cuda(np.ones(1, np.float32)), [0, 1]), pose, [2.0])
    with pytest.raises(_lib.S2DError, match="1024"):
        tracker.step((cuda(np.zeros((1025, 9), np.float32)), cuda(np.zeros(1025, np.int64)), cuda(np.ones(1025, np.float32)), [0, 1025]), pose, [2.0])
    with pytest.raises(ValueError, match="7-column"):
        tracker.step([dict(box3d_lidar=cuda(np.zeros((2, 7), np.float32)), label_preds=cuda(np.zeros(2, np.int64)), scores=cuda(np.ones(2, np.float32)))],
                     pose, [2.0])
    U.same_state(tracker.state(0), U.host_state(state, 0), "after the refused steps")


# ---- targeted cases ------------------------------------------------------------------------------------------------------------------
def _frame(xy, label=0, score=0.9):
    boxes = np.zeros((len(xy), 9), np.float32)
    boxes[:, :2] = xy
    return boxes, np.full(len(xy), label, np.int64), np.full(len(xy), score, np.float32)


def _both(table, max_age, frames_xy, thresh=None):
    """the same frames (identity pose, half-second steps) through the device tracker and the restatement, compared exactly every step"""
    tracker, state, pose = T.Tracker(1, table, max_age, thresh, device=DEV), T.new_state(1), np.eye(4)[None]
    out = []
    for k, xy in enumerate(frames_xy):
        boxes, labels, scores = _frame(np.asarray(xy, np.float64).reshape(-1, 2))
        off = [0, len(boxes)]
        want = T.step_host(state, boxes, labels, scores, off, pose, [0.5 if k else 0.0], [k == 0], None, table, max_age, thresh)
        tid, act, _ = tracker.step((cuda(boxes), cuda(labels), cuda(scores), off), pose, [0.5 * k])
        assert np.array_equal(tid.cpu().numpy(), want[0]) and np.array_equal(act.cpu().numpy(), want[1]), k
        U.same_state(tracker.state(0), U.host_state(state, 0), k)
        out.append((want[0], want[1]))
    return out


def test_contention_takes_the_recompute_path():
    rng = np.random.RandomState(5)
    # 64 detections within range of the same 2 tracks: the first two that come take them, whichever they prefer
    crowd = U._snap(rng.uniform(-1.0, 2.0, (64, 2)))
    out = _both([(0, 5.0)], 3, [[(0.0, 0.0), (1.0, 0.0)], crowd])
    tid, act = out[1]
    assert sorted(tid[:2].tolist()) == [1, 2] and act[:2].tolist() == [2, 2] and tid[2:].tolist() == list(range(3, 65))
    # 300 detections over 300 tracks of one class packed in 10 m with a 5 m gate: most first choices are taken already
    a, b = U._snap(rng.uniform(0, 10, (300, 2))), U._snap(rng.uniform(0, 10, (300, 2)))
    out = _both([(0, 5.0)], 3, [a, b, a])
    assert (out[1][1] == 2).sum() >= 290 and (out[2][1] == 3).sum() >= 280


def test_exact_ties_go_to_the_lower_index():
    out = _both([(0, 5.0)], 3, [[(2.0, 0.0), (-2.0, 0.0), (0.0, 2.0), (0.0, -2.0)], [(0.0, 0.0)], [(0.0, 3.0), (0.0, 3.0)]])
    assert out[1][0].tolist() == [1]                 # four tracks at distance 2: index 0
    assert out[2][0].tolist() == [3, 1]              # both prefer id 3 at (0, 2); the second finds it taken and recomputes: id 1 at (0, 0)
    out = _both([(0, 5.0)], 3, [[(3.0, 4.0), (-3.0, 4.0), (5.0, 0.0)], [(0.0, 0.0), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0)]])
    assert out[1][0].tolist() == [1, 2, 3, 4]        # three tracks at distance exactly 5 = the gate (not beyond it), taken in index order


def _random_step_inputs(seed, segments, n=65):
    seqs = [U.random_sequence(seed + s, lambda f: n, frames=3) for s in range(segments)]
    return [U.pack([q[k] for q in seqs]) for k in range(3)]


def _drive(tracker, steps, **flags):
    out = []
    for k, (boxes, labels, scores, off, poses, stamps) in enumerate(steps):
        kw = {name: v[k] for name, v in flags.items()}
        out.append(tracker.step((cuda(boxes), cuda(labels), cuda(scores), off), poses, stamps, **kw))
    return out


def test_skip_leaves_the_segment_bit_for_bit():
    steps = _random_step_inputs(40, 3)
    tracker = T.Tracker(3, U.RANDOM_TABLE, 3, None, device=DEV)
    _drive(tracker, steps[:2])
    before = [t.clone() for t in tracker.buffers()]
    boxes, labels, scores, off, poses, stamps = steps[2]
    tid, act, _ = tracker.step((cuda(boxes), cuda(labels), cuda(scores), off), poses, stamps, skip=[False, True, False])
    after = tracker.buffers()
    for b, a in zip(before, after):
        assert torch.equal(b[1], a[1]) and not torch.equal(b[0], a[0]) and not torch.equal(b[2], a[2])
    lo, hi = int(off[1]), int(off[2])
    assert (tid[lo:hi] == -1).all() and (act[lo:hi] == 0).all() and (tid[:lo] > 0).any()
    # the skipped segment goes on from where it was: the same step later gives what an unskipped tracker gives
    reference = T.Tracker(3, U.RANDOM_TABLE, 3, None, device=DEV)
    _drive(reference, steps)
    tracker.step((cuda(boxes), cuda(labels), cuda(scores), off), poses, stamps, skip=[True, False, True])
    for r, t in zip(reference.buffers(), tracker.buffers()):
        assert torch.equal(r[1], t[1])


def test_first_resets_the_ids():
    steps = _random_step_inputs(50, 2)
    tracker = T.Tracker(2, U.RANDOM_TABLE, 3, None, device=DEV)
    out = _drive(tracker, steps, first=[[True, True], [False, False], [False, True]])
    tid, off = out[2][0].cpu().numpy(), steps[2][3]
    kept = np.array([U.RANDOM_TABLE[l][0] >= 0 for l in steps[2][1]])
    second = tid[off[1]:off[2]][kept[off[1]:off[2]]]
    assert second.tolist() == list(range(1, len(second) + 1))          # reset: every kept row is a new track, ids from 1
    assert tracker.state(1)["id_count"] == len(second) and len(tracker.state(1)["ids"]) == len(second)
    assert tracker.state(0)["id_count"] > kept[:off[1]].sum()           # the other segment went on counting


def test_two_runs_give_the_same_bits():
    steps = _random_step_inputs(60, 3, n=257)
    a, b = T.Tracker(3, U.RANDOM_TABLE, 3, 0.5, device=DEV), T.Tracker(3, U.RANDOM_TABLE, 3, 0.5, device=DEV)
    for x, y in zip(_drive(a, steps), _drive(b, steps)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])
    for x, y in zip(a.buffers(), b.buffers()):
        assert torch.equal(x, y)


def test_center_head_predict_dictionaries():
    """Tracker.step on the dictionaries of a CenterHead.predict device call equals step_host on their host copies.  The decoded boxes are
    no grid values, so no margin is asserted: both sides evaluate the same IEEE float64 operations one by one on the same float32 boxes (the
    library is built with contraction off, numpy does not contract), hence the same float32 centres and the same decisions."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import predict_tasks_util as P
    from sparse2dense_amd.heads import CenterHead
    tasks = [dict(num_class=3, class_names=["a", "b", "c"])]
    head = CenterHead(in_channels=64, tasks=tasks, dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10, common_heads=P.COMMON_HEADS).eval()
    maps = [{k: v.cuda() for k, v in P.seeded_task_maps(3, 77, 37, 45, 2, False, vel=True).items()}]
    cfg = dict(P.CFG, double_flip=False, circular_nms=False, min_radius=[2.0], post_center_limit_range=[-100.0, -100.0, -10.0, 100.0, 100.0, 10.0])
    dets = head.predict({}, maps, cfg)
    assert head.predict_paths["device"] == 1 and len(dets) == 2 and all(d["box3d_lidar"].is_cuda and d["box3d_lidar"].shape[1] == 9 for d in dets)
    table = [(0, 2.0), (1, 1.0), (-1, 0.0)]
    tracker, state = T.Tracker(2, table, 3, 0.2, device=DEV), T.new_state(2)
    rng = np.random.RandomState(3)
    host = [{k: d[k].cpu().numpy() for k in ("box3d_lidar", "label_preds", "scores")} for d in dets]
    off = np.cumsum([0] + [len(h["scores"]) for h in host])
    assert off[-1] >= 20
    cat = lambda k: np.concatenate([h[k] for h in host], 0)
    last = np.zeros(2)
    for k in range(3):   # the same detections under three poses a little apart: the second and third steps match
        poses = np.stack([U.random_pose(rng) for _ in range(2)])
        poses[:, :2, 3] = [[100.0, -50.0], [-30.0, 20.0]]
        poses[:, :2, :2] = np.eye(2)
        poses[:, 0, 3] += 0.125 * k
        stamps = np.array([10.0, 20.0]) + 0.5 * k
        lag = np.where(k == 0, 0.0, stamps - last)
        last = stamps
        want_tid, want_act = T.step_host(state, cat("box3d_lidar"), cat("label_preds"), cat("scores"), off, poses, lag, [k == 0] * 2, None, table, 3, 0.2)
        tid, act, got_off = tracker.step(dets, poses, stamps)
        assert got_off.tolist() == off.tolist()
        assert np.array_equal(tid.cpu().numpy(), want_tid) and np.array_equal(act.cpu().numpy(), want_act), k
        for s in range(2):
            U.same_state(tracker.state(s), U.host_state(state, s), (k, s))
    assert (want_act >= 2).any()
