"""The static tracker step on the device (s2d_track_step_static through tracking.StaticTracker): padded rows with device counts, the time
lag and the buffer parity formed on the device, one launch, capturable.  Against the golden of the reference's two trackers; bit for bit
against the existing device tracker (`Tracker.step` on the packed rows: the same association code behind another entry) at the sizes
where the kernel changes path - a wave of 64 rows or tracks and its neighbours, the 1024-row limit, the largest plan the static bound
accepts (cap 1024 x (max_age 3 + 1) = 4096); skip, first, the empty frame, bit-equal repetition; no synchronisation and no allocation in `run`; one
captured HIP graph of the tracker alone and one of predict and track together, replayed.

The padding of every input below is a trap: the rows behind counts[s] hold NaN boxes, a label that IS a tracking class and score 1.0, so
any read past the count changes ids or the track list.

Both sides of a bit-for-bit comparison run the same device function on the same float32 boxes, float64 poses and float64 time lag
(`stamp - previous stamp` in double on both sides), so no margin is needed and none is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

import tracking_util as U
from tracking_static_util import padded
from sparse2dense_amd import _lib, tracking as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAP = 0   # label 0 is a tracking class of U.RANDOM_TABLE


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return U.load_golden(golden_dir)


def _empty():
    return dict(boxes=np.zeros((0, 9), np.float32), labels=np.zeros(0, np.int64), scores=np.zeros(0, np.float32), pose=np.eye(4), stamp=0.0)


class Static:
    """a StaticTracker with static input tensors of its own: `load` copies one frame per segment into them (trap padding), `step` also
    sets the frame block and launches (or replays the graph that holds the launch)"""

    def __init__(self, segments, cap, table, max_age, thresh, trap=TRAP):
        self.tracker = T.StaticTracker(segments, cap, table, max_age, thresh, device=DEV)
        self.cap, self.trap = cap, trap
        self.det = (torch.zeros(segments, cap, 9, device=DEV), torch.zeros(segments, cap, dtype=torch.int64, device=DEV),
                    torch.zeros(segments, cap, device=DEV), torch.zeros(segments, dtype=torch.int32, device=DEV))
        self.graph = None

    def load(self, frs):
        for dst, src in zip(self.det, padded(frs, self.cap, self.trap)):
            dst.copy_(torch.from_numpy(src))

    def step(self, frs, first=None, skip=None):
        self.load(frs)
        self.tracker.set_frames(np.stack([f["pose"] for f in frs]), [f["stamp"] for f in frs], first, skip)
        if self.graph is None:
            return self.tracker.run(self.det)
        self.graph.replay()
        return self.tracker.out


def _packed(frs):
    boxes, labels, scores, off, poses, stamps = U.pack(frs)
    return (cuda(boxes), cuda(labels), cuda(scores), off), poses, stamps


def _want_padded(tid, act, off, segments, cap, skip=None):
    """the packed outputs of Tracker.step as the padded ones: -1 / 0 behind the counts and in skipped segments"""
    tid, act = tid.cpu(), act.cpu()
    want_tid, want_act = torch.full((segments, cap), -1, dtype=torch.int32), torch.zeros((segments, cap), dtype=torch.int32)
    for s in range(segments):
        if skip is not None and skip[s]:
            continue
        lo, hi = int(off[s]), int(off[s + 1])
        want_tid[s, :hi - lo], want_act[s, :hi - lo] = tid[lo:hi], act[lo:hi]
    return want_tid, want_act


def _assert_outputs(out, tid, act, off, segments, cap, what, skip=None):
    want_tid, want_act = _want_padded(tid, act, off, segments, cap, skip)
    assert out.tracking_id.dtype == out.active.dtype == torch.int32 and out.tracking_id.shape == out.active.shape == (segments, cap), what
    assert torch.equal(out.tracking_id.cpu(), want_tid) and torch.equal(out.active.cpu(), want_act), what


def _assert_lists(static, tracker, segments, what):
    """every segment's current list (the rows below its count) and head, bit for bit"""
    a, b = static.buffers(), tracker.buffers()
    assert torch.equal(a[3], b[3]), what
    for s, count in enumerate(a[3][:, 0].tolist()):
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x[s, :count], y[s, :count]), (what, s)


def _same_state(got, want, what):
    assert got["id_count"] == want["id_count"], what
    for k in ("ids", "classes", "ages", "active", "ct", "tracking"):
        assert np.array_equal(got[k], want[k]), (what, k)


# ---- golden parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["w", "n"])
def test_golden_one_segment(golden, tag):
    table, thresh, _ = U.flavour(golden, tag)
    trap = next(l for l, (c, _) in enumerate(table) if c >= 0)
    fr = U.frames(golden, tag)
    cap = max(len(f["boxes"]) for f in fr) + 5
    st = Static(1, cap, table, U.MAX_AGE, thresh, trap)
    for f in fr:   # (both sequences, one after the other: the second begins with first = 1)
        out = st.step([f], first=[f["first"]])
        n = len(f["boxes"])
        tid, act = out.tracking_id.cpu().numpy()[0], out.active.cpu().numpy()[0]
        assert (tid[n:] == -1).all() and (act[n:] == 0).all()
        U.check_step(golden, tag, f["index"], tid[:n], act[:n], st.tracker.state(0))


@pytest.mark.parametrize("tag", ["w", "n"])
def test_golden_two_sequences_as_two_segments(golden, tag):
    table, thresh, _ = U.flavour(golden, tag)
    trap = next(l for l, (c, _) in enumerate(table) if c >= 0)
    seqs = [U.frames(golden, tag, 0), U.frames(golden, tag, 1)]
    assert len(seqs[0]) != len(seqs[1])
    cap = max(len(f["boxes"]) for q in seqs for f in q) + 5
    st = Static(2, cap, table, U.MAX_AGE, thresh, trap)
    unequal = False
    for k in range(max(len(q) for q in seqs)):
        live = [k < len(q) for q in seqs]
        fr = [q[k] if ok else _empty() for q, ok in zip(seqs, live)]
        out = st.step(fr, first=[k == 0, k == 0], skip=[not ok for ok in live])
        tid, act = out.tracking_id.cpu().numpy(), out.active.cpu().numpy()
        unequal |= all(live) and len(fr[0]["boxes"]) != len(fr[1]["boxes"])
        for s in range(2):   # (a finished sequence is skipped: its last state stays)
            n = len(fr[s]["boxes"])
            assert (tid[s, n:] == -1).all() and (act[s, n:] == 0).all()
            index = fr[s]["index"] if live[s] else seqs[s][-1]["index"]
            if live[s]:
                U.check_step(golden, tag, index, tid[s, :n], act[s, :n], st.tracker.state(s))
            else:
                want = golden[f"{tag}_tracks"][golden[f"{tag}_track_offsets"][index]:golden[f"{tag}_track_offsets"][index + 1]]
                assert np.array_equal(st.tracker.state(s)["ids"], want[:, 0].astype(np.int64))
    assert unequal


# ---- bit for bit the existing device tracker -------------------------------------------------------------------------------------------
def _rows_plan(n, segments):
    """segment 0 and the last one see n rows every frame; the others walk through the small sizes"""
    return lambda s, f: n if s in (0, segments - 1) else U.SMALL_SIZES[(s + f) % len(U.SMALL_SIZES)]


@pytest.mark.parametrize("segments", [1, 3, 64])
@pytest.mark.parametrize("max_age", [0, 3])
@pytest.mark.parametrize("n", U.SIZES)
def test_random_sequences_equal_tracker_step(n, max_age, segments):
    thresh = 0.5 if max_age else None
    plan, cap = _rows_plan(n, segments), 1024
    seqs = [U.random_sequence(1000 + s, lambda f, s=s: plan(s, f)) for s in range(segments)]
    st, tracker = Static(segments, cap, U.RANDOM_TABLE, max_age, thresh), T.Tracker(segments, U.RANDOM_TABLE, max_age, thresh, device=DEV)
    peak = 0
    for k in range(6):
        frs = [q[k] for q in seqs]
        dets, poses, stamps = _packed(frs)
        tid, act, _ = tracker.step(dets, poses, stamps, first=[k == 0] * segments)
        out = st.step(frs, first=[k == 0] * segments)
        _assert_outputs(out, tid, act, dets[3], segments, cap, (n, max_age, segments, k))
        for a, b in zip(st.tracker.buffers(), tracker.buffers()):   # the whole current half: both sides wrote the same rows from zero
            assert a.shape == b.shape and torch.equal(a, b), (n, max_age, segments, k)
        peak = max(peak, int(tracker.buffers()[3][:, 0].max()))
    assert st.tracker._parity.tolist() == [0] * segments   # six steps: every segment is back on half 0
    if n >= 257 and max_age:
        assert peak > 256   # the track lists cross a wave (64) and 256 on their way up
    if n >= 63 and max_age:
        assert peak > 64


def test_full_frames_at_the_static_bound():
    """cap 1024, max_age 3 (cap x (max_age + 1) = 4096, the largest plan the bound accepts): frames of 1024 rows that match nothing leave
    1024, 2048 and then 3072 tracks - a track lives max_age frames - with the oldest 1024 dropped at every further step"""
    table = [(0, 0.25)]
    st, tracker, state = Static(1, 1024, table, 3, None), T.Tracker(1, table, 3, None, device=DEV), T.new_state(1)
    for k in range(5):
        boxes = np.zeros((1024, 9), np.float32)
        boxes[:, 0], boxes[:, 1] = np.arange(1024) % 32 * 4.0 + k, np.arange(1024) // 32 * 4.0   # frame k is shifted by k m: no match at 0.25 m
        f = dict(boxes=boxes, labels=np.zeros(1024, np.int64), scores=np.ones(1024, np.float32), pose=np.eye(4), stamp=0.5 * k)
        want = T.step_host(state, boxes, f["labels"], f["scores"], [0, 1024], f["pose"][None], [0.5 if k else 0.0], [k == 0], None, table, 3)
        out = st.step([f])
        assert np.array_equal(out.tracking_id.cpu().numpy()[0], want[0]) and np.array_equal(out.active.cpu().numpy()[0], want[1])
        assert int(state["head"][0, 0]) == 1024 * min(k + 1, 3)
        U.same_state(st.tracker.state(0), U.host_state(state, 0), k)
        tid, act, _ = tracker.step(_packed([f])[0], f["pose"][None], [f["stamp"]])
        _assert_outputs(out, tid, act, [0, 1024], 1, 1024, k)
        _assert_lists(st.tracker, tracker, 1, k)


# ---- skip, first, the empty frame ------------------------------------------------------------------------------------------------------
def test_skip_keeps_parity_state_and_stamp():
    segments, cap = 3, 80
    seqs = [U.random_sequence(40 + s, lambda f: 65, frames=4) for s in range(segments)]
    st, tracker = Static(segments, cap, U.RANDOM_TABLE, 3, None), T.Tracker(segments, U.RANDOM_TABLE, 3, None, device=DEV)
    flags = [None, None, [False, True, False], None]
    for k in range(4):
        frs = [q[k] for q in seqs]
        dets, poses, stamps = _packed(frs)
        before = {name: t.clone() for name, t in st.tracker.all_buffers().items()}
        tid, act, _ = tracker.step(dets, poses, stamps, skip=flags[k])
        out = st.step(frs, skip=flags[k])
        _assert_outputs(out, tid, act, dets[3], segments, cap, k, flags[k])
        _assert_lists(st.tracker, tracker, segments, k)
        after = st.tracker.all_buffers()
        if k == 2:   # the skipped segment: parity, both halves of the state and the stamp keep every bit; its outputs are all -1 / 0
            for name in ("ct", "tracking", "meta", "head"):
                assert torch.equal(before[name][:, 1], after[name][:, 1]), name
                assert not torch.equal(before[name][:, 0], after[name][:, 0]) and not torch.equal(before[name][:, 2], after[name][:, 2]), name
            assert before["parity"].tolist() == [0, 0, 0] and after["parity"].tolist() == [1, 0, 1]
            assert after["prev_stamp"].tolist() == [seqs[0][2]["stamp"], seqs[1][1]["stamp"], seqs[2][2]["stamp"]]
            assert bool((out.tracking_id[1] == -1).all()) and bool((out.active[1] == 0).all()) and bool((out.tracking_id[0] > 0).any())
        if k == 3:   # its next step measured the lag from its last stepped stamp: the tracking of its new entries is -velocity * that lag
            assert after["parity"].tolist() == [0, 1, 0]
            assert after["prev_stamp"].tolist() == [q[3]["stamp"] for q in seqs]
            lag = seqs[1][3]["stamp"] - seqs[1][1]["stamp"]
            state, f = st.tracker.state(1), seqs[1][3]
            kept = np.array([U.RANDOM_TABLE[l][0] >= 0 for l in f["labels"]])
            vel = f["boxes"][kept][:, 6:8].astype(np.float64) @ f["pose"][:2, :2].T
            fresh = state["ages"] == 1
            assert fresh.sum() == kept.sum() and lag > seqs[1][3]["stamp"] - seqs[1][2]["stamp"]
            got, want = np.sort(state["tracking"][fresh], 0), np.sort(vel * -1 * lag, 0)
            assert np.array_equal(got, want) and np.abs(want).max() > 0


def _one(n, label=0, x0=0.0, vx=0.0, stamp=0.0):
    boxes = np.zeros((n, 9), np.float32)
    boxes[:, 0], boxes[:, 6] = x0 + 10.0 * np.arange(n), vx
    return dict(boxes=boxes, labels=np.full(n, label, np.int64), scores=np.full(n, 0.9, np.float32), pose=np.eye(4), stamp=stamp)


def test_first_the_empty_frame_and_the_all_filtered_frame():
    table = [(0, 1.0), (-1, 0.0)]
    st = Static(1, 8, table, 2, None)
    ids = lambda out, n: out.tracking_id[0, :n].tolist()
    out = st.step([_one(3, stamp=0.0)])
    assert ids(out, 3) == [1, 2, 3] and out.active[0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and out.tracking_id[0, 3:].tolist() == [-1] * 5
    # THE DEVIATION: rows present, all filtered (the reference raises IndexError): every track is unmatched and ages
    out = st.step([_one(2, label=1, stamp=0.5)])
    state = st.tracker.state(0)
    assert out.tracking_id[0].tolist() == [-1] * 8 and out.active[0].tolist() == [0] * 8
    assert state["ids"].tolist() == [1, 2, 3] and state["ages"].tolist() == [2, 2, 2] and state["active"].tolist() == [0, 0, 0] and state["id_count"] == 3
    st.step([_one(2, label=1, stamp=1.0)])
    state = st.tracker.state(0)
    assert len(state["ids"]) == 0 and state["id_count"] == 3   # age 2 is not < max_age
    assert ids(st.step([_one(1, stamp=1.5)]), 1) == [4]
    # counts[s] == 0 clears the tracks and keeps id_count
    out = st.step([_one(0, stamp=2.0)])
    state = st.tracker.state(0)
    assert out.tracking_id[0].tolist() == [-1] * 8 and len(state["ids"]) == 0 and state["id_count"] == 4
    out = st.step([_one(2, vx=1.0, stamp=2.5)])
    state = st.tracker.state(0)
    assert ids(out, 2) == [5, 6] and state["tracking"][:, 0].tolist() == [-0.5, -0.5]   # -velocity * (2.5 - 2.0): the empty frame's stamp counts
    # first: reset() - ids from 1 again, and the lag is 0 whatever the stamps are
    out = st.step([_one(2, vx=1.0, stamp=7.0)], first=[True])
    state = st.tracker.state(0)
    assert ids(out, 2) == [1, 2] and state["id_count"] == 2 and not state["tracking"].any() and st.tracker._prev_stamp.tolist() == [7.0]
    assert st.tracker._parity.tolist() == [1]   # seven steps


def test_two_trackers_driven_identically_give_the_same_bits():
    segments, cap = 3, 300
    seqs = [U.random_sequence(60 + s, lambda f: 257, frames=3) for s in range(segments)]
    a, b = Static(segments, cap, U.RANDOM_TABLE, 3, 0.5), Static(segments, cap, U.RANDOM_TABLE, 3, 0.5)
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t
    for k in range(3):
        frs = [q[k] for q in seqs]
        x, y = a.step(frs, skip=[False, k == 1, False]), b.step(frs, skip=[False, k == 1, False])
        assert torch.equal(x.tracking_id, y.tracking_id) and torch.equal(x.active, y.active) and bool((x.tracking_id > 0).any())
        for (name, p), q in zip(a.tracker.all_buffers().items(), b.tracker.all_buffers().values()):
            assert torch.equal(bits(p), bits(q)), (k, name)
    # the outputs are a function of the inputs alone: the same call again writes the same rows (parity and state moved on)
    before = [t.clone() for t in a.tracker.out]
    a.tracker.set_frames(np.stack([q[2]["pose"] for q in seqs]), [q[2]["stamp"] for q in seqs], skip=[True] * segments)
    out = a.tracker.run(a.det)
    assert bool((out.tracking_id == -1).all()) and bool((out.active == 0).all()) and not torch.equal(before[0], out.tracking_id)


# ---- no host round trip, graph capture ---------------------------------------------------------------------------------------------------
def test_run_neither_synchronises_nor_allocates():
    segments, cap = 3, 80
    seqs = [U.random_sequence(70 + s, lambda f: 65, frames=2) for s in range(segments)]
    st = Static(segments, cap, U.RANDOM_TABLE, 3, 0.5)
    out = st.step([q[0] for q in seqs])   # warm-up: the code object is loaded
    st.load([q[1] for q in seqs])
    st.tracker.set_frames(np.stack([q[1]["pose"] for q in seqs]), [q[1]["stamp"] for q in seqs])
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in st.tracker.all_buffers().items()}
    assert set(ptrs) == {"table", "ct", "tracking", "meta", "head", "parity", "prev_stamp", "frames", "tracking_id", "active"}
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = st.tracker.run(st.det)
        again = st.tracker.run(st.det)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert again is out and again.tracking_id is out.tracking_id and again.active is out.active
    assert {k: v.data_ptr() for k, v in st.tracker.all_buffers().items()} == ptrs
    torch.cuda.synchronize()
    assert st.tracker._parity.tolist() == [1] * segments and bool((out.tracking_id > 0).any())   # three steps were taken


def _capture(run):
    """warm up on a side stream, then record one call of `run` into a graph"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    return graph


def test_one_captured_graph_of_the_tracker_replays_as_the_next_step():
    segments, cap, sizes = 3, 80, (65, 0, 64, 1, 63, 65, 7, 65)
    seqs = [U.random_sequence(80 + s, lambda f, s=s: sizes[(f + s) % 8], frames=8) for s in range(segments)]
    st, tracker = Static(segments, cap, U.RANDOM_TABLE, 3, 0.5), T.Tracker(segments, U.RANDOM_TABLE, 3, 0.5, device=DEV)
    st.load([q[0] for q in seqs])
    st.tracker.set_frames(np.stack([q[0]["pose"] for q in seqs]), [q[0]["stamp"] for q in seqs], skip=[True] * segments)   # the warm-up steps nothing
    st.graph = _capture(lambda: st.tracker.run(st.det))
    assert st.tracker._parity.tolist() == [0] * segments and not st.tracker._head.any()
    matched = False
    for k in range(8):   # DESIGN rule 32's defect showed from the fourth replay on
        frs = [q[k] for q in seqs]
        dets, poses, stamps = _packed(frs)
        tid, act, _ = tracker.step(dets, poses, stamps, first=[k == 0] * segments)
        out = st.step(frs, first=[k == 0] * segments)   # copy_ of the rows and counts, set_frames, one replay
        torch.cuda.synchronize()
        _assert_outputs(out, tid, act, dets[3], segments, cap, k)
        for a, b in zip(st.tracker.buffers(), tracker.buffers()):
            assert torch.equal(a, b), k
        assert st.tracker._parity.tolist() == [(k + 1) % 2] * segments
        for s in range(segments):   # after an odd and after an even number of replays
            _same_state(st.tracker.state(s), tracker.state(s), (k, s))
        matched |= bool((act >= 2).any())
    assert matched


H = W = 40
CLASSES = [1, 2, 2]
PREDICT_TABLE = [(0, 2.0), (1, 2.0), (-1, 0.0), (2, 1.5), (0, 2.0)]   # label -> (tracking class, gate in metres); label 2 is not tracked


def _predict_maps(frame, samples=2):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import predict_tasks_util as P
    peaks = [150, 0 if frame == 3 else 150, 150]   # frame 3 empties task 1's segments: its tracks survive unmatched
    return [{k: v.cuda() for k, v in P.seeded_task_maps(c, (30 + frame) * 1000 + i, H, W, samples, False, vel=True, peaks=peaks[i],
                                                        peak_logit=(-1.0, 2.0)).items()} for i, c in enumerate(CLASSES)]


def test_one_captured_graph_of_predict_and_track():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import predict_tasks_util as P
    from sparse2dense_amd import center_predict
    from sparse2dense_amd.heads import CenterHead
    tasks = [dict(num_class=c, class_names=[f"c{i}_{j}" for j in range(c)]) for i, c in enumerate(CLASSES)]
    head = CenterHead(in_channels=64, tasks=tasks, dataset="nuscenes", weight=0.25, code_weights=[1.0] * 10, common_heads=P.COMMON_HEADS).eval()
    cfg = dict(P.CFG, double_flip=False, circular_nms=False, min_radius=P.CFG["min_radius"][:3],
               nms=dict(nms_pre_max_size=64, nms_post_max_size=83, nms_iou_threshold=0.2), post_center_limit_range=[-100.0, -100.0, -10.0, 100.0, 100.0, 10.0])
    static = [{k: v.clone() for k, v in p.items()} for p in _predict_maps(0)]
    plan = center_predict.StaticPredictPlan(cfg, head.num_classes, 2, H, W, True, static[0]["hm"].device)
    assert plan.cap == 3 * 64
    st, tracker = T.StaticTracker(2, plan.cap, PREDICT_TABLE, 3, 0.2, device=DEV), T.Tracker(2, PREDICT_TABLE, 3, 0.2, device=DEV)
    with pytest.raises(_lib.S2DError, match="built for"):
        T.StaticTracker(2, plan.cap + 1, PREDICT_TABLE, 3, 0.2, device=DEV).run(plan.out)
    poses = np.stack([np.eye(4), np.eye(4)])
    poses[:, :2, 3] = [[100.0, -50.0], [-30.0, 20.0]]
    st.set_frames(poses, [0.0, 0.0], skip=[True, True])   # the warm-up steps nothing
    graph = _capture(lambda: st.run(plan.run(static)))
    assert st._parity.tolist() == [0, 0] and not st._head.any()
    matched = survived = False
    for k in range(6):
        maps = _predict_maps(k)
        for dst, src in zip(static, maps):
            for name in dst:
                dst[name].copy_(src[name])
        poses[:, 0, 3] += 0.125
        stamps = np.array([10.0, 20.0]) + 0.5 * k
        st.set_frames(poses, stamps)
        graph.replay()
        torch.cuda.synchronize()
        want = head.predict({}, maps, cfg)
        tid, act, off = tracker.step(want, poses, stamps)
        counts, off = plan.out.counts.tolist(), off.tolist()
        assert counts == [len(w["scores"]) for w in want] and min(counts) > 0
        for b, n in enumerate(counts):
            assert torch.equal(plan.out.boxes[b, :n], want[b]["box3d_lidar"]), (k, b)
            assert torch.equal(st.out.tracking_id[b, :n], tid[off[b]:off[b + 1]]) and torch.equal(st.out.active[b, :n], act[off[b]:off[b + 1]]), (k, b)
            assert bool((st.out.tracking_id[b, n:] == -1).all()) and bool((st.out.active[b, n:] == 0).all()), (k, b)
        rows = st.out.as_list(plan.out, ["m0", "m1"])
        assert [r["metadata"] for r in rows] == ["m0", "m1"] and all(torch.equal(r["label_preds"], w["label_preds"]) for r, w in zip(rows, want))
        assert torch.equal(torch.cat([r["tracking_id"] for r in rows]), tid)
        matched |= bool((act >= 2).any())
        survived |= any(bool(((tracker.state(s)["active"] == 0) & (tracker.state(s)["ages"] > 1)).any()) for s in range(2))
    for s in range(2):
        _same_state(st.state(s), tracker.state(s), s)
    for a, b in zip(st.buffers(), tracker.buffers()):
        assert torch.equal(a, b)
    assert matched and survived   # a matched detection and a surviving unmatched track were both seen


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def test_bounds():
    from sparse2dense_amd import center_predict
    st = Static(1, 1024, U.RANDOM_TABLE, 3, None)   # cap 1024 x (3 + 1) = 4096: accepted
    f = U.random_sequence(90, lambda f: 65, frames=1)[0]
    out = st.step([f])
    kept = np.array([U.RANDOM_TABLE[l][0] >= 0 for l in f["labels"]])
    assert out.tracking_id[0, :65].cpu()[torch.from_numpy(kept)].tolist() == list(range(1, int(kept.sum()) + 1))
    assert bool((out.tracking_id[0, 65:] == -1).all())
    with pytest.raises(_lib.S2DError, match="cap 1025"):
        T.StaticTracker(1, 1025, U.RANDOM_TABLE, 0, device=DEV)
    with pytest.raises(_lib.S2DError, match="5120 tracks"):
        T.StaticTracker(1, 1024, U.RANDOM_TABLE, 4, device=DEV)
    small = T.StaticTracker(2, 16, U.RANDOM_TABLE, 3, device=DEV)
    det = lambda cap, dim: center_predict.StaticDetections(torch.zeros(2, cap, dim, device=DEV), torch.zeros(2, cap, device=DEV),
                                                           torch.zeros(2, cap, dtype=torch.int64, device=DEV),
                                                           torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="7-column"):
        small.run(det(16, 7))
    with pytest.raises(_lib.S2DError, match="built for"):   # a plan whose cap differs from the tracker's
        small.run(det(17, 9))
    d = det(16, 9)
    with pytest.raises(_lib.S2DError, match="labels is torch.int32"):
        small.run((d.boxes, d.labels.int(), d.scores, d.counts))
    with pytest.raises(_lib.S2DError, match="not contiguous"):
        small.run((torch.zeros(2, 9, 16, device=DEV).permute(0, 2, 1), d.labels, d.scores, d.counts))
    with pytest.raises(_lib.S2DError, match="on cpu"):
        small.run((d.boxes, d.labels, d.scores, d.counts.cpu()))
    with pytest.raises(ValueError, match="first=True"):
        small.set_frames(np.stack([np.eye(4)] * 2), [0.0, 0.0], first=[True, False])
    assert small._parity.tolist() == [0, 0] and not small._head.any()   # nothing was launched
    small.set_frames(np.stack([np.eye(4)] * 2), [0.0, 0.0])
    out = small.run(det(16, 9))   # zero counts: two empty frames
    assert bool((out.tracking_id == -1).all()) and small._parity.tolist() == [1, 1]
