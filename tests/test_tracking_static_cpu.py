"""Host side of the static tracker step (tracking.StaticTracker, pack_padded, s2d_track_step_static): the host definition of the step -
`step_host` on `pack_padded(...)` - against the golden of the reference's two trackers with trap rows in the padding; what the class
refuses, before any HIP call, so all of it runs without a GPU; and the C boundary of the new entry."""
import os
import re

import numpy as np
import pytest
import torch

import tracking_util as U
from tracking_static_util import padded
from sparse2dense_amd import _lib, tracking as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = [(0, 1.0), (-1, 0.0)]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return U.load_golden(golden_dir)


@pytest.fixture
def no_hip(monkeypatch):
    """a refusal must come before the library is even loaded"""
    def load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("tag", ["w", "n"])
def test_step_host_on_pack_padded_equals_the_reference(golden, tag):
    table, thresh, _ = U.flavour(golden, tag)
    trap = next(l for l, (c, _) in enumerate(table) if c >= 0)
    fr = U.frames(golden, tag)
    cap = max(len(f["boxes"]) for f in fr) + 3
    state, last = T.new_state(1), None
    for f in fr:
        lag = 0.0 if f["first"] else f["stamp"] - last
        last = f["stamp"]
        boxes, labels, scores, off = T.pack_padded(*padded([f], cap, trap))
        assert off.tolist() == [0, len(f["boxes"])] and boxes.shape == (len(f["boxes"]), 9) and not np.isnan(boxes).any()
        tid, act = T.step_host(state, boxes, labels, scores, off, f["pose"][None], [lag], [f["first"]], [False], table, U.MAX_AGE, thresh)
        U.check_step(golden, tag, f["index"], tid, act, U.host_state(state, 0))


def test_pack_padded_clamps_the_counts_and_checks_the_shapes():
    boxes = np.arange(2 * 3 * 9, dtype=np.float32).reshape(2, 3, 9)
    labels, scores = np.arange(6).reshape(2, 3), np.arange(6, dtype=np.float32).reshape(2, 3) / 8
    b, l, s, off = T.pack_padded(boxes, labels, scores, [5, -2])
    assert off.tolist() == [0, 3, 3] and np.array_equal(b, boxes[0]) and l.tolist() == [0, 1, 2] and s.dtype == np.float32
    b, l, s, off = T.pack_padded(torch.from_numpy(boxes), torch.from_numpy(labels), torch.from_numpy(scores), torch.tensor([1, 2], dtype=torch.int32))
    assert off.tolist() == [0, 1, 3] and l.tolist() == [0, 3, 4] and np.array_equal(b, np.concatenate([boxes[0, :1], boxes[1, :2]]))
    with pytest.raises(ValueError, match="7-column"):
        T.pack_padded(np.zeros((2, 3, 7), np.float32), labels, scores, [1, 1])
    with pytest.raises(ValueError):
        T.pack_padded(boxes, labels[:1], scores, [1, 1])


def test_the_class_refuses_before_any_hip_call(no_hip):
    with pytest.raises(_lib.S2DError, match="65 samples"):
        T.StaticTracker(65, 16, TABLE, 3, device="cuda")
    with pytest.raises(_lib.S2DError, match="0 samples"):
        T.StaticTracker(0, 16, TABLE, 3, device="cuda")
    with pytest.raises(_lib.S2DError, match="cap 1025"):
        T.StaticTracker(1, 1025, TABLE, 0, device="cuda")
    with pytest.raises(_lib.S2DError, match="cap 0"):
        T.StaticTracker(1, 0, TABLE, 0, device="cuda")
    with pytest.raises(_lib.S2DError, match=r"cap 1024 x \(max_age 4 \+ 1\) = 5120 tracks"):
        T.StaticTracker(1, 1024, TABLE, 4, device="cuda")
    with pytest.raises(_lib.S2DError, match="4097 tracks"):
        T.StaticTracker(1, 241, TABLE, 16, device="cuda")
    with pytest.raises(_lib.S2DError, match="CUDA device expected"):
        T.StaticTracker(1, 16, TABLE, 3, device="cpu")
    with pytest.raises(_lib.S2DError, match="labels"):
        T.StaticTracker(1, 16, [], 3, device="cuda")
    with pytest.raises(NotImplementedError):
        T.StaticTracker(1, 16, TABLE, 3, device="cuda", hungarian=True)
    with pytest.raises(NotImplementedError):
        T.StaticTracker.nuscenes(16, device="cuda", hungarian=True)
    with pytest.raises(_lib.S2DError, match="CUDA device expected"):
        T.StaticTracker.waymo(dict(VEHICLE=0.8, PEDESTRIAN=0.4, CYCLIST=0.6), 16, device="cpu")
    with pytest.raises(_lib.S2DError, match="CUDA device expected"):
        T.StaticTracker.nuscenes(16, device="cpu")


def test_constants_and_the_frame_block_layout():
    assert (T.STATIC_STEP_LAUNCHES, T.STATIC_STEP_HOST_READS, T.STATIC_STEP_UPLOADS) == (1, 0, 1)
    assert T._FRAME.itemsize == 112 and T._FRAME.names == ("pose", "stamp", "first", "skip")
    assert [T._FRAME.fields[n][1] for n in T._FRAME.names] == [0, 96, 104, 108]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s2d.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*s2d_track_frame;", src)
    assert body and [f.strip() for f in body.group(1).split(";") if f.strip()] == ["double pose[12]", "double stamp", "int32_t first, skip"]
    tracks = T.StaticTracks(torch.full((2, 3), -1, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32))
    tracks.tracking_id[0, :2] = torch.tensor([4, 7], dtype=torch.int32)
    det = (torch.arange(2 * 3 * 9, dtype=torch.float32).reshape(2, 3, 9), torch.tensor([[1, 0, 5], [5, 5, 5]]), torch.ones(2, 3),
           torch.tensor([2, 0], dtype=torch.int32))
    out = tracks.as_list(det, ["a", "b"])
    assert [sorted(d) for d in out] == [["active", "box3d_lidar", "label_preds", "metadata", "scores", "tracking_id"]] * 2
    assert out[0]["tracking_id"].tolist() == [4, 7] and out[0]["label_preds"].tolist() == [1, 0] and out[0]["box3d_lidar"].shape == (2, 9)
    assert out[1]["tracking_id"].shape == (0,) and out[1]["active"].shape == (0,) and [d["metadata"] for d in out] == ["a", "b"]


def test_header_and_binding_agree_on_the_entry():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "s2d.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+s2d_track_step_static\s*\(([^;]*)\)\s*;", src)
    assert decl
    params = [p.strip() for p in decl.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["s2d_track_step_static"]
    assert restype is _lib.ctypes.c_int and len(params) == len(argtypes) == 20
    for p, a in zip(params, argtypes):
        if "*" in p or p.startswith("s2d_stream_t"):
            assert a is _lib.ctypes.c_void_p, p
        else:
            assert a is (_lib.ctypes.c_float if p.startswith("float") else _lib.ctypes.c_int), p


def test_the_entry_refuses_bad_arguments_without_a_device():
    """the library loads without a GPU; every refusal comes before any HIP call and names its argument"""
    from sparse2dense_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    keep = np.zeros(64, np.uint8)   # any non-null address: a refused call never reads it
    p = keep.ctypes.data

    def call(segments=2, cap=16, labels=3, max_age=3, null=None):
        ptrs = dict.fromkeys(("boxes", "labels", "scores", "counts", "frames", "table", "ct", "tracking", "meta", "head", "parity", "prev_stamp",
                              "tracking_id", "active"), p)
        if null:
            ptrs[null] = None
        return lib.s2d_track_step_static(ptrs["boxes"], ptrs["labels"], ptrs["scores"], ptrs["counts"], segments, cap, ptrs["frames"], ptrs["table"],
                                         labels, max_age, -1.0, ptrs["ct"], ptrs["tracking"], ptrs["meta"], ptrs["head"], ptrs["parity"],
                                         ptrs["prev_stamp"], ptrs["tracking_id"], ptrs["active"], None)
    cases = [(dict(segments=65), "65 segments"), (dict(segments=0), "0 segments"), (dict(cap=0), "cap 0"), (dict(cap=1025), "cap 1025"),
             (dict(cap=241, max_age=16), "4097 tracks"), (dict(cap=1024, max_age=4), "5120 tracks"), (dict(max_age=-1), "max_age -1"),
             (dict(labels=0), "0 labels"), (dict(labels=128), "128 labels"), (dict(null="counts"), "null boxes, labels, scores, counts"),
             (dict(null="boxes"), "null boxes"), (dict(null="active"), "row outputs"), (dict(null="frames"), "null frame block"),
             (dict(null="table"), "label table"), (dict(null="parity"), "parity"), (dict(null="prev_stamp"), "prev_stamp"),
             (dict(null="meta"), "null state buffer")]
    for bad, word in cases:
        assert call(**bad) == -1 and word in _lib.last_error(), (bad, _lib.last_error())
