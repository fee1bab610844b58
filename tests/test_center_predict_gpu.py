"""CenterHead.predict on the device (csrc/center_predict.hip, center_predict.py, nms.*_batched) against the float64 restatement
(tests/predict_ref.py), the per-segment torch chain it replaces (CenterHead.predict_torch), the reference's recorded outputs and
oracle.iou_nms.  Every input set is first checked in the restatement to keep clear of each decision a last-ulp difference could flip
(predict_ref.Margins.check), so keep lists are compared exactly."""
import os
import sys

import numpy as np
import pytest
import torch

import predict_ref as R
from oracle import iou_nms as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import predict_tasks_util as U   # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 37, 45
CLASSES = {1: [3], 3: [1, 2, 2], 6: [1, 2, 2, 1, 2, 2]}
# seeds picked on the CPU (predict_ref.Margins.check holds for the rotated and the circular configuration): (tasks, double_flip) -> seed
GRID_SEEDS = {(1, False): 1, (1, True): 1, (3, False): 1, (3, True): 2, (6, False): 1, (6, True): 6}
WIDE = [-100.0, -100.0, -10.0, 100.0, 100.0, 10.0]


def _head(classes, vel):
    from sparse2dense_amd.heads import CenterHead
    heads = {k: v for k, v in U.COMMON_HEADS.items() if vel or k != "vel"}
    tasks = [dict(num_class=c, class_names=[f"c{i}_{j}" for j in range(c)]) for i, c in enumerate(classes)]
    return CenterHead(in_channels=64, tasks=tasks, dataset="nuscenes", weight=0.25, code_weights=[1.0] * (10 if vel else 8), common_heads=heads).eval()


def _cfg(tasks, flip, circular, **over):
    radii = U.CFG["min_radius"][:tasks] if tasks > 1 else [2.0]
    cfg = dict(U.CFG, double_flip=flip, circular_nms=circular, min_radius=radii)
    cfg.update(over)
    return cfg


def _maps(classes, seed, flip, vel, h=H, w=W, samples=2, **kw):
    return [U.seeded_task_maps(c, seed * 1000 + i, h, w, samples, flip, vel=vel, **kw) for i, c in enumerate(classes)]


def _cuda(maps):
    return [{k: v.cuda() for k, v in p.items()} for p in maps]


def _np(maps):
    return [{k: v.float().numpy() for k, v in p.items()} for p in maps]


def _same(got, want, what):
    """the bars of the existing predict tests: labels, box count and keep order exactly; scores rtol 1e-5; boxes rtol 1e-4, atol 2e-4"""
    assert len(got) == len(want), what
    for i, (g, r) in enumerate(zip(got, want)):
        g = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in g.items()}
        r = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}
        assert g["box3d_lidar"].shape == r["box3d_lidar"].shape, (what, i, g["box3d_lidar"].shape, r["box3d_lidar"].shape)
        assert g["label_preds"].dtype == np.int64 and g["scores"].dtype == np.float32 and g["box3d_lidar"].dtype == np.float32
        assert np.array_equal(g["label_preds"], r["label_preds"]), (what, i)
        np.testing.assert_allclose(g["scores"], r["scores"], rtol=1e-5, err_msg=f"{what} {i}")
        np.testing.assert_allclose(g["box3d_lidar"], r["box3d_lidar"], rtol=1e-4, atol=2e-4, err_msg=f"{what} {i}")


def _run_both(head, maps, cfg, example=None):
    """(device path, torch chain) of the same head on the same maps; asserts that predict() took the device path"""
    before = dict(head.predict_paths)
    dev = head.predict(example or {}, _cuda(maps), cfg)
    assert head.predict_paths == dict(before, device=before["device"] + 1), head.predict_paths
    old = head.predict_torch(example or {}, _cuda(maps), cfg)
    return dev, old


@pytest.mark.parametrize("circular", [False, True], ids=["rotated", "circular"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "double_flip"])
@pytest.mark.parametrize("vel", [True, False], ids=["vel", "no_vel"])
@pytest.mark.parametrize("tasks", [1, 3, 6])
def test_device_path_matches_restatement_and_old_chain(tasks, vel, flip, circular):
    classes = CLASSES[tasks]
    cfg = _cfg(tasks, flip, circular)
    maps = _maps(classes, GRID_SEEDS[tasks, flip], flip, vel)
    want, margins = R.predict(_np(maps), cfg)
    margins.check()
    assert min(margins.candidates) >= 30 and sum(len(w["scores"]) for w in want) < sum(margins.candidates)   # the NMS does suppress
    head = _head(classes, vel)
    dev, old = _run_both(head, maps, cfg, example={"metadata": [f"m{i}" for i in range(maps[0]["hm"].shape[0])]})
    assert dev[0]["box3d_lidar"].shape[1] == (9 if vel else 7) and dev[0]["box3d_lidar"].is_cuda
    assert [d["metadata"] for d in dev] == [d["metadata"] for d in old] == (["m0", "m4"] if flip else ["m0", "m1"])
    _same(dev, want, "device vs restatement")
    _same(dev, old, "device vs torch chain")


def test_device_path_matches_both_reference_goldens(golden_dir):
    from golden_util import PREDICT_FLIP_CIRCLE_CFG, predict_flip_circle_inputs
    from sparse2dense_amd import waymo_configs
    from sparse2dense_amd.registry import build_head
    cases = [(_head(CLASSES[6], True), U.predict_tasks_inputs(), U.CFG, "predict_tasks_flip_circle.npz"),
             (build_head(waymo_configs.centerpoint_voxelnet()["bbox_head"]).eval(), [predict_flip_circle_inputs()], PREDICT_FLIP_CIRCLE_CFG,
              "predict_flip_circle.npz")]
    for head, maps, cfg, name in cases:
        g = np.load(os.path.join(golden_dir, name))
        out = head.predict({}, _cuda(maps), cfg)
        assert head.predict_paths == {"device": 1, "torch": 0}
        _same(out, [dict(box3d_lidar=g[f"boxes{i}"], scores=g[f"scores{i}"], label_preds=g[f"labels{i}"]) for i in range(int(g["samples"]))], name)


# ---- edges: each against the torch chain (and the restatement's margins) ------------------------------------------------------------------
# name -> classes, generator arguments, test_cfg changes, expected candidates per segment (None: not pinned); seeds picked on the CPU
ALL_PASS = dict(peak_logit=(-1.0, 2.0))   # every peak above the 0.1 threshold
EDGES = {
    "empty_segment": dict(classes=[2, 1], seed=3, task_peaks=[None, 0], cfg=dict(circular_nms=False)),
    "empty_call": dict(classes=[2, 1], seed=3, gen=dict(peaks=0), cfg=dict(circular_nms=False), counts=0),
    "empty_call_circular": dict(classes=[2], seed=3, gen=dict(peaks=0), flip=True, counts=0),
    "one_candidate": dict(classes=[2], seed=3, gen=dict(peaks=1, **ALL_PASS), cfg=dict(post_center_limit_range=WIDE, circular_nms=False), counts=1),
    "64_candidates": dict(classes=[2], seed=3, gen=dict(peaks=64, **ALL_PASS), cfg=dict(post_center_limit_range=WIDE, circular_nms=False), counts=64),
    "65_candidates": dict(classes=[2], seed=3, gen=dict(peaks=65, **ALL_PASS), cfg=dict(post_center_limit_range=WIDE, circular_nms=False), counts=65),
    "pre_max_cut": dict(classes=[2, 1], seed=3, gen=dict(peaks=300, **ALL_PASS), flip=True,
                        cfg=dict(post_center_limit_range=WIDE, circular_nms=False, nms=dict(nms_pre_max_size=64, nms_post_max_size=83, nms_iou_threshold=0.2)),
                        counts=300),
    "post_max_cut": dict(classes=[2, 1], seed=3, gen=dict(peaks=300, **ALL_PASS),
                         cfg=dict(min_radius=[0.175, 0.175], nms=dict(nms_pre_max_size=1000, nms_post_max_size=20, nms_iou_threshold=0.2)), kept=20),
    "no_range": dict(classes=[1, 2], seed=3, flip=True, cfg=dict(post_center_limit_range=[], circular_nms=False)),
    "channels_last": dict(classes=[3, 2], seed=3, flip=True, cfg=dict(circular_nms=False), layout="channels_last"),
    "bf16": dict(classes=[2, 1], seed=3, gen=dict(peaks=12), cfg=dict(circular_nms=False), dtype=torch.bfloat16),
    "nan_logits": dict(classes=[2, 3], seed=3, flip=True, cfg=dict(circular_nms=False), nan=True),
    "one_pixel": dict(classes=[2], seed=3, h=1, w=1, gen=dict(peaks=1, peak_logit=(1.0, 2.0)), flip=True, cfg=dict(post_center_limit_range=WIDE), counts=1),
}


def edge_inputs(name):
    """(classes, maps on the CPU as the head would produce them, test_cfg) of one edge"""
    e = EDGES[name]
    classes, flip = e["classes"], e.get("flip", False)
    h, w = e.get("h", H), e.get("w", W)
    maps = []
    for i, c in enumerate(classes):
        gen = dict(e.get("gen", {}))
        if "task_peaks" in e and e["task_peaks"][i] is not None:
            gen["peaks"] = e["task_peaks"][i]
        maps.append(U.seeded_task_maps(c, e["seed"] * 1000 + i, h, w, 2, flip, **gen))
    if e.get("nan"):   # NaN logits at a few cells of every image, peaks among them: torch drops such a cell, and so must the kernel
        for p in maps:
            hm = p["hm"].reshape(p["hm"].shape[0], p["hm"].shape[1], -1)
            peaks = (hm[0].max(0).values > -3).nonzero()[:4, 0]
            hm[:, 0, peaks] = float("nan")
            hm[:, -1, 5::97] = float("nan")
    if "dtype" in e:
        maps = [{k: v.to(e["dtype"]) for k, v in p.items()} for p in maps]
    cfg = _cfg(len(classes), flip, True, **e.get("cfg", {}))
    return classes, maps, cfg


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_match_the_old_chain(name):
    from sparse2dense_amd import center_predict
    e = EDGES[name]
    classes, maps, cfg = edge_inputs(name)
    want, margins = R.predict(_np(maps), cfg)   # (bf16 maps: the restatement sees the rounded values, as both paths do)
    margins.check()
    if "counts" in e:
        assert set(margins.candidates) == {e["counts"]}, margins.candidates
    if name == "empty_segment":
        assert 0 in margins.candidates and max(margins.candidates) > 30
    if name == "nan_logits":
        assert all(np.isnan(p["hm"]).sum() > 20 for p in _np(maps))
    head = _head(classes, True)
    dev_maps = maps
    if e.get("layout") == "channels_last":
        dev_maps = [{k: v.cuda().contiguous(memory_format=torch.channels_last) for k, v in p.items()} for p in maps]
        assert not dev_maps[0]["hm"].is_contiguous()
    dev, old = _run_both(head, dev_maps, cfg)
    if "counts" in e:
        cand = center_predict.decode_center_maps(_cuda(maps), cfg, cfg["double_flip"])
        assert cand.passed == [e["counts"]] * len(cand.passed), cand.passed
    if "kept" in e:   # more survivors than nms_post_max_size in every segment
        assert [len(d["scores"]) for d in dev] == [e["kept"] * len(classes)] * 2
    if name.startswith("empty_call"):
        assert all(d["box3d_lidar"].shape == (0, 9) and d["scores"].shape == (0,) and d["label_preds"].dtype == torch.int64 for d in dev)
    _same(dev, old, name)
    _same(dev, want, name + " (restatement)")


# ---- the batched NMS entries alone ---------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 700, 0, 4097)
RADII = (1.0, 0.5, 2.0, 9.0, 0.25, 1.5, 3.0, 9.0)
IOU_THRESHOLD = 0.25
NMS_SEED = 43   # picked on the CPU: the pair margins asserted in _packed_segments hold


def _packed_segments(width=9, seed=NMS_SEED, _cache={}):
    """boxes of SIZES segments, each sorted by descending score, packed; x y z dx dy dz (filler) heading.  As in the predict tests, no
    pair may lie within 1e-4 of the IoU threshold or within a relative 1e-4 of its segment's radius: asserted here, once."""
    if (width, seed) not in _cache:
        per_seg, margins = [], []
        for s, n in enumerate(SIZES):
            rs = np.random.RandomState(seed + s)
            b = np.zeros((n, width), np.float32)
            b[:, :2] = rs.rand(n, 2) * 6.0 * np.sqrt(max(n, 1))   # a few overlapping neighbours per box at every size
            b[:, 2] = rs.randn(n)
            b[:, 3:6] = rs.rand(n, 3) * 6.0 + 1.5
            b[:, 6:width - 1] = 77.0   # columns between the size and the heading (the velocity of a 9-float box) take no part
            b[:, -1] = rs.rand(n) * 6.28 - 3.14
            per_seg.append(b)
            margins.append((R._pair_margin(b[:, [0, 1, 2, 3, 4, 5, -1]], False, IOU_THRESHOLD), R._pair_margin(b, True, RADII[s])))
        _cache[width, seed] = per_seg, margins
    per_seg, margins = _cache[width, seed]
    assert min(min(m) for m in margins) >= 1e-4, margins
    counts = list(SIZES)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    seg = torch.from_numpy(np.stack([offsets, np.asarray(counts, np.int32)])).cuda() if torch.cuda.is_available() else None
    return np.concatenate(per_seg), per_seg, seg, counts


@pytest.mark.parametrize("post", [None, 50])
def test_batched_nms_entries_match_the_oracle(post):
    from sparse2dense_amd import nms
    packed, per_seg, seg, counts = _packed_segments()
    boxes = torch.from_numpy(packed).cuda()
    keep, n_keep = nms.rotate_nms_batched(boxes, seg, counts, IOU_THRESHOLD, post)
    assert keep.shape == (len(SIZES), 4097 if post is None else post) and keep.dtype == torch.int64
    for s, b in enumerate(per_seg):
        desc = -np.arange(len(b), dtype=np.float32)   # already in score order
        want = O.rotate_nms(b[:, [0, 1, 2, 3, 4, 5, -1]], desc, IOU_THRESHOLD, None, post).tolist()
        assert keep[s, :n_keep[s]].tolist() == want, s
        assert post is not None or len(b) < 60 or len(want) < len(b), s   # the larger segments do lose boxes
    keep, n_keep = nms.circle_nms_batched(boxes, seg, counts, RADII, post)
    for s, b in enumerate(per_seg):
        desc = -np.arange(len(b), dtype=np.float32)
        want = O.circle_nms(b[:, :2], desc, RADII[s], post).tolist()
        assert keep[s, :n_keep[s]].tolist() == want, s
    assert n_keep[0] == n_keep[6] == 0 and n_keep[1] == 1 and 1 < n_keep[7] <= (post or 4097)


def test_a_workspace_above_the_bound_takes_the_old_chain(monkeypatch):
    from sparse2dense_amd import center_predict
    classes = CLASSES[3]
    cfg = _cfg(3, True, True)
    maps = _maps(classes, GRID_SEEDS[3, True], True, True)
    head = _head(classes, True)
    on = head.predict({}, _cuda(maps), cfg)
    monkeypatch.setattr(center_predict, "NMS_MAX_WORKSPACE_BYTES", 1024)
    off = head.predict({}, _cuda(maps), cfg)
    assert head.predict_paths == {"device": 1, "torch": 1}
    _same(on, off, "workspace bound")
    with pytest.raises(IndexError):   # a head without tasks never enters the device path: the chain's own error, as before
        head.predict({}, [], cfg)
    assert head.predict_paths == {"device": 1, "torch": 2}


def test_entries_stay_inside_their_buffers_and_repeat_bit_for_bit():
    """the C entries on test-owned outputs with sentinel guard bands on both sides of the packed boxes / scores / labels, `keep` and `n_keep`"""
    from sparse2dense_amd import _lib, center_predict as CP
    lib = _lib.load()
    classes, flip = [2, 1, 2], True
    cfg = _cfg(3, flip, False)
    maps = _cuda(_maps(classes, 2, flip, True))
    dev = maps[0]["hm"].device
    st = torch.cuda.current_stream().cuda_stream
    table, alive = CP._task_table(maps, [0, 2, 3])
    segs, hw, G = 6, H * W, 64
    geo = (4.0, 0.2, 0.2, -51.2, -51.2)
    rng = (_lib.ctypes.c_float * 6)(*cfg["post_center_limit_range"])

    def guarded(n, dtype, fill):
        buf = torch.full((n + 2 * G,), fill, dtype=dtype, device=dev)
        return buf, buf[G:G + n]

    def run():
        score_b, score = guarded(segs * hw, torch.float32, -5.0)
        label_b, label = guarded(segs * hw, torch.int32, -5)
        count_b, count = guarded(segs, torch.int32, -5)
        _lib.check(lib.s2d_center_predict_score(table, 3, 2, H, W, 1, 0.1, rng, *geo, score.data_ptr(), label.data_ptr(), count.data_ptr(), st))
        sorted_, order = torch.sort(score.view(segs, hw), dim=1, descending=True, stable=True)
        counts = count.tolist()
        offsets = [sum(counts[:s]) for s in range(segs)]
        total, nd, max_keep = sum(counts), 9, 40
        seg = torch.tensor([offsets, counts], dtype=torch.int32).to(dev)
        boxes_b, boxes = guarded(total * nd, torch.float32, -5.0)
        scores_b, scores = guarded(total, torch.float32, -5.0)
        labels_b, labels = guarded(total, torch.int64, -5)
        _lib.check(lib.s2d_center_predict_boxes(table, 3, 2, H, W, 1, *geo, order.data_ptr(), sorted_.data_ptr(), label.data_ptr(), seg[0].data_ptr(),
                                                seg[1].data_ptr(), max(counts), total, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), st))
        outs = {}
        for form in ("rotated", "circle"):
            keep_b, keep = guarded(segs * max_keep, torch.int64, -5)
            nk_b, nk = guarded(segs, torch.int32, -5)
            ws = torch.empty(lib.s2d_nms_batched_workspace_bytes(total, max(counts)), dtype=torch.uint8, device=dev)
            if form == "rotated":
                rc = lib.s2d_nms_rotated_bev_batched(boxes.data_ptr(), nd, seg[0].data_ptr(), seg[1].data_ptr(), segs, max(counts), total, 0.2, max_keep,
                                                     keep.data_ptr(), nk.data_ptr(), ws.data_ptr(), ws.numel(), st)
            else:
                radius = torch.tensor([4.0, 4.0, 12.0, 12.0, 10.0, 10.0], device=dev)
                rc = lib.s2d_nms_circle_batched(boxes.data_ptr(), nd, seg[0].data_ptr(), seg[1].data_ptr(), segs, max(counts), total, radius.data_ptr(),
                                                max_keep, keep.data_ptr(), nk.data_ptr(), ws.data_ptr(), ws.numel(), st)
            _lib.check(rc, form)
            outs[form] = (keep_b, nk_b)
        torch.cuda.synchronize()
        n = dict(score=segs * hw, label=segs * hw, count=segs, boxes=total * nd, scores=total, labels=total, keep=segs * max_keep, nk=segs)
        bufs = dict(score=score_b, label=label_b, count=count_b, boxes=boxes_b, scores=scores_b, labels=labels_b)
        for form, (keep_b, nk_b) in outs.items():
            bufs[f"keep_{form}"], bufs[f"nk_{form}"] = keep_b, nk_b
        for k, b in bufs.items():
            size = n[k.split("_")[0]]
            assert bool((b[:G] == -5).all()) and bool((b[G + size:] == -5).all()), f"guard band of {k} overwritten"
            if k.startswith("keep_"):
                rows, kept = b[G:G + size].view(segs, max_keep), bufs["nk_" + k[5:]][G:G + segs].tolist()
                assert all(0 < c <= max_keep for c in kept), kept
                for s, c in enumerate(kept):
                    assert bool((rows[s, c:] == -5).all()) and bool((rows[s, :c] >= 0).all()) and bool((rows[s, :c] < counts[s]).all()), (k, s)
        assert min(counts) > 30 and bool((boxes != -5.0).all()) and bool((labels >= 0).all())
        return bufs

    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), f"{k} differs between two calls"
    del alive


def test_the_switch_selects_the_path(monkeypatch):
    classes = CLASSES[3]
    cfg = _cfg(3, False, True)
    maps = _maps(classes, GRID_SEEDS[3, False], False, True)
    head = _head(classes, True)
    monkeypatch.delenv("S2D_CENTER_DEVICE_PREDICT", raising=False)
    on = head.predict({}, _cuda(maps), cfg)
    assert head.predict_paths == {"device": 1, "torch": 0}
    monkeypatch.setenv("S2D_CENTER_DEVICE_PREDICT", "0")
    off = head.predict({}, _cuda(maps), cfg)
    assert head.predict_paths == {"device": 1, "torch": 1}
    monkeypatch.setenv("S2D_CENTER_DEVICE_PREDICT", "1")
    head.predict({}, _cuda(maps), cfg)
    assert head.predict_paths == {"device": 2, "torch": 1}
    _same(on, off, "switch")
    with pytest.raises(NotImplementedError):
        head.predict({}, _cuda(maps), dict(cfg, per_class_nms=True))


def test_detector_callers_agree_with_the_device_path_on_and_off(monkeypatch):
    """VoxelNet.forward(return_loss=False) and forward_two_stage(return_loss=False) - the proposal source of two-stage training -
    through both paths on the same frames"""
    from sparse2dense_amd import registry, waymo_configs
    from sparse2dense_amd.data import SyntheticFrames
    torch.manual_seed(0)
    det = registry.build_detector(waymo_configs.centerpoint_voxelnet()).to("cuda").eval()
    det.test_cfg = dict(post_center_limit_range=[-80, -80, -10.0, 80, 80, 10.0], score_threshold=0.1, pc_range=[-75.2, -75.2], out_size_factor=8,
                        voxel_size=[0.1, 0.1], nms=dict(nms_pre_max_size=4096, nms_post_max_size=500, nms_iou_threshold=0.7))
    ex = SyntheticFrames(2, n_points=12000, seed=5, device="cuda").example()
    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("S2D_CENTER_DEVICE_PREDICT", flag)
        with torch.no_grad():
            outs[flag] = (det(ex, return_loss=False), det.forward_two_stage(ex, return_loss=False)[0])
    assert det.bbox_head.predict_paths == {"device": 2, "torch": 2}
    assert sum(len(o["scores"]) for o in outs["1"][0]) > 0
    for k, what in enumerate(("forward", "forward_two_stage")):
        _same(outs["1"][k], outs["0"][k], what)
