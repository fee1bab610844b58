"""The static anchor predict path: s2d_anchor_predict_finish_static against s2d_anchor_predict_finish + anchor_predict.assembly_rows, and
anchor_predict.StaticAnchorPlan / MultiGroupHead.predict_static against MultiGroupHead.predict (the device path, bit for bit: both run the
same decode, NMS and finish code on the same candidate order), the reference's recorded outputs, the absence of host round trips and the
replay of one captured HIP graph."""
import copy
import os

import numpy as np
import pytest
import torch

import anchor_predict_ref as R
import anchor_util as AU
from sparse2dense_amd import _lib, anchor_predict as AP, waymo_configs as WC
from sparse2dense_amd.registry import build_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 64   # guard band, in elements, on both sides of every output of the finish entry
OFFSET = 0.25   # direction_offset of the kernel cases: headings are drawn on both sides of it


@pytest.fixture(autouse=True)
def _switch_unset(monkeypatch):
    monkeypatch.delenv("S2D_ANCHOR_DEVICE_PREDICT", raising=False)


# ---- s2d_anchor_predict_finish_static against s2d_anchor_predict_finish + assembly_rows ------------------------------------------------------
# what a segment is made of; segment s of a case takes KINDS[(s + shift) % len(KINDS)], so that the cases of one segment meet all of them
KINDS = ("plain", "n_keep_0", "n_keep_1", "n_keep_full", "n_keep_above", "n_keep_negative", "all_out_of_range", "counts_0", "keep_out_of_range",
         "outside_the_lists")


def _packed_case(tasks, samples, max_keep, shift):
    """hand-built packed candidate lists, keep lists and the segment table (CPU tensors) for tasks * samples segments"""
    gen = torch.Generator().manual_seed(100 * tasks + 10 * samples + max_keep + shift)
    segs = tasks * samples
    kinds = [KINDS[(s + shift) % len(KINDS)] for s in range(segs)]
    counts = [0 if kind == "counts_0" else int(torch.randint(max_keep // 2 + 1, max_keep + 40, (1,), generator=gen)) for kind in kinds]
    offsets, total = [], 3   # three rows no segment owns in front, the segments in reverse order: offsets are not ascending
    for s in reversed(range(segs)):
        offsets.insert(0, total)
        total += counts[s] + 2
    boxes = torch.randn((total, 7), generator=gen)
    boxes[:, 6] = -(OFFSET + (torch.rand(total, generator=gen) - 0.5))   # the NMS form: the heading negated; r - OFFSET in (-0.5, 0.5)
    boxes[::5, 6] = -OFFSET   # r - direction_offset == 0 exactly: `> 0` is false
    scores = torch.rand(total, generator=gen)
    labels = torch.randint(0, 3, (total,), generator=gen, dtype=torch.int32)
    dirs = torch.randint(0, 2, (total,), generator=gen, dtype=torch.int32)
    in_range = (torch.rand(total, generator=gen) < 0.7).to(torch.uint8)
    keep = torch.zeros((segs, max_keep), dtype=torch.int64)
    n_keep = torch.zeros((segs,), dtype=torch.int32)
    for s, kind in enumerate(kinds):
        c = counts[s]
        keep[s] = torch.randint(0, max(c, 1), (max_keep,), generator=gen)
        n_keep[s] = dict(n_keep_0=0, n_keep_1=1, n_keep_full=max_keep, n_keep_above=max_keep + 7, n_keep_negative=-2).get(kind, min(max_keep, max(c // 2, 1)))
        if kind == "all_out_of_range":
            in_range[offsets[s]:offsets[s] + c] = 0
        if kind in ("n_keep_1", "n_keep_full", "n_keep_above"):   # at least the first kept row survives
            in_range[offsets[s] + keep[s, 0]] = 1
        if kind == "keep_out_of_range":   # an index at the count, far above it and below zero; the row behind the segment is in range
            n_keep[s] = max_keep
            keep[s, 0], keep[s, 2], keep[s, max_keep - 1] = c, 1 << 40, -1
            in_range[offsets[s] + c] = 1
            in_range[offsets[s] + keep[s, 1]] = 1
        if kind == "outside_the_lists":
            offsets[s] = total - c + 1
    table = torch.tensor([offsets, counts], dtype=torch.int32)
    return dict(boxes=boxes, scores=scores, labels=labels, dirs=dirs, in_range=in_range, keep=keep, n_keep=n_keep, table=table, total=total,
                kinds=kinds)


def _guarded(n, dtype, fill):
    """(view of n elements, whole buffer): the view lies between two guard bands of G elements, everything filled with `fill`"""
    whole = torch.full((n + 2 * G,), fill, dtype=dtype, device=DEV)
    return whole[G:G + n], whole


@pytest.mark.parametrize("use_direction", [0, 1], ids=["no_dir", "dir"])
@pytest.mark.parametrize("max_keep", [5, 300])
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("tasks", [1, 3, 8])
def test_finish_static_equals_finish_and_assembly(tasks, samples, max_keep, use_direction):
    lib = _lib.load()
    segs, cap = tasks * samples, tasks * max_keep
    seen, headings = set(), []
    for shift in range(len(KINDS) if segs < len(KINDS) else 1):   # few segments: one launch per rotation, so every kind is met
        case = _packed_case(tasks, samples, max_keep, shift)
        seen |= set(case["kinds"])
        d = {k: v.to(DEV) for k, v in case.items() if torch.is_tensor(v)}
        task_table = (_lib.AnchorPredictTask * tasks)()
        for t, rec in enumerate(task_table):
            rec.label_base = 10 * t + 1
        ptr = lambda t: t.data_ptr()
        common = (task_table, tasks, samples, ptr(d["boxes"]), ptr(d["scores"]), ptr(d["labels"]), ptr(d["dirs"]), ptr(d["in_range"]), ptr(d["table"][0]),
                  ptr(d["table"][1]), case["total"], ptr(d["keep"]), ptr(d["n_keep"]), max_keep, use_direction, OFFSET)
        st = torch.cuda.current_stream().cuda_stream
        # the reference: the per-segment finish, its counts read on the host, the rows gathered in output order
        seg_boxes = torch.full((segs * max_keep, 7), float("nan"), device=DEV)
        seg_scores = torch.full((segs * max_keep,), float("nan"), device=DEV)
        seg_labels = torch.full((segs * max_keep,), -9, dtype=torch.int64, device=DEV)
        seg_count = torch.full((segs,), -9, dtype=torch.int32, device=DEV)
        _lib.check(lib.s2d_anchor_predict_finish(*common, ptr(seg_boxes), ptr(seg_scores), ptr(seg_labels), ptr(seg_count), st), "s2d_anchor_predict_finish")
        final = seg_count.tolist()
        rows, sizes = AP.assembly_rows(final, tasks, samples, max_keep)
        rows = torch.tensor(rows, dtype=torch.int64, device=DEV)
        # the entry under test, every output between sentinel-filled guard bands
        boxes, boxes_b = _guarded(samples * cap * 7, torch.float32, 7.0)
        scores, scores_b = _guarded(samples * cap, torch.float32, 7.0)
        labels, labels_b = _guarded(samples * cap, torch.int64, 7)
        counts, counts_b = _guarded(samples, torch.int32, 7)
        _lib.check(lib.s2d_anchor_predict_finish_static(*common, ptr(boxes), ptr(scores), ptr(labels), ptr(counts), st), "s2d_anchor_predict_finish_static")
        torch.cuda.synchronize()
        boxes, scores, labels = boxes.view(samples, cap, 7), scores.view(samples, cap), labels.view(samples, cap)
        assert counts.tolist() == sizes, (shift, counts.tolist(), sizes)
        want = list(zip(seg_boxes[rows].split(sizes), seg_scores[rows].split(sizes), seg_labels[rows].split(sizes)))
        for b, (n, (wb, ws, wl)) in enumerate(zip(sizes, want)):
            assert torch.equal(boxes[b, :n].view(torch.int32), wb.view(torch.int32)), (shift, b)   # bit for bit, NaN-proof
            assert torch.equal(scores[b, :n], ws) and torch.equal(labels[b, :n], wl), (shift, b)
            # the padding: exactly zero (the bits: no -0.0) with label -1
            assert not boxes[b, n:].contiguous().view(torch.int32).any() and not scores[b, n:].contiguous().view(torch.int32).any(), (shift, b)
            assert bool((labels[b, n:] == -1).all()), (shift, b)
        for whole in (boxes_b, scores_b, labels_b, counts_b):
            assert bool((whole[:G] == 7).all()) and bool((whole[-G:] == 7).all()), shift
        # what the case was built for
        for s, kind in enumerate(case["kinds"]):
            if kind in ("n_keep_0", "n_keep_negative", "all_out_of_range", "counts_0", "outside_the_lists"):
                assert final[s] == 0, (kind, final[s])
            if kind == "n_keep_1":
                assert final[s] == 1
            if kind in ("n_keep_full", "n_keep_above", "keep_out_of_range"):
                assert 0 < final[s] <= max_keep - (3 if kind == "keep_out_of_range" else 0), (kind, final[s])
            if kind == "n_keep_full" and max_keep == 300:   # rows behind the first 256-row chunk survive
                assert bool(case["in_range"][case["table"][0, s] + case["keep"][s, 256:]].any())
        headings += [boxes[b, :n, 6].clone() for b, n in enumerate(sizes)]
    assert seen == set(KINDS)
    headings = torch.cat(headings)
    flipped = headings > OFFSET + 1.0   # r lies in OFFSET +- 0.5; a flipped row has pi added
    assert bool(flipped.any()) and not bool(flipped.all()) if use_direction else not bool(flipped.any())


def test_finish_static_is_a_no_op_without_samples():
    lib = _lib.load()
    task_table = (_lib.AnchorPredictTask * 1)()
    out, whole = _guarded(8, torch.int32, 7)
    p = out.data_ptr()
    assert lib.s2d_anchor_predict_finish_static(task_table, 1, 0, p, p, p, p, p, p, p, 0, p, p, 4, 1, 0.0, p, p, p, p, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((whole == 7).all())


# ---- the static path against MultiGroupHead.predict -----------------------------------------------------------------------------------------
def _head():
    return build_head(WC.second_voxelnet_train()["bbox_head"]).to(DEV).eval()


def _cuda(preds):
    return [{k: v.to(DEV) for k, v in p.items()} for p in preds]


def _example(tables, batch):
    return dict(anchors=[torch.from_numpy(t).to(DEV).unsqueeze(0).expand(batch, -1, -1) for t in tables], metadata=[f"m{i}" for i in range(batch)])


def _assert_equals_predict(det, want, what=""):
    """the first counts[b] rows of every sample equal `predict`'s lists bit for bit; the rows behind them are zero / -1"""
    counts = det.counts.tolist()
    assert len(counts) == len(want) and det.boxes.shape[:2] == det.scores.shape == det.labels.shape and det.boxes.shape[2] == 7, what
    assert det.labels.dtype == torch.int64 and det.counts.dtype == torch.int32 and det.boxes.dtype == det.scores.dtype == torch.float32
    for b, (n, w) in enumerate(zip(counts, want)):
        assert n == len(w["scores"]), (what, b, n, len(w["scores"]))
        assert torch.equal(det.boxes[b, :n], w["box3d_lidar"]) and torch.equal(det.scores[b, :n], w["scores"]), (what, b)
        assert torch.equal(det.labels[b, :n], w["label_preds"]), (what, b)
        assert not det.boxes[b, n:].any() and not det.scores[b, n:].any() and bool((det.labels[b, n:] == -1).all()), (what, b)


def _assert_lists_identical(got, want, what=""):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert set(a) == {"box3d_lidar", "scores", "label_preds", "metadata"} and a["metadata"] == b["metadata"], (what, i)
        for k in ("scores", "label_preds", "box3d_lidar"):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, i, k)


def _static_and_predict(head, example, preds, cfg, what):
    """(StaticDetections, predict's lists) on the same inputs, with everything the two must agree on asserted"""
    calls, paths = head.static_predict_calls, dict(head.predict_paths)
    det, meta = head.predict_static(example, preds, cfg)
    assert head.static_predict_calls == calls + 1 and head.predict_paths == paths   # predict_static leaves predict's counters alone
    want = head.predict(example, preds, cfg)
    assert head.predict_paths == dict(paths, device=paths["device"] + 1)
    assert meta == example["metadata"]
    _assert_equals_predict(det, want, what)
    _assert_lists_identical(det.as_list(meta), want, what)
    # overflow is the pre_max cut `predict` takes itself: the pass counts against k
    nms = cfg["nms"]
    k = nms["nms_pre_max_size"]
    anchors = [head._task_anchors(example, t) for t in range(len(preds))]
    passed = AP.decode_anchor_candidates(preds, anchors, cfg).passed
    assert det.overflow.dtype == torch.int32 and det.overflow.tolist() == [int(p > k) for p in passed], (what, passed)
    cap = len(preds) * min(k, nms["nms_post_max_size"])
    assert det.boxes.shape == (len(want), cap, 7), what
    return det, want, passed


def _close(got, ref, what=""):
    """the tolerances of test_anchor_predict_gpu.py for anchor_predict.npz; kept scores and labels in order"""
    assert len(got) == len(ref), what
    for i, (a, r) in enumerate(zip(got, ref)):
        assert a["scores"].shape == r["scores"].shape, (what, i, a["scores"].shape, r["scores"].shape)
        np.testing.assert_allclose(a["scores"].cpu().numpy(), r["scores"], rtol=1e-5, err_msg=f"{what} {i}")
        assert np.array_equal(a["label_preds"].cpu().numpy(), r["label_preds"]) and a["label_preds"].dtype == torch.int64, (what, i)
        np.testing.assert_allclose(a["box3d_lidar"].cpu().numpy(), r["box3d_lidar"], rtol=1e-4, atol=2e-4, err_msg=f"{what} {i}")


def test_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "anchor_predict.npz"))
    head = _head()
    box, cls, dirs = [t.to(DEV) for t in AU.predict_inputs(2)]
    preds = [dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)]
    example = _example([R.second_table(AU.H, AU.W)], 2)
    det, want, passed = _static_and_predict(head, example, preds, WC.SECOND_TEST_CFG, "golden")
    assert passed == [len(g["cand_index_0"]), len(g["cand_index_1"])] and not det.overflow.any()
    _close(det.as_list(), [dict(scores=g[f"scores_{i}"], label_preds=g[f"label_preds_{i}"], box3d_lidar=g[f"box3d_lidar_{i}"]) for i in range(2)], "golden")


_SMALL = {}


def _small():
    """the small case and the restatement's result, computed once"""
    if not _SMALL:
        box, cls, dirs, table, cfg = R.small_case()
        ref, segments = R.check_small_case(box, cls, dirs, table, cfg)   # asserts the properties of the inputs on the host (see its docstring)
        _SMALL.update(box=box, cls=cls, dirs=dirs, table=table, cfg=cfg, ref=ref, passed=[len(c[0]) for c, _ in segments[0]])
    return _SMALL


def _small_preds(cls=None):
    s = _small()
    return _cuda([dict(box_preds=s["box"], cls_preds=s["cls"] if cls is None else cls, dir_cls_preds=s["dirs"])])


def test_small_shapes_every_cut_and_the_range_after_the_nms():
    s = _small()
    cfg = s["cfg"]
    head = _head()
    det, want, passed = _static_and_predict(head, _example([s["table"]], R.SMALL_B), _small_preds(), cfg, "small")
    _close(det.as_list(), s["ref"], "small")
    assert passed == s["passed"] and passed[0] == 24 and det.overflow.tolist() == [1, 0, 0]   # the pre_max cut (24 > 16), an empty sample
    assert det.counts.tolist()[2] == 0 and det.counts.tolist()[1] < cfg["nms"]["nms_post_max_size"]   # the range drop after the post_max cut
    assert det.boxes.shape == (3, 5, 7)
    # no range: nothing is dropped after the NMS, the post_max cut fills the sample's rows
    open_cfg = dict(cfg, post_center_limit_range=None)
    det, want, _ = _static_and_predict(head, _example([s["table"]], R.SMALL_B), _small_preds(), open_cfg, "small, no range")
    assert det.counts.tolist()[1] == cfg["nms"]["nms_post_max_size"] and len(head._static_plans) == 2 and head.static_predict_calls == 2


def test_two_tasks_with_different_anchor_and_class_counts():
    preds, tables = R.two_task_case()
    head = R.two_task_head().to(DEV).eval()
    assert head.num_classes == [1, 2] and [t.shape[0] for t in tables] == [128, 256]
    cfg = copy.deepcopy(WC.SECOND_TEST_CFG)
    det, want, passed = _static_and_predict(head, _example(tables, 2), _cuda(preds), cfg, "two tasks")
    ref, _ = R.predict(preds, tables, cfg, [1, 2])
    _close(det.as_list(), ref, "two tasks")
    plan = next(iter(head._static_plans.values()))
    assert plan.max_anchors == 256 and plan.score.shape == (4, 256) and bool((plan.score[:2, 128:] == -1).all())   # the padded score columns
    assert min(passed) > 0 and min(det.counts.tolist()) > 0
    # a pre_max cut below the pass counts: padded columns never enter, the two paths still agree
    cut = copy.deepcopy(cfg)
    cut["nms"].update(nms_pre_max_size=7, nms_post_max_size=4)
    det, _, passed = _static_and_predict(head, _example(tables, 2), _cuda(preds), cut, "two tasks, cut")
    assert det.overflow.any() and det.boxes.shape == (2, 8, 7)


def test_no_anchor_passes_anywhere():
    s = _small()
    head = _head()
    preds = _small_preds(torch.full_like(s["cls"], -6.0))
    det, want, passed = _static_and_predict(head, _example([s["table"]], R.SMALL_B), preds, s["cfg"], "empty")
    assert passed == [0, 0, 0] and det.counts.tolist() == [0, 0, 0] and not det.overflow.any()
    assert [d["box3d_lidar"].shape for d in det.as_list()] == [(0, 7)] * 3


def test_a_plan_without_the_direction_classifier():
    s = _small()
    table = torch.from_numpy(s["table"]).to(DEV)
    preds = _small_preds()
    plan = AP.StaticAnchorPlan(s["cfg"], [3], [table], R.SMALL_B, False, 0.0, DEV)
    det = plan.run(preds)
    want = AP.predict_on_device(preds, [table], s["cfg"], [3], use_direction=False)
    _assert_equals_predict(det, [dict(box3d_lidar=b, scores=sc, label_preds=l) for b, sc, l in want], "no direction classifier")
    bare = [{k: v for k, v in preds[0].items() if k != "dir_cls_preds"}]   # dir_cls_preds is not even needed
    assert plan.run(bare) is det
    _assert_equals_predict(det, [dict(box3d_lidar=b, scores=sc, label_preds=l) for b, sc, l in want], "no dir_cls_preds")
    with_dir = AP.predict_on_device(preds, [table], s["cfg"], [3], use_direction=True)
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(want, with_dir))   # the flag matters on these inputs


# ---- stale state, no host round trip, graph capture -------------------------------------------------------------------------------------------
def _small_plan():
    s = _small()
    table = torch.from_numpy(s["table"]).to(DEV)
    return AP.StaticAnchorPlan(s["cfg"], [3], [table], R.SMALL_B, True, 0.0, DEV), table


def _snapshot(det):
    return [t.clone() for t in det]


def test_stale_state_does_not_reach_the_outputs():
    plan, _ = _small_plan()
    preds = _small_preds()
    first = _snapshot(plan.run(preds))
    second = _snapshot(plan.run(preds))
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, second))   # two runs are bit-equal
    # traps in everything a run leaves behind: NaN boxes, score 1.0, valid labels, large indices
    b = plan.buffers()
    b["cand_boxes"].fill_(float("nan"))
    b["cand_scores"].fill_(1.0)
    b["cand_labels"].fill_(2)
    b["cand_dirs"].fill_(1)
    b["cand_in_range"].fill_(1)
    b["keep"].fill_(1 << 40)
    b["n_keep"].fill_(plan.max_keep)
    b["order"].fill_(1 << 40)
    b["score_sorted"].fill_(1.0)
    b["table"].fill_(1 << 20)
    b["passed"].fill_(1 << 20)
    for name in ("boxes", "scores"):
        b[name].fill_(float("nan"))
    b["labels"].fill_(2)
    b["counts"].fill_(plan.cap)
    third = _snapshot(plan.run(preds))
    assert all(torch.equal(a.view(torch.uint8), c.view(torch.uint8)) for a, c in zip(first, third))
    # ... and in front of a run on which nothing passes: nothing of the earlier frame survives
    s = _small()
    empty = plan.run(_small_preds(torch.full_like(s["cls"], -6.0)))
    assert empty.counts.tolist() == [0, 0, 0] and not empty.boxes.any() and not empty.scores.any() and bool((empty.labels == -1).all())


def test_run_neither_synchronises_nor_allocates():
    s = _small()
    head = _head()
    plan, table = _small_plan()
    preds = _small_preds()
    out = plan.run(preds)   # warm-up: code objects loaded
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in plan.buffers().items()}
    assert set(ptrs) >= {"score", "label", "passed", "order", "score_sorted", "table", "cand_boxes", "cand_scores", "cand_labels", "cand_dirs", "cand_in_range",
                         "keep", "n_keep", "nms_ws", "boxes", "scores", "labels", "counts", "anchors_0"}
    assert ptrs["anchors_0"] == table.data_ptr()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = plan.run(preds)
        again = plan.run(preds)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert again is out and {k: v.data_ptr() for k, v in plan.buffers().items()} == ptrs
    _assert_equals_predict(out, head.predict(dict(anchors=[table]), preds, s["cfg"]))


def test_one_captured_graph_replays_on_new_predictions():
    s = _small()
    cfg = s["cfg"]
    head = _head()
    plan, table = _small_plan()
    example = dict(anchors=[table])

    def fresh(i):
        box, cls, dirs, _, _ = R.small_case(seed=4400 + i)
        if i == 2:
            cls = torch.full_like(cls, -6.0)   # nothing passes anywhere
        return _cuda([dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)])
    static = [{k: v.clone() for k, v in p.items()} for p in fresh(0)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            plan.run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan.run(static)
    cuts = 0
    for i in range(6):
        preds = fresh(i)
        for dst, src in zip(static, preds):
            for k in dst:
                dst[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        want = head.predict(example, preds, cfg)
        _assert_equals_predict(out, want, f"replay {i}")
        cuts += int(out.overflow.sum())
        if i == 2:
            assert out.counts.tolist() == [0, 0, 0] and not out.overflow.any()
        else:
            assert out.overflow.tolist()[0] == 1 and out.counts.tolist()[0] > 0   # frame 0 of the small case passes 24 > 16 anchors
    assert cuts >= 5 and head.predict_paths == {"device": 6, "torch": 0}
