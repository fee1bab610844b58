"""The static predict path: s2d_segment_topk against torch.sort, s2d_predict_static_gather and center_predict.StaticPredictPlan /
CenterHead.predict_static against CenterHead.predict (the device path, bit for bit), the reference's recorded outputs, the absence of
host round trips and the replay of one captured HIP graph."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import predict_tasks_util as U   # noqa: E402

pytestmark = pytest.mark.gpu

G = 64   # guard band, in elements, on both sides of every output of the top-K entry
ORDER_FILL, SCORE_FILL = -7, -7.0


# ---- s2d_segment_topk against torch.sort -----------------------------------------------------------------------------------------------------
def _sparse(segs, n, gen):
    """what the score kernel writes: sigmoid values, about 99 % of the cells dropped"""
    s = torch.sigmoid(torch.randn(segs, n, generator=gen))
    s[torch.rand(segs, n, generator=gen) < 0.99] = float("-inf")
    return s


def _sentinel_mix(segs, n, gen):
    s = torch.rand(segs, n, generator=gen)
    s[torch.rand(segs, n, generator=gen) < 0.7] = -1.0
    return s


def _zero_mix(segs, n, gen):
    s = torch.zeros(segs, n)
    s[torch.rand(segs, n, generator=gen) < 0.5] = -0.0
    return s


CONTENTS = {
    "sparse": _sparse,
    "all_neg_inf": lambda segs, n, gen: torch.full((segs, n), float("-inf")),
    "all_half": lambda segs, n, gen: torch.full((segs, n), 0.5),
    "eight_levels": lambda segs, n, gen: torch.randint(0, 8, (segs, n), generator=gen).float() / 8,
    "ascending": lambda segs, n, gen: torch.arange(n, dtype=torch.float32).repeat(segs, 1) - 100.0,
    "descending": lambda segs, n, gen: 100.0 - torch.arange(n, dtype=torch.float32).repeat(segs, 1),
    "sentinel_mix": _sentinel_mix,
    "zero_mix": _zero_mix,
}
# (segments, row_len, k, row_stride): k > row_len; rows in several groups of four; 4097 > 4096 = the largest k; a row longer than any
# single LDS pass; the six-task nuScenes score map; a stride that puts every row at another distance from a 16-byte boundary
SHAPES = [(1, 1, 1, 1), (3, 63, 64, 63), (2, 193, 64, 193), (5, 4097, 4096, 4097), (2, 70001, 1000, 70001), (24, 32400, 1000, 32400),
          (4, 1001, 100, 1003)]


def _topk(score, row_len, k, passed=None, out_stride=None):
    """the entry on outputs carved out of sentinel-filled buffers; returns (order, score_sorted, table, whole buffers)"""
    from sparse2dense_amd import _lib
    lib = _lib.load()
    segs, row_stride = score.shape
    out_stride = out_stride or k + 3
    dev = score.device
    order_b = torch.full((segs * out_stride + 2 * G,), ORDER_FILL, dtype=torch.int64, device=dev)
    sorted_b = torch.full((segs * out_stride + 2 * G,), SCORE_FILL, dtype=torch.float32, device=dev)
    table_b = torch.full((3 * segs + 2 * G,), ORDER_FILL, dtype=torch.int32, device=dev)
    order, sorted_ = order_b[G:G + segs * out_stride].view(segs, out_stride), sorted_b[G:G + segs * out_stride].view(segs, out_stride)
    table = table_b[G:G + 3 * segs].view(3, segs)
    tp = (lambda i: table[i].data_ptr()) if passed is not None else (lambda i: None)
    _lib.check(lib.s2d_segment_topk(score.data_ptr(), segs, row_len, row_stride, k, passed.data_ptr() if passed is not None else None,
                                    order.data_ptr(), sorted_.data_ptr(), out_stride, tp(0), tp(1), tp(2),
                                    torch.cuda.current_stream().cuda_stream), "s2d_segment_topk")
    torch.cuda.synchronize()
    return order, sorted_, table, (order_b, sorted_b, table_b)


@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_topk_is_the_head_of_the_stable_descending_sort(shape, content):
    segs, n, k, stride = shape
    gen = torch.Generator().manual_seed(1000 * n + k)
    score = torch.full((segs, stride), 9.0)   # the columns between row_len and row_stride would win every rank if they were read
    score[:, :n] = CONTENTS[content](segs, n, gen)
    score = score.cuda()
    want_sorted, want_order = torch.sort(score[:, :n], dim=1, descending=True, stable=True)
    kk = min(k, n)
    passed = torch.tensor([(k - 1, k, k + 1, 0, 5 * k)[s % 5] for s in range(segs)], dtype=torch.int32).cuda()
    order, sorted_, table, bufs = _topk(score, n, k, passed)
    assert torch.equal(order[:, :kk], want_order[:, :kk])
    assert torch.equal(sorted_[:, :kk], want_sorted[:, :kk])
    assert torch.equal(sorted_[:, :kk].contiguous().view(torch.int32), want_sorted[:, :kk].contiguous().view(torch.int32))   # the sign of a zero too
    if content == "all_half" and n > k:
        assert order[:, :kk].tolist() == [list(range(k))] * segs
    # untouched: the ranks from min(k, row_len) on and the guard bands
    assert bool((order[:, kk:] == ORDER_FILL).all()) and bool((sorted_[:, kk:] == SCORE_FILL).all())
    for b, fill in zip(bufs, (ORDER_FILL, SCORE_FILL, ORDER_FILL)):
        assert bool((b[:G] == fill).all()) and bool((b[-G:] == fill).all())
    # the segment table
    p = passed.tolist()
    assert table[0].tolist() == [s * k for s in range(segs)]
    assert table[1].tolist() == [min(c, k) for c in p]
    assert table[2].tolist() == [int(c > k) for c in p]
    # bit for bit the same at a second call, with or without the table
    again = _topk(score, n, k, passed)
    plain = _topk(score, n, k, None)
    for i, a in enumerate(bufs):
        assert torch.equal(a.view(torch.uint8), again[3][i].view(torch.uint8)), i
        if i < 2:
            assert torch.equal(a.view(torch.uint8), plain[3][i].view(torch.uint8)), i
    assert bool((plain[3][2] == ORDER_FILL).all())


def test_topk_refuses_what_it_cannot_do():
    from sparse2dense_amd import _lib
    lib = _lib.load()
    score = torch.zeros(2, 100).cuda()
    out = torch.zeros(2, 100, dtype=torch.int64).cuda()
    args = lambda row_len=100, stride=100, k=10, out_stride=10: (score.data_ptr(), 2, row_len, stride, k, None, out.data_ptr(), score.data_ptr(), out_stride,
                                                                 None, None, None, None)
    for bad in (dict(k=0), dict(k=4097), dict(row_len=101), dict(out_stride=9), dict(row_len=(1 << 20) + 1, stride=1 << 21)):
        with pytest.raises(_lib.S2DError):
            _lib.check(lib.s2d_segment_topk(*args(**bad)), "s2d_segment_topk")


# ---- the static path against CenterHead.predict --------------------------------------------------------------------------------------------
H = W = 40
SIX = [1, 2, 2, 1, 2, 2]
WIDE = [-100.0, -100.0, -10.0, 100.0, 100.0, 10.0]
CUT = dict(nms_pre_max_size=64, nms_post_max_size=83, nms_iou_threshold=0.2)   # every segment below has more than 64 passing pixels


def _head(classes, vel=True):
    from sparse2dense_amd.heads import CenterHead
    heads = {k: v for k, v in U.COMMON_HEADS.items() if vel or k != "vel"}
    tasks = [dict(num_class=c, class_names=[f"c{i}_{j}" for j in range(c)]) for i, c in enumerate(classes)]
    return CenterHead(in_channels=64, tasks=tasks, dataset="nuscenes", weight=0.25, code_weights=[1.0] * (10 if vel else 8), common_heads=heads).eval()


def _cfg(tasks, flip, circular, **over):
    cfg = dict(U.CFG, double_flip=flip, circular_nms=circular, min_radius=U.CFG["min_radius"][:tasks], nms=dict(CUT), post_center_limit_range=WIDE)
    cfg.update(over)
    return cfg


def _maps(classes, seed, flip, vel=True, h=H, w=W, samples=2, peaks=150, task_peaks=None):
    out = []
    for i, c in enumerate(classes):
        n = peaks if task_peaks is None else task_peaks[i]
        p = U.seeded_task_maps(c, seed * 1000 + i, h, w, samples, flip, vel=vel, peaks=n, peak_logit=(-1.0, 2.0))
        out.append({k: v.cuda() for k, v in p.items()})
    return out


def _assert_equals_predict(det, want, what=""):
    """the first counts[b] rows of every sample equal `predict`'s lists bit for bit; the rows behind them are zero / -1"""
    counts = det.counts.tolist()
    assert len(counts) == len(want) and det.boxes.shape[:2] == det.scores.shape == det.labels.shape, what
    assert det.labels.dtype == torch.int64 and det.counts.dtype == torch.int32 and det.boxes.dtype == det.scores.dtype == torch.float32
    for b, (n, w) in enumerate(zip(counts, want)):
        assert n == len(w["scores"]), (what, b, n, len(w["scores"]))
        assert torch.equal(det.boxes[b, :n], w["box3d_lidar"]) and torch.equal(det.scores[b, :n], w["scores"]), (what, b)
        assert torch.equal(det.labels[b, :n], w["label_preds"]), (what, b)
        assert not det.boxes[b, n:].any() and not det.scores[b, n:].any() and bool((det.labels[b, n:] == -1).all()), (what, b)
    for got, w in zip(det.as_list(), want):
        assert torch.equal(got["box3d_lidar"], w["box3d_lidar"]) and torch.equal(got["label_preds"], w["label_preds"])


@pytest.mark.parametrize("circular", [False, True], ids=["rotated", "circular"])
@pytest.mark.parametrize("flip", [False, True], ids=["plain", "double_flip"])
@pytest.mark.parametrize("vel", [True, False], ids=["vel", "no_vel"])
@pytest.mark.parametrize("tasks", [1, 6])
def test_static_equals_predict(tasks, vel, flip, circular):
    classes = SIX[:tasks]
    cfg = _cfg(tasks, flip, circular)
    maps = _maps(classes, 11, flip, vel)
    head = _head(classes, vel)
    example = {"metadata": [f"m{i}" for i in range(maps[0]["hm"].shape[0])]}
    want = head.predict(example, maps, cfg)
    assert head.predict_paths == {"device": 1, "torch": 0} and head.static_predict_calls == 0
    det, meta = head.predict_static(example, maps, cfg)
    assert head.predict_paths == {"device": 1, "torch": 0} and head.static_predict_calls == 1
    assert det.boxes.shape == (2, tasks * (64 if not circular else 83), 9 if vel else 7)
    assert meta == [w["metadata"] for w in want] == (["m0", "m4"] if flip else ["m0", "m1"])
    from sparse2dense_amd import center_predict
    passed = center_predict.decode_center_maps(maps, cfg, flip).passed
    assert min(passed) > 64 and max(passed) < 4096, passed   # the rotated cut is taken; the circular form takes every passing pixel
    assert not det.overflow.any() if circular else bool(det.overflow.all())
    assert sum(len(w["scores"]) for w in want) > 0
    _assert_equals_predict(det, want)
    assert [d["metadata"] for d in det.as_list(meta)] == meta


def test_static_on_channels_last_empty_segments_and_an_empty_sample():
    classes = SIX[:3]
    head = _head(classes)
    cfg = _cfg(3, True, False, post_center_limit_range=U.CFG["post_center_limit_range"])
    maps = _maps(classes, 12, True, task_peaks=[150, 0, 150])   # task 1 has no passing pixel in either sample
    maps = [{k: v.contiguous(memory_format=torch.channels_last) for k, v in p.items()} for p in maps]
    assert not maps[0]["dim"].is_contiguous()
    det, _ = head.predict_static({}, maps, cfg)
    want = head.predict({}, maps, cfg)
    _assert_equals_predict(det, want, "channels_last, empty task")
    assert min(det.counts.tolist()) > 0
    for p in maps:   # sample 1 (images 4..7) loses every peak: all of its segments are empty
        p["hm"][4:] = -9.0
    det, _ = head.predict_static({}, maps, cfg)
    assert head.static_predict_calls == 2 and len(head._static_plans) == 1
    _assert_equals_predict(det, head.predict({}, maps, cfg), "empty sample")
    assert det.counts.tolist()[1] == 0 and det.counts.tolist()[0] > 0


def test_circular_overflow_is_flagged_and_is_the_nms_of_the_k_best():
    from sparse2dense_amd import center_predict, nms
    classes, k = SIX[:2], 32
    head = _head(classes)
    cfg = _cfg(2, False, True)
    maps = _maps(classes, 13, False, task_peaks=[150, 20])
    det, _ = head.predict_static({}, maps, cfg, max_candidates=k)
    assert det.overflow.tolist() == [1, 1, 0, 0]   # segments task * samples + sample: task 0 passes more than 32 pixels, task 1 fewer
    cand = center_predict.decode_center_maps(maps, cfg, False, pre_max_size=k, label_bases=[0, 1])
    assert cand.counts[:2] == [k, k] and max(cand.counts[2:]) < k and min(cand.passed[:2]) > k
    radius = [float(cfg["min_radius"][t]) for t in range(2) for _ in range(2)]
    keep, n_keep = nms.circle_nms_batched(cand.boxes, cand.segments, cand.counts, radius, 83)
    want = []
    for b in range(2):
        rows = torch.cat([cand.offsets[t * 2 + b] + keep[t * 2 + b, :n_keep[t * 2 + b]] for t in range(2)])
        want.append(dict(box3d_lidar=cand.boxes[rows], scores=cand.scores[rows], label_preds=cand.labels[rows]))
    _assert_equals_predict(det, want, "overflow")


def _same(got, want, what):
    """the bars of test_center_predict_gpu.py: labels, box count and keep order exactly; scores rtol 1e-5; boxes rtol 1e-4, atol 2e-4"""
    assert len(got) == len(want), what
    for i, (g, r) in enumerate(zip(got, want)):
        g = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in g.items()}
        assert g["box3d_lidar"].shape == r["box3d_lidar"].shape, (what, i, g["box3d_lidar"].shape, r["box3d_lidar"].shape)
        assert g["label_preds"].dtype == np.int64 and g["scores"].dtype == np.float32 and g["box3d_lidar"].dtype == np.float32
        assert np.array_equal(g["label_preds"], r["label_preds"]), (what, i)
        np.testing.assert_allclose(g["scores"], r["scores"], rtol=1e-5, err_msg=f"{what} {i}")
        np.testing.assert_allclose(g["box3d_lidar"], r["box3d_lidar"], rtol=1e-4, atol=2e-4, err_msg=f"{what} {i}")


def test_static_matches_both_reference_goldens(golden_dir):
    from golden_util import PREDICT_FLIP_CIRCLE_CFG, predict_flip_circle_inputs
    from sparse2dense_amd import waymo_configs
    from sparse2dense_amd.registry import build_head
    cases = [(_head(SIX, True), U.predict_tasks_inputs(), U.CFG, "predict_tasks_flip_circle.npz"),
             (build_head(waymo_configs.centerpoint_voxelnet()["bbox_head"]).eval(), [predict_flip_circle_inputs()], PREDICT_FLIP_CIRCLE_CFG,
              "predict_flip_circle.npz")]
    for head, maps, cfg, name in cases:
        g = np.load(os.path.join(golden_dir, name))
        det, _ = head.predict_static({}, [{k: v.cuda() for k, v in p.items()} for p in maps], cfg)
        assert head.static_predict_calls == 1 and head.predict_paths == {"device": 0, "torch": 0}
        # the one-task fixture passes more than 4096 pixels per sample (overflow set): its 83 survivors are all found among the 4096 best
        assert det.overflow.tolist() == ([0] * 12 if len(maps) == 6 else [1, 1])
        _same(det.as_list(), [dict(box3d_lidar=g[f"boxes{i}"], scores=g[f"scores{i}"], label_preds=g[f"labels{i}"]) for i in range(int(g["samples"]))], name)


# ---- no host round trip, graph capture ------------------------------------------------------------------------------------------------------
def _plan(head, maps, cfg, max_candidates=4096):
    from sparse2dense_amd import center_predict
    images, _, h, w = maps[0]["hm"].shape
    samples = images // 4 if cfg["double_flip"] else images
    return center_predict.StaticPredictPlan(cfg, head.num_classes, samples, h, w, "vel" in maps[0], maps[0]["hm"].device, max_candidates)


@pytest.mark.parametrize("circular", [False, True], ids=["rotated", "circular"])
def test_run_neither_synchronises_nor_allocates(circular):
    classes = SIX
    head = _head(classes)
    cfg = _cfg(6, True, circular)
    maps = _maps(classes, 14, True)
    plan = _plan(head, maps, cfg)
    out = plan.run(maps)   # warm-up: code objects loaded
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in plan.buffers().items()}
    assert set(ptrs) >= {"score", "label", "passed", "order", "score_sorted", "table", "cand_boxes", "keep", "n_keep", "nms_ws", "boxes", "counts"}
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = plan.run(maps)
        again = plan.run(maps)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert again is out and {k: v.data_ptr() for k, v in plan.buffers().items()} == ptrs
    _assert_equals_predict(out, head.predict({}, maps, cfg))


def test_one_captured_graph_replays_on_new_maps():
    classes = SIX[:3]
    head = _head(classes)
    cfg = _cfg(3, True, False)
    fresh = lambda i: _maps(classes, 20 + i, True, task_peaks=[150, 0 if i == 3 else 150, 150])   # replay 3 empties task 1's segments
    static = [{k: v.clone() for k, v in p.items()} for p in fresh(0)]
    plan = _plan(head, static, cfg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            plan.run(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = plan.run(static)
    for i in range(6):   # DESIGN rule 32's defect showed from the fourth replay on
        maps = fresh(i)
        for dst, src in zip(static, maps):
            for k in dst:
                dst[k].copy_(src[k])
        graph.replay()
        torch.cuda.synchronize()
        want = head.predict({}, maps, cfg)
        _assert_equals_predict(out, want, f"replay {i}")
        assert out.counts.tolist() == [len(w["scores"]) for w in want] and min(out.counts.tolist()) > 0
        if i == 3:
            assert out.overflow.tolist() == [1, 1, 0, 0, 1, 1]
