"""SECOND anchor head on the device (csrc/anchor_head.hip through sparse2dense_amd/anchors.py and heads.MultiGroupHead) against the
reference's numbers (tests/golden/anchor_*.npz, tests/golden/make_golden_anchor.py) and against the float64 / vectorised restatements
of tests/anchor_util.py (which tests/test_anchor_head_cpu.py pins to the same fixtures)."""
import copy
import os

import numpy as np
import pytest
import torch

import anchor_util as AU
from sparse2dense_amd import anchors as A, waymo_configs as WC
from sparse2dense_amd.registry import build_detector, build_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold(golden_dir):
    return {k: np.load(os.path.join(golden_dir, f"anchor_{k}.npz")) for k in ("targets", "loss", "predict")}


@pytest.fixture(scope="module")
def table():
    return A.get_assigner(WC.SECOND_ASSIGNER).anchors_numpy([1, AU.H, AU.W])


def _assign(boxes, classes):
    out = A.assign_anchor_targets(torch.from_numpy(boxes).to(DEV), torch.from_numpy(classes).to(DEV), WC.SECOND_ASSIGNER)
    return out, [out[k][0].cpu().numpy() for k in ("labels", "reg_targets", "reg_weights")]


def test_assignment_vs_reference(gold, table):
    g = gold["targets"]
    labels, targets, weights = AU.golden_targets(g)
    out, (lab, tgt, w) = _assign(g["boxes"], g["classes"])
    assert out["anchors"][0].shape == (3, AU.A, 7) and np.array_equal(out["anchors"][0][1].cpu().numpy(), table)
    assert lab.dtype == np.int32 and lab.shape == labels.shape
    for f in range(3):
        print(f"frame {f}: label mismatches {(lab[f] != labels[f]).sum()}, weight mismatches {(w[f] != weights[f]).sum()}, "
              f"max target error {np.abs(tgt[f] - targets[f]).max():.3e}")
    assert np.array_equal(lab, labels)            # every anchor of every frame
    assert np.array_equal(w, weights)
    np.testing.assert_allclose(tgt, targets, rtol=1e-4, atol=1e-5)
    assert np.all(tgt[lab <= 0] == 0)
    # the batch == each frame alone, bit for bit (with its own padding width); two runs bit-equal
    for f in range(3):
        k = max(int((g["classes"][f] > 0).sum()), 1)
        _, (lab1, tgt1, w1) = _assign(g["boxes"][f:f + 1, :k].copy(), g["classes"][f:f + 1, :k].copy())
        assert np.array_equal(lab1[0], lab[f]) and np.array_equal(tgt1[0], tgt[f]) and np.array_equal(w1[0], w[f])
    _, (lab2, tgt2, w2) = _assign(g["boxes"], g["classes"])
    assert np.array_equal(lab2, lab) and np.array_equal(tgt2, tgt) and np.array_equal(w2, w)
    # the float64 restatement the next test uses gives the same on this device as on the host (where the CPU tests pin it)
    asg = A.get_assigner(WC.SECOND_ASSIGNER)
    rl, rt, rw = AU.assign_restatement(torch.from_numpy(g["boxes"]).to(DEV), torch.from_numpy(g["classes"]).to(DEV),
                                             torch.from_numpy(table).to(DEV), [float(v) for v in asg.matched], [float(v) for v in asg.unmatched])
    assert np.array_equal(rl.cpu().numpy(), labels) and np.array_equal(rw.cpu().numpy(), weights)
    np.testing.assert_allclose(rt.cpu().numpy(), targets, rtol=1e-4, atol=1e-5)


def test_assignment_at_benchmark_shape(table):
    """B = 4, K = 200 boxes per frame drawn by the scene generator, against the vectorised float64 restatement
    (tests/anchor_util.assign_restatement, run on the device: the CPU tests and the previous test pin it to the reference's labels)"""
    from sparse2dense_amd import scene
    asg = A.get_assigner(WC.SECOND_ASSIGNER)
    frames = []
    for b in range(4):
        sc = scene.make_scene(2000, seed=300 + b, n_cars=133, n_peds=54)   # 133 + 54 + 13 = 200 boxes
        frames.append((sc["gt_boxes"][:, [0, 1, 2, 3, 4, 5, 8]].astype(np.float32), sc["gt_classes"].astype(np.int32)))
    boxes, classes = AU.pad_frames(frames)
    assert boxes.shape == (4, 200, 7)
    _, (lab, tgt, w) = _assign(boxes, classes)
    ref = AU.assign_restatement(torch.from_numpy(boxes).to(DEV), torch.from_numpy(classes).to(DEV), torch.from_numpy(table).to(DEV),
                                      [float(v) for v in asg.matched], [float(v) for v in asg.unmatched])
    rl, rt, rw = [t.cpu().numpy() for t in ref]
    for b in range(4):
        print(f"frame {b}: positives {(rl[b] > 0).sum()}, ignored {(rl[b] < 0).sum()}, label mismatches {(rl[b] != lab[b]).sum()}")
    assert np.array_equal(lab, rl) and np.array_equal(w, rw)
    np.testing.assert_allclose(tgt, rt, rtol=1e-4, atol=1e-5)


def _loss_case(gold, table, frames=(0, 1), grad=True):
    labels, targets, _ = AU.golden_targets(gold["targets"])
    labels, targets = labels[list(frames)], targets[list(frames)]
    box, cls, dirs = AU.loss_inputs(len(frames))
    dev = [t.to(DEV).requires_grad_(grad) for t in (box, cls, dirs)]
    tg = (torch.from_numpy(labels).to(DEV), torch.from_numpy(targets).to(DEV), torch.from_numpy(table).to(DEV))
    return labels, targets, (box, cls, dirs), dev, tg


def test_loss_forward_vs_reference(gold, table):
    g = gold["loss"]
    _, _, _, dev, tg = _loss_case(gold, table, grad=False)
    ret = A.anchor_loss(*dev, *tg, AU.LOSS_PARAMS)
    for k in A.LOSS_KEYS:
        print(k, float(ret[k]), float(g[k]))
        np.testing.assert_allclose(float(ret[k]), float(g[k]), rtol=1e-4, err_msg=k)
    np.testing.assert_allclose([float(v) for v in ret["loc_loss_elem"]], g["loc_loss_elem"], rtol=1e-4)
    assert int(ret["num_pos"]) == int(g["num_pos"]) and int(ret["num_neg"]) == int(g["num_neg"])


def test_loss_backward_vs_float64(gold, table):
    g = gold["loss"]
    labels, targets, cpu_in, dev, tg = _loss_case(gold, table)
    ret = A.anchor_loss(*dev, *tg, AU.LOSS_PARAMS)
    (ret["loss"] * 1.0).backward()
    ref_in = [t.double().requires_grad_(True) for t in cpu_in]
    ref = AU.loss_restatement(*ref_in, torch.from_numpy(labels), torch.from_numpy(targets), torch.from_numpy(table))
    ref["loss"].backward()
    np.testing.assert_allclose(ret["loss"].item(), ref["loss"].item(), rtol=1e-4)
    flat = labels.reshape(-1)
    pos, neg, ign = np.flatnonzero(flat > 0), AU.negative_sample(labels), np.flatnonzero(flat < 0)
    first = {}
    for name, t, r, width in (("box", dev[0], ref_in[0], 7), ("cls", dev[1], ref_in[1], 3), ("dir", dev[2], ref_in[2], 2)):
        got, want = t.grad.cpu().reshape(-1, width).numpy(), r.grad.reshape(-1, width).numpy()
        bar = 1e-4 * np.abs(want).max()
        print(f"d{name}: max |g64| {np.abs(want).max():.3e}, max error {np.abs(got - want).max():.3e} (bar {bar:.3e})")
        assert np.abs(got - want).max() <= bar, name
        gbar = 1e-4 * float(g[f"d{name}_absmax"])
        assert np.abs(got[pos] - g[f"d{name}_pos"]).max() <= gbar and np.abs(got[neg] - g[f"d{name}_neg"]).max() <= gbar, name
        assert len(ign) > 0 and np.all(got[ign] == 0), name
        first[name] = got
    # two runs bit-equal (forward scalars and gradients)
    dev2 = [t.detach().clone().requires_grad_(True) for t in dev]
    ret2 = A.anchor_loss(*dev2, *tg, AU.LOSS_PARAMS)
    ret2["loss"].backward()
    assert all(torch.equal(ret[k], ret2[k]) for k in A.LOSS_KEYS)
    for name, t, width in (("box", dev2[0], 7), ("cls", dev2[1], 3), ("dir", dev2[2], 2)):
        assert np.array_equal(t.grad.cpu().reshape(-1, width).numpy(), first[name]), name


def test_loss_frame_without_positives_is_finite(gold, table):
    labels, targets, cpu_in, dev, tg = _loss_case(gold, table, frames=(2, 0))   # frame 2 is empty: the clamp(min=1) path
    ret = A.anchor_loss(*dev, *tg, AU.LOSS_PARAMS)
    ret["loss"].backward()
    assert int(ret["num_pos"]) == 0 and int(ret["num_neg"]) == AU.A
    assert all(torch.isfinite(ret[k]).item() for k in A.LOSS_KEYS) and all(torch.isfinite(t.grad).all().item() for t in dev)
    ref = AU.loss_restatement(*[t.double() for t in cpu_in], torch.from_numpy(labels), torch.from_numpy(targets), torch.from_numpy(table))
    for k in A.LOSS_KEYS:
        np.testing.assert_allclose(ret[k].item(), float(ref[k]), rtol=1e-4, err_msg=k)


def test_predict_vs_reference(gold, table):
    g = gold["predict"]
    head = build_head(WC.second_voxelnet_train()["bbox_head"]).to(DEV)
    box, cls, dirs = [t.to(DEV) for t in AU.predict_inputs(2)]
    anchors = torch.from_numpy(table).to(DEV)
    boxes, scores, labels, dlab, keep = A.decode_anchors(box, cls, dirs, anchors, WC.SECOND_TEST_CFG["score_threshold"])
    for i in range(2):
        idx = torch.nonzero(keep[i]).reshape(-1)
        assert np.array_equal(idx.cpu().numpy(), g[f"cand_index_{i}"])
        assert np.array_equal(labels[i][idx].cpu().numpy(), g[f"cand_labels_{i}"])
        assert np.array_equal(dlab[i][idx].cpu().numpy(), g[f"cand_dir_{i}"])
        np.testing.assert_allclose(boxes[i][idx].cpu().numpy(), g[f"cand_boxes_{i}"], rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(scores[i][idx].cpu().numpy(), g[f"cand_scores_{i}"], rtol=1e-5)
    example = dict(anchors=[anchors.unsqueeze(0).expand(2, -1, -1)], metadata=[dict(token="a"), dict(token="b")])
    rets = head.predict(example, [dict(box_preds=box, cls_preds=cls, dir_cls_preds=dirs)], WC.SECOND_TEST_CFG)
    assert len(rets) == 2
    for i, r in enumerate(rets):
        assert set(r) == {"box3d_lidar", "scores", "label_preds", "metadata"} and r["metadata"] == example["metadata"][i]
        # the keep set, identified by the (untied) scores, in the same order
        np.testing.assert_allclose(r["scores"].cpu().numpy(), g[f"scores_{i}"], rtol=1e-5)
        assert np.array_equal(r["label_preds"].cpu().numpy(), g[f"label_preds_{i}"]) and r["label_preds"].dtype == torch.int64
        np.testing.assert_allclose(r["box3d_lidar"].cpu().numpy(), g[f"box3d_lidar_{i}"], rtol=1e-4, atol=2e-4)


def test_second_detector_trains_and_tests(table):
    """SECOND on the 8 k-point scene, B = 2, fp32 mode: the HIP loss equals the float64 restatement on the same raw predictions; five
    optimizer steps track the same steps taken with the fp32 torch restatement as the head's loss; predict and use_hip_graphs run."""
    from golden_util import fill_params
    from sparse2dense_amd.data import SyntheticFrames
    from sparse2dense_amd.solver import OneCycleAdam
    from sparse2dense_amd.train_step import backward_and_step, single_stage_loss
    frames = SyntheticFrames(2, n_points=8000, seed=7, device=DEV, anchor_targets=WC.SECOND_ASSIGNER)
    ex = frames.example()
    assert ex["labels"][0].shape == (2, AU.A) and int((ex["labels"][0] > 0).sum()) > 0
    model = fill_params(build_detector(WC.second_voxelnet_train(), test_cfg=WC.SECOND_TEST_CFG)).to(DEV).train()
    start = copy.deepcopy(model.state_dict())
    anchors = torch.from_numpy(table).to(DEV)

    # (a) loss == float64 restatement on the raw predictions of the same forward
    seen = {}
    head_loss = model.bbox_head.loss

    def spy(example, preds, **kw):
        seen["preds"] = {k: v.detach() for k, v in preds[0].items()}
        return head_loss(example, preds, **kw)
    model.bbox_head.loss = spy
    losses = model(ex, return_loss=True)
    p = seen["preds"]
    ref = AU.loss_restatement(p["box_preds"], p["cls_preds"], p["dir_cls_preds"], ex["labels"][0], ex["reg_targets"][0], anchors)
    for k in A.LOSS_KEYS:
        np.testing.assert_allclose(losses[k][0].item(), float(ref[k]), rtol=1e-4, err_msg=k)
    model.bbox_head.loss = head_loss

    # (b) five optimizer steps, HIP loss vs the fp32 torch restatement as the head's loss, from the same initial state
    def run(loss_fn):
        model.load_state_dict(start)
        model.bbox_head.loss = loss_fn
        params = [q for q in model.parameters() if q.requires_grad]
        # The step size is chosen so that the reference's own spread sits far below the 1e-3 bar.  Adam's normalised update turns
        # rounding-level gradient differences into O(lr) parameter differences, and this model starts in a violent transient (loss 642
        # -> ~500 in five steps).  Measured over five steps from this state: at lr 3e-4 the torch fp32 and torch float64 losses already
        # differ by 2.4e-3 from each other and one implementation differs from itself run to run by 1e-4 (the sparse backward's atomics);
        # at lr 1e-5 those figures are 4.8e-6 and 1.9e-5, HIP vs torch fp32 4.6e-5, and the loss still falls by 9 %.
        opt = OneCycleAdam(params, lr=1e-5, model=model)
        out = []
        for _ in range(5):
            loss, _ = single_stage_loss(model, ex)
            backward_and_step(loss, params, opt)
            assert all(q.grad is None or torch.isfinite(q.grad).all().item() for q in params)
            assert any(q.grad is not None for q in model.neck.parameters()) and any(q.grad is not None for q in model.backbone.parameters())
            out.append(float(loss))
        return out

    def torch_loss(example, preds, **kw):
        q = preds[0]
        r = AU.loss_restatement(q["box_preds"], q["cls_preds"], q["dir_cls_preds"], example["labels"][0], example["reg_targets"][0], anchors,
                                dtype=torch.float32)
        return {k: [v] for k, v in r.items()}
    hip, eager = run(head_loss), run(torch_loss)
    model.bbox_head.loss = head_loss
    print("per-step loss, HIP:", hip, "torch fp32:", eager)
    assert all(np.isfinite(hip)) and hip[-1] < hip[0]
    for a, b in zip(hip, eager):
        assert abs(a - b) <= 1e-3 * abs(b), (hip, eager)

    # (c) test path: per-sample dictionaries with the four keys; use_hip_graphs on this detector does not raise
    model.eval()
    with torch.no_grad():
        dets = model(ex, return_loss=False)
    assert len(dets) == 2 and all(set(d) == {"box3d_lidar", "scores", "label_preds", "metadata"} and d["box3d_lidar"].shape[1] == 7 for d in dets)
    model.train().use_hip_graphs()
    loss, _ = single_stage_loss(model, ex)
    loss.backward()
    model.eval()
    with torch.no_grad():
        assert len(model(ex, return_loss=False)) == 2
    assert torch.isfinite(loss).item()
