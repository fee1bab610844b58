"""The float64 definitions of the RoI head's training branch (second_stage.roi_mlp_train_reference, roi_loss_reference) against the
module's own training forward, its loss functions and autograd, the reference's recorded training step, the shape family and workspace
sizes of csrc/roi_mlp_train.hip and the reasons RoIHead.train_mlp_reason names - all without a GPU."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_util import fill_params, seeded
from roi_train_util import LOSS_CFG, SHAPES, TWO_ROWS, chain_mlp, check_step, draw_masks, head_cls_loss, layers_of, make_case, make_train_head, run_step
from sparse2dense_amd import _lib, registry, second_stage as S


def _close(a, b, what):
    """rtol 1e-12 per element; elements that cancel to (almost) nothing are held to 1e-12 of the tensor's largest"""
    a, b = a.detach().numpy(), b.detach().numpy()
    assert float(np.abs(b).max()) > 1e-6, what
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * float(np.abs(b).max()), err_msg=what)


def _objective(cls, reg):
    return (cls * seeded(cls.shape, 5).double()).sum() + (reg * seeded(reg.shape, 6).double()).sum()


@pytest.mark.parametrize("shared,cls,reg", [((64, 64), (64, 64), (64, 64)), ((64,), (), (48, 32)), ((32, 64), (16,), ())])
def test_reference_is_the_modules_own_training_forward_and_autograd_in_float64(shared, cls, reg):
    """DP_RATIO = 0: no shared site, Dropout(0) sites in the branches.  Pins the biased variance, eps, the layer order, the final biases, and
    the unbiased variance and momentum of the running statistics: depths (2, 2, 2), (1, 0, 2) and (2, 1, 0)"""
    head = make_train_head(40, shared, cls, reg, dp=0.0).double()
    assert [p for _, p in S.roi_mlp_train_sites(head)] == [0.0] * ((len(cls) > 0) + (len(reg) > 0))
    x = seeded((23, 40), 3).double()
    mine, theirs = copy.deepcopy(head), copy.deepcopy(head)
    got_cls, got_reg, stats = S.roi_mlp_train_reference(mine, x.reshape(1, 23, 40))   # leading dimensions are flattened
    ref_cls, ref_reg = chain_mlp(theirs, x)
    assert got_cls.shape == (23, 1) and got_reg.shape == (23, 7) and got_cls.dtype == torch.float64 and got_cls.grad_fn is not None
    _close(got_cls, ref_cls, "rcnn_cls"), _close(got_reg, ref_reg, "rcnn_reg")
    _objective(got_cls, got_reg).backward()
    _objective(ref_cls, ref_reg).backward()
    for (n, a), (_, b) in zip(mine.named_parameters(), theirs.named_parameters()):
        _close(a.grad, b.grad, n)
    hidden = [(a[1], b[1]) for a, b in zip(layers_of(mine), layers_of(theirs)) if a[1] is not None]
    assert len(stats) == len(hidden) == len(shared) + len(cls) + len(reg)
    for (mean, var), (a, b) in zip(stats, hidden):   # the definition leaves the module's statistics alone and returns what moves them
        _close((1 - a.momentum) * a.running_mean + a.momentum * mean, b.running_mean, "running_mean")
        _close((1 - a.momentum) * a.running_var + a.momentum * var, b.running_var, "running_var")
        assert int(a.num_batches_tracked) == 0 and int(b.num_batches_tracked) == 1


def test_reference_with_masks_is_the_modules_walk_with_dropout_replaced():
    """DP_RATIO = 0.3: one site behind the first shared layer (`> 0`, every shared layer but the last) and one behind the first hidden
    layer of each branch (`>= 0`)"""
    head = make_train_head(40, (64, 48), (32, 64), (64,), dp=0.3).double()
    assert S.roi_mlp_train_sites(head) == [(64, 0.3), (32, 0.3), (64, 0.3)]
    assert S.roi_mlp_train_sites(make_train_head(40, (64,), (), (64, 64))) == [(64, 0.3)]
    x, masks = seeded((19, 40), 4).double(), draw_masks(head, 19, 7)
    assert all(0 < float(m.mean()) < 1 for m in masks)
    mine, theirs = copy.deepcopy(head), copy.deepcopy(head)
    got, ref = S.roi_mlp_train_reference(mine, x, masks), chain_mlp(theirs, x, masks)
    _close(got[0], ref[0], "rcnn_cls"), _close(got[1], ref[1], "rcnn_reg")
    _objective(*got[:2]).backward()
    _objective(*ref).backward()
    for (n, a), (_, b) in zip(mine.named_parameters(), theirs.named_parameters()):
        _close(a.grad, b.grad, n)
    none = S.roi_mlp_train_reference(head, x)   # masks=None: no dropout
    ones = S.roi_mlp_train_reference(head, x, [torch.ones_like(m).double() * (1 - 0.3) for m in masks])
    _close(none[1], ones[1], "masks=None")
    assert float((none[1] - got[1]).detach().abs().max()) > 1e-3


def _loss_case(kind):
    rows = 24
    cls, reg = seeded((rows, 1), 21).double() * 2, seeded((rows, 7), 22).double()
    labels, fg, target = torch.rand((rows,), generator=torch.Generator().manual_seed(23)), (torch.arange(rows) % 3 == 0).long(), seeded((2, 12, 8), 24)
    if kind == "hard":
        labels = (torch.arange(rows) % 3 - 1).float()   # -1, 0, 1
    elif kind == "no fg":
        fg = torch.zeros(rows, dtype=torch.long)
    elif kind == "no valid":
        labels = -torch.ones(rows)
    elif kind == "saturated":
        cls = cls.clone()
        cls[3], cls[4], cls[5], cls[6] = 200.0, -200.0, 200.0, -200.0
        labels[3], labels[4], labels[5], labels[6] = 1.0, 0.0, 0.25, 0.75
    return cls, reg, labels, fg, target


@pytest.mark.parametrize("kind", ["soft", "hard", "no fg", "no valid", "saturated"])
def test_loss_reference_is_the_heads_own_losses_as_torch_computes_them(kind):
    """values and gradients, in fp32 (the head's loss functions cast to fp32 themselves), then the float64 definition against that.  A
    saturated logit has sigmoid exactly 0 or 1 in either dtype: the clamp of the logarithm at -100 gives the value, and torch's BCE
    backward gives a gradient of exactly zero there (not 0 * inf)"""
    dtype = torch.float32
    cls, reg, labels, fg, target = _loss_case(kind)
    head = make_train_head(40, (64,), (64,), (64,))
    outs = []
    for how in ("definition", "head"):
        c, r = cls.to(dtype).requires_grad_(), reg.to(dtype).requires_grad_()
        if how == "definition":
            lc, lr = S.roi_loss_reference(c, r, labels.reshape(2, 12), fg.reshape(2, 12), target.to(dtype), LOSS_CFG)
        else:
            ret = dict(rcnn_cls=c, rcnn_reg=r, rcnn_cls_labels=labels.to(dtype), reg_valid_mask=fg, gt_of_rois=target.to(dtype))
            lc, lr = head_cls_loss(head, ret), head.get_box_reg_layer_loss(ret)[0]
        (lc + lr).backward()
        outs.append((lc.detach(), lr.detach(), c.grad, r.grad))
    c, r = cls.clone().requires_grad_(), reg.clone().requires_grad_()
    lc, lr = S.roi_loss_reference(c, r, labels, fg, target.double(), LOSS_CFG)
    (lc + lr).backward()
    for a, b, d in zip(*outs, (lc.detach(), lr.detach(), c.grad, r.grad)):
        assert a.dtype == dtype and d.dtype == torch.float64 and torch.isfinite(a).all()
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(d.numpy(), b.numpy(), rtol=1e-5, atol=1e-7)
    lc, lr, dc, dr = outs[0]
    assert (float(lr) == 0 and float(dr.abs().max()) == 0) if kind == "no fg" else float(lr) > 0
    assert (float(lc) == 0 and float(dc.abs().max()) == 0) if kind == "no valid" else float(lc) > 0
    if kind == "saturated":
        assert torch.equal(dc[3:7], torch.zeros_like(dc[3:7])) and float(dc.abs().max()) > 0
        assert float(lc) > 100 * (0.75 + 0.75) / 24    # rows 3 and 4 (y = 1 / 0) cost nothing, rows 5 and 6 cost 100 (1 - y) and 100 y
    if kind == "hard":
        assert float(dc[::3].abs().max()) == 0 and float(dc[1::3].abs().min()) > 0


def test_reference_reproduces_the_reference_projects_training_step(golden_dir):
    """roi_training.npz through the CPU target assignment of test_second_stage.py, then the two definitions and autograd, in the fixture's fp32:
    the recorded outputs, both losses and the gradient of every parameter at that test's tolerances.  The fixture's logits reach 219:
    where fp32 rounds the sigmoid to 1 the recorded loss is the clamp's 100 (1 - y), which a float64 run would not reproduce."""
    from oracle import iou_nms as OI
    from test_second_stage import ROI_TRAIN_CFG, _check_roi_training
    g = np.load(os.path.join(golden_dir, "roi_training.npz"))
    roi = registry.build(dict(type="RoIHead", input_channels=40, code_size=7, model_cfg=ROI_TRAIN_CFG), registry.ROI_HEAD)
    fill_params(roi).train()
    roi.proposal_target_layer.iou_fn = lambda a, b: S.boxes_iou3d(a, b, bev_iou=lambda x, y: torch.from_numpy(OI.bev_iou(x.numpy(), y.numpy())))
    np.random.seed(int(g["np_seed"])); torch.manual_seed(int(g["torch_seed"]))
    t = lambda k: torch.from_numpy(g[k])
    batch = dict(rois=t("rois"), roi_labels=t("roi_labels"), roi_scores=t("roi_scores"), roi_features=t("roi_features"), gt_boxes_and_cls=t("gt"),
                 batch_size=2)
    ret = roi.assign_targets(batch)
    cls, reg, _ = S.roi_mlp_train_reference(roi, ret["roi_features"])
    assert float(cls.detach().abs().max()) > 200
    loss_cls, loss_reg = S.roi_loss_reference(cls, reg, ret["rcnn_cls_labels"], ret["reg_valid_mask"], ret["gt_of_rois"], ROI_TRAIN_CFG["LOSS_CONFIG"])
    total = loss_cls + loss_reg
    total.backward()
    ret["rcnn_cls"], ret["rcnn_reg"] = cls, reg
    _check_roi_training(g, roi, ret, total, dict(rcnn_loss_cls=loss_cls.detach(), rcnn_loss_reg=loss_reg.detach()), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape", SHAPES + [TWO_ROWS], ids=lambda s: f"cin{s[0]}-rows{s[4]}")
def test_the_gpu_parity_cases_meet_the_rules_conditions(shape):
    """the seeds of test_roi_train_gpu.py's parity cases are chosen here, where the float64 definition and the fp32 chain both run: every
    compared tensor has a finite, non-zero largest reference value and the chain is within 1e-3 of it"""
    cin, shared, cls, reg, rows, seed = shape
    head = make_train_head(cin, shared, cls, reg, seed=seed)
    case, masks = make_case(cin, rows, seed), draw_masks(head, rows, 31 + seed)
    check_step(run_step(head, case, masks, "ref"), run_step(head, case, masks, "chain"), None, data_grads=rows > 2, fused=False)


def test_shape_family_and_workspace_of_the_library():
    lib = _lib.load()   # loads without a GPU
    cfg = (2560, 2, 256, 256, 2, 256, 256, 2, 256, 256, 1, 7)
    ok = lambda *a: lib.s2d_roi_mlp_train_supported(*a)
    assert ok(*cfg, 512, 0.3) and ok(*cfg, 2, 0.0) and ok(*cfg, 8192, 0.99) and ok(40, 1, 64, 0, 0, 0, 0, 2, 48, 32, 1, 7, 17, -1.0)
    assert not ok(*cfg, 1, 0.3) and not ok(*cfg, 8193, 0.3) and not ok(*cfg, 0, 0.3) and not ok(*cfg, 512, 1.0) and not ok(*cfg, 512, float("nan"))
    for bad in [(42, 1, 64, 0, 0, 0, 0, 0, 0, 0, 1, 7), (40, 3, 64, 64, 0, 0, 0, 0, 0, 0, 1, 7), (40, 2, 64, 200, 0, 0, 0, 0, 0, 0, 1, 7),
                (40, 1, 64, 0, 0, 0, 0, 0, 0, 0, 1, 9), (40, 1, 64, 0, 0, 0, 0, 0, 0, 0, 3, 7)]:
        assert not ok(*bad, 64, 0.3), bad
    size = lambda plan, rows: lib.s2d_roi_mlp_train_scratch_bytes(ctypes.byref(plan), rows)
    plan = _lib.RoiMlpPlan()
    assert size(plan, 64) == 0                                         # not a plan of s2d_roi_mlp_plan_make
    _lib.check(lib.s2d_roi_mlp_plan_make(120, 2, 64, 32, 1, 48, 0, 0, 0, 0, 1, 7, ctypes.byref(plan)))
    assert size(plan, 1) == size(plan, 0) == size(plan, 8193) == size(plan, -5) == 0
    # per hidden layer: z and dy [rows][w], per-tile (mean, M2) and (S1, S2) [tiles][2][w], (mean, invstd) [2][w]
    want = lambda rows: 4 * sum(2 * rows * w + 4 * ((rows + 15) // 16) * w + 2 * w for w in (64, 32, 48))
    sizes = [size(plan, rows) for rows in range(2, 100)]
    assert sizes == [want(rows) for rows in range(2, 100)] and all(b > a for a, b in zip(sizes, sizes[1:]))
    _lib.check(lib.s2d_roi_mlp_plan_make(*cfg, ctypes.byref(plan)))
    assert size(plan, 8192) == 4 * 6 * (2 * 8192 * 256 + 4 * 512 * 256 + 2 * 256)
    fwd, bwd = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.s2d_roi_mlp_train_launches(ctypes.byref(plan), ctypes.byref(fwd), ctypes.byref(bwd)))
    assert (fwd.value, bwd.value) == (5, 8)   # + weight pack, mask draw, counter bump, loss forward, loss backward: 18, under the plan's 24
    plan.layer[1].cout = 250
    assert size(plan, 64) == 0


def test_train_mlp_reason_names_what_keeps_the_torch_chain(monkeypatch):
    monkeypatch.delenv("S2D_ROI_MLP", raising=False)
    x = torch.zeros(4, 40)
    head = make_train_head(40, (64, 64), (64, 64), (64, 64))
    assert head.fused_training is False and head.train_paths == {"fused": 0, "torch": 0}
    assert "CPU tensor" in head.train_mlp_reason(x)
    assert "training mode" in head.mlp_reason(x)                       # the eval kernel's reason is unchanged
    dev = torch.device("cuda", 0)
    why = lambda h, dtype=torch.float32, channels=40, rows=64, device=torch.device("cpu"), grad=False: h._train_mlp_check_for(True, dtype, channels, rows,
                                                                                                                           device, grad)[0]
    assert why(head) is None
    assert "feature dtype torch.bfloat16" in why(head, dtype=torch.bfloat16)
    assert "44 feature channels" in why(head, channels=44)
    assert "1 rows (2 .. 8192" in why(head, rows=1) and "8193 rows" in why(head, rows=8193) and why(head, rows=2) is None and why(head, rows=8192) is None
    assert "another device or not fp32" in why(head, device=dev) and "another device or not fp32" in why(copy.deepcopy(head).double())
    assert "require a gradient" in why(head, grad=True)
    with torch.no_grad():
        assert "grad mode is disabled" in why(head)
    assert "eval mode" in why(copy.deepcopy(head).eval())
    assert "width 200" in why(make_train_head(40, (64, 200), (64,), (64,)))
    assert "3 shared layers" in why(make_train_head(40, (64, 64, 64), (64,), (64,)))
    assert "42 input channels" in why(make_train_head(42, (64,), (), ()), channels=42)
    assert "DP_RATIO 1.0" in why(make_train_head(40, (64,), (64,), (64,), dp=1.0))
    assert "CrossEntropy / L1 losses" in why(make_train_head(40, (64,), (64,), (64,), LOSS_CONFIG=dict(LOSS_CFG, CLS_LOSS="CrossEntropy")))
    assert "smooth-l1" in why(make_train_head(40, (64,), (64,), (64,), LOSS_CONFIG=dict(LOSS_CFG, REG_LOSS="smooth-l1")))
    odd = copy.deepcopy(head)
    odd.shared_fc_layer[1].momentum = None
    assert "without momentum" in why(odd)
    code9 = registry.build(dict(type="RoIHead", input_channels=40, code_size=9, model_cfg=dict(head.model_cfg)), registry.ROI_HEAD).train()
    assert "code_size 9" in why(code9)
    monkeypatch.setenv("S2D_ROI_MLP", "0")
    assert why(head) == "S2D_ROI_MLP=0"
    with pytest.raises(_lib.S2DError, match="S2D_ROI_MLP=0"):
        S.roi_mlp_train_fused(head, x)   # the direct entry has no fallback
    monkeypatch.delenv("S2D_ROI_MLP")
    with pytest.raises(_lib.S2DError, match="CPU tensor"):
        S.roi_mlp_train_fused(head, x)
    with pytest.raises(_lib.S2DError, match="CrossEntropy"):
        S.roi_loss_fused(x[:, :1], torch.zeros(4, 7), x[:, 0], x[:, 0], torch.zeros(4, 7), dict(LOSS_CFG, CLS_LOSS="CrossEntropy"))
    # the switch changes nothing off the device path: a CPU training forward keeps the torch chain and says why
    assert head.mlp_paths == {"fused": 0, "torch": 0} and head.train_paths == {"fused": 0, "torch": 0}
